"""CPU: the restatement of ORBmatcher::SearchForInitialization in tests/search_init_common.py against hand-built known answers and against the truth of generated
problems, so that the GPU tests may compare the kernel with it; what the generated parity batch exercises; the frame lists of the caller program; the ctypes
mirrors of include/oslam_hip.h, "Initialisation search"."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import initializer_common as ic
import search_init_common as sic
import sim3_match_common as smc
from object_slam_amd import search_init   # (at import: every test of this file belongs to the operator, also those that pin the restatement it is compared with)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in sic.hand_cases()}
f32 = np.float32


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_gives_the_known_answer(name):
    c = CASES[name]
    d = {}
    m12, prev, n, removed, displaced = sic.run_problem(c, d)
    e = c["expect"]
    print(name, m12.tolist(), n, removed, displaced)
    assert m12.tolist() == list(e["m12"]) and (n, removed, displaced) == (e["n"], e["removed"], e["displaced"])
    assert n == sum(1 for v in e["m12"] if v >= 0)
    # the carried points: the F2 key's position where a match survived, untouched elsewhere
    K2 = c["f2"]["keysUn"]
    want = np.array([(K2["x"][k], K2["y"][k]) if k >= 0 else tuple(c["prev"][i]) for i, k in enumerate(e["m12"])], f32).reshape(-1, 2)
    assert np.array_equal(prev, want, equal_nan=True)
    if "prev" in e:
        assert np.array_equal(prev, np.array(e["prev"], f32), equal_nan=True)
    if "overflow" in e:
        assert int((d["lines"] > sic.CACHE_CAP).sum()) == e["overflow"]


def test_hand_cases_are_what_their_comments_say():
    pop = lambda a, b: int(smc._POP[np.bitwise_xor(a, b)].sum())
    D1, D2 = (lambda c: c["f1"]["desc"]), (lambda c: c["f2"]["desc"])
    c = CASES["displacement"]
    assert [[pop(D1(c)[i], D2(c)[k]) for k in range(2)] for i in range(3)] == [[10, 56], [4, 50], [6, 40]]
    assert not f32(40) < f32(6) * f32(0.9) and f32(6) < f32(40) * f32(0.9)   # k as second best would reject c; k not skipped would take c
    c = CASES["equal_distance"]
    assert [pop(D1(c)[i], D2(c)[0]) for i in range(2)] == [5, 5]
    c = CASES["skipped_is_not_second"]
    assert [[pop(D1(c)[i], D2(c)[k]) for k in range(2)] for i in range(2)] == [[0, 41], [20, 21]] and not f32(21) < f32(20) * f32(0.9)
    c = CASES["th_low"]
    assert [pop(D1(c)[i], D2(c)[i]) for i in range(2)] == [50, 51]
    # the float product: 25 * 0.6f is the float after 15, 20 * 0.6f is 12 exactly; in double both products lie above
    c = CASES["ratio_float"]
    r = f32(0.6)
    assert c["nnratio"] == r and [pop(D1(c)[0], D2(c)[k]) for k in (0, 1)] == [15, 25] and [pop(D1(c)[1], D2(c)[k]) for k in (2, 3)] == [12, 20]
    assert f32(25) * r == np.nextafter(f32(15), f32(16)) and f32(20) * r == f32(12) and 20.0 * float(r) > 12.0 and 25.0 * float(r) > 15.0
    c = CASES["ratio_strict"]
    assert [pop(D1(c)[0], D2(c)[k]) for k in range(2)] == [20, 40] and f32(40) * c["nnratio"] == f32(20)
    c = CASES["window_edge"]
    K1, K2 = c["f1"]["keysUn"], c["f2"]["keysUn"]
    assert K2["x"][0] - K1["x"][0] == 100.0 and 0 < f32(100) - (K2["x"][1] - K1["x"][1]) < 1e-4 and K2["y"][2] - K1["y"][2] == 100.0 and 0 < f32(100) - (K1["y"][3] - K2["y"][3]) < 1e-4
    c = CASES["tie"]
    assert [pop(D1(c)[0], D2(c)[k]) for k in range(2)] == [10, 10] and c["nnratio"] == f32(1.5)
    px, py = smc._grid_cells(c["f2"]["keysUn"], sic.BOUNDS, f32(0.1), f32(0.1))
    assert (px.tolist(), py.tolist()) == ([11, 9], [9, 11])   # the column-first traversal reaches key 1 first; row-first, or index order, would reach key 0
    for name, n in sic.CACHE_CASES.items():
        c = CASES[name]
        assert len(D1(c)) == len(D2(c)) == n and all(pop(D1(c)[i], D2(c)[k]) == 3 * k + 1 for i in range(n) for k in range(n))
        assert all(f32(3 * j + 1) < f32(3 * j + 4) * f32(0.9) for j in range(n - 1)) and 3 * (n - 1) + 1 <= sic.TH_LOW
        d = {}
        sic.run_problem(c, d)
        assert (d["lines"] == n).all()
    assert sorted(sic.CACHE_CASES.values()) == [sic.CACHE_CAP, sic.CACHE_CAP + 1, 10]
    # the histogram pair differs in the displaced entry alone
    a, b = CASES["histo_with_displaced"], CASES["histo_without_displaced"]
    assert (a["f1"]["keysUn"]["octave"][0], b["f1"]["keysUn"]["octave"][0]) == (0, 1) and np.array_equal(a["f1"]["desc"], b["f1"]["desc"]) and sic.rot_bin(90.0, 0.0) == 3
    assert not f32(2) < f32(0.1) * f32(20) and f32(1) < f32(0.1) * f32(20)
    assert f32(15.0) * (f32(1.0) / f32(30)) == f32(0.5) and sic.rot_bin(15.0, 0.0) == 1 and (sic.rot_bin(165.0, 0.0), sic.rot_bin(285.0, 0.0)) == (6, 10)
    assert sic.rot_bin(10.0, 350.0) == 1 and sic.rot_bin(np.nan, 0.0) is None
    # the cut of the candidate lists at nnratio 0.9f: 55 can matter, 56 cannot; at 0.6f the cut is at 84
    assert sic.can_matter(55, 0.9) and not sic.can_matter(56, 0.9) and sic.can_matter(50, 1e-3) and sic.can_matter(83, 0.6) and not sic.can_matter(84, 0.6)


def test_generated_problems_exercise_the_operator():
    """On every generated problem the restatement alone reaches what the GPU parity test relies on: enough matches, displacements, histogram removals, a line
    beyond the kernel's cache, and the truth (a random descriptor is within 50 bits of another with probability 1e-23 per candidate)."""
    problems = sic.batch_problems()[:sic.N_GENERATED]
    overflow = 0
    for p, (r, det) in zip(problems, sic.reference_of(problems, "generated")):
        m12, prev, n, removed, displaced = r
        want, got, false = sic.truth_score(p, m12)
        n1, n2 = len(p["f1"]["desc"]), len(p["f2"]["desc"])
        oct0 = [int((p[f]["keysUn"]["octave"] == 0).sum()) for f in ("f1", "f2")]
        dont_care = int((p["truth"] == sic.DONT_CARE).sum())
        print("%s: n1 %d n2 %d octave-0 %s: %d of %d true matches, %d false, nmatches %d, removed %d, displaced %d, lines beyond the cache %d, DONT_CARE %d" % (
            p["name"], n1, n2, oct0, got, want, false, n, removed, displaced, int((det["lines"] > sic.CACHE_CAP).sum()), dont_care))
        assert n >= 100 and displaced >= 5 and removed >= 1
        assert got * 10 >= want * 9 and false <= 2 and dont_care * 100 <= 15 * p["n_findable"]
        assert min(oct0) >= 150 and n1 % 64 != 0 and n2 % 64 != 0
        overflow += int((det["lines"] > sic.CACHE_CAP).sum())
        # every planted displacement happened: the early key lost the F2 key to the pair's own key
        assert all(m12[e] == -1 and (m12[i1] == i2 or p["truth"][i1] == sic.DONT_CARE) for e, i1, i2 in p["planted"]) and displaced >= len(p["planted"])
        assert all(det["lines"][i] > sic.CACHE_CAP for i in p["crowded"])
        assert np.array_equal(prev[m12 < 0], p["prev"][m12 < 0]) and np.array_equal(prev[m12 >= 0, 0], p["f2"]["keysUn"]["x"][m12[m12 >= 0]])
    assert overflow >= 1
    assert all(300 <= len(p[f]["desc"]) <= 520 for p in problems[:-1] for f in ("f1", "f2"))
    full = problems[-1]
    assert len(full["f1"]["desc"]) == len(full["f2"]["desc"]) == search_init.MAX_KEYPOINTS == 2400
    assert min(int((full[f]["keysUn"]["octave"] == 0).sum()) for f in ("f1", "f2")) > 1024     # a thread of the workgroup holds two keys
    names = [p["name"] for p in sic.batch_problems()]
    assert {"n1_zero", "n2_zero", "both_zero"} <= set(names) and len(set(names)) == len(names)
    q = sic.make_problem(*sic.PARITY_SPECS[1])
    assert all(np.array_equal(q[f][k], problems[1][f][k]) for f in ("f1", "f2") for k in sic.ROW_KEYS) and np.array_equal(q["truth"], problems[1]["truth"])


def _track(frames, K, seed):
    """src/Tracking.cc:644-716 over the frames with the restatements: the events, and the searches as (reference, frame, prev before, result)"""
    events, searches = [], []
    ref, prev = None, None
    for j, F in enumerate(frames):
        n = len(F["desc"])
        if ref is None:
            if n > 100:
                ref, prev = j, np.stack([F["keysUn"]["x"], F["keysUn"]["y"]], 1).astype(f32)
                events.append("reference")
            else:
                events.append("idle")
            continue
        if n <= 100:
            ref = None
            events.append("few_keys")
            continue
        r = sic.search_for_initialization(frames[ref], F, prev)
        searches.append((ref, j, prev, r))
        prev = r[1]
        if r[2] < 100:
            ref = None
            events.append("few_matches")
            continue
        xy = lambda G: np.stack([G["keysUn"]["x"], G["keysUn"]["y"]], 1).astype(f32)
        out = ic.initialize(xy(frames[ref]), xy(F), r[0], K, sigma=1.0, seed=seed)
        assert not out["rec"]["near"]   # (no CheckRT test near its threshold: the operator decides as the restatement does)
        events.append("initialized" if out["returned"] else "failed")
        if out["returned"]:
            break
    return events, searches


@pytest.mark.parametrize("name", sic.SCENARIOS)
def test_scenarios_of_the_caller_program(name):
    """with both restatements in place of the operators, the frame lists take the paths they were built for"""
    s = sic.make_scenario(name)
    events, searches = _track(s["frames"], s["K"], s["seed"])
    print(name, events, [(a, b, r[2]) for a, b, _, r in searches])
    assert events == s["events"]
    if name == "low_parallax":
        # the second search starts from the carried points the first one left: those of its matches lie on frame 1's keys, not on the reference's
        (_, _, p0, r0), (ref, j, p1, r1) = searches
        assert ref == 0 and j == 2 and np.array_equal(p1, r0[1]) and (r0[0] >= 0).sum() >= 100 and not np.array_equal(p1, p0)
        own = sic.search_for_initialization(s["frames"][0], s["frames"][2], p0)
        assert r1[2] >= 100 and own[2] >= 100


def test_struct_mirrors_have_the_sizes_of_the_header(tmp_path):
    pairs = [("oslam_init_match_problem_t", search_init.Problem), ("oslam_init_match_f1_rows_t", search_init.F1Rows), ("oslam_init_match_f2_rows_t", search_init.F2Rows)]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "oslam_hip.h"\nint main(void) {\n' + "".join('    printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n, _ in pairs)
                   + '    printf("windowSize_at %zu\\ndesc1_at %zu\\ndesc2_at %zu\\n", offsetof(oslam_init_match_problem_t, windowSize), offsetof(oslam_init_match_f1_rows_t, desc), '
                   'offsetof(oslam_init_match_f2_rows_t, desc));\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    c_vals = dict((l.split()[0], int(l.split()[1])) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, cls in pairs:
        assert C.sizeof(cls) == c_vals[name], (name, C.sizeof(cls), c_vals[name])
    assert search_init.PROBLEM_DTYPE.itemsize == c_vals["oslam_init_match_problem_t"] == 24 and c_vals["oslam_init_match_problem_t"] % 8 == 0
    assert search_init.Problem.windowSize.offset == c_vals["windowSize_at"] == search_init.PROBLEM_DTYPE.fields["windowSize"][1] == 16
    assert search_init.F1Rows.desc.offset == c_vals["desc1_at"] and search_init.F2Rows.desc.offset == c_vals["desc2_at"]
    pr = search_init.pack_problems([3, 0, 5], [7, 2, 0], [100, 10, 0])
    assert pr["off1"].tolist() == [0, 3, 3] and pr["off2"].tolist() == [0, 7, 9] and pr["windowSize"].tolist() == [100, 10, 0]
    one = search_init.Problem.from_buffer_copy(pr[2].tobytes())
    assert (one.n1, one.off1, one.n2, one.off2, one.windowSize, one.reserved) == (5, 3, 0, 9, 0, 0)
    assert (search_init.NNRATIO, search_init.WINDOW_SIZE) == (0.9, 100) and f32(search_init.NNRATIO) == sic.NNRATIO and sic.WINDOW == 100


def test_library_exports_the_symbols():
    from object_slam_amd import build
    from object_slam_amd._lib import lib
    build.build_hip()
    L = lib()
    for name in ("oslam_init_match_create", "oslam_init_match_destroy", "oslam_match_search_for_initialization_batch", "oslam_match_search_for_initialization_batch_device"):
        assert hasattr(L, name), name
    import object_slam_amd
    assert object_slam_amd.InitMatcher is search_init.InitMatcher


def test_no_device_is_an_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from object_slam_amd._lib import OSLAM_E_HIP, OslamError
    with pytest.raises(OslamError) as ei:
        search_init.InitMatcher(4, 400, 1000)
    assert ei.value.code == OSLAM_E_HIP and "no CPU fallback" in str(ei.value)


def test_adapter_and_caller_program_compile():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adapter_mono_init_program.cc")])
