"""GPU: the initialisation search (include/oslam_hip.h, "Initialisation search") against the sequential numpy restatement of tests/search_init_common.py — every
entry of matches12, the carried points bit for bit and every count, no tolerance — against hand-written answers and against the truth of generated problems."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import search_init_common as sic
from object_slam_amd import search_init   # (at import: every test of this file needs the operator's module)
from object_slam_amd._lib import check, ptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "object_slam_amd")
FILL = -77            # the pattern the int output rows hold before a call
PREV_FILL = -1234.5   # the carried points of the rows no problem owns
GAP = 5               # frames-1 rows between the problems that no problem owns
f32 = np.float32


def _pack(problems, gap=GAP, prevs=None):
    """the records and flat arrays of a batch; the frames-1 rows of problem j start `gap` rows after those of problem j - 1 end, so that some rows belong to no problem"""
    f1c, f2, prev_c, off1, off2 = sic.concat_batch(problems)
    n = len(problems)
    if prevs is not None:
        prev_c = np.concatenate([np.asarray(p, f32).reshape(-1, 2) for p in prevs]) if n else prev_c
    out1 = off1 + gap * (1 + np.arange(n, dtype=np.int32))
    M1 = len(f1c["desc"]) + gap * (n + 1)
    f1, prev = sic.empty_rows(M1), np.full((M1, 2), PREV_FILL, f32)
    for p, a, o in zip(problems, off1, out1):
        k = len(p["f1"]["desc"])
        f1["keysUn"][o:o + k], f1["desc"][o:o + k], prev[o:o + k] = f1c["keysUn"][a:a + k], f1c["desc"][a:a + k], prev_c[a:a + k]
    pr = search_init.pack_problems([len(p["f1"]["desc"]) for p in problems], [len(p["f2"]["desc"]) for p in problems], [p["window"] for p in problems], out1, off2)
    return pr, f1, f2, prev


def _call(m, pr, f1, f2, prev, nnratio=sic.NNRATIO, check_ori=True, device=False):
    """the raw outputs of one call, over FILL; `prev` is not modified"""
    n, M1 = len(pr), len(f1["desc"])
    ints = lambda k: np.full(k, FILL, np.int32)
    return m.search_batch(pr, f1, f2, sic.BOUNDS, prev.copy(), nnratio=nnratio, check_orientation=check_ori, matches12=ints(M1), n_matches=ints(n), n_removed=ints(n),
                          n_displaced=ints(n), n_overflow=ints(n), device=device)


def _split(pr, raw):
    """per problem, in run_problem's form with the overflow count appended: (m12, prev, n, removed, displaced, overflow)"""
    return [(raw["matches12"][o:o + k].copy(), raw["prev_matched"][o:o + k].copy(), int(c), int(r), int(d), int(v))
            for o, k, c, r, d, v in zip(pr["off1"], pr["n1"], raw["n_matches"], raw["n_removed"], raw["n_displaced"], raw["n_overflow"])]


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same_one(x, y, upto=6):
    return np.array_equal(x[0], y[0]) and np.array_equal(_bits(x[1]), _bits(y[1])) and tuple(x[2:upto]) == tuple(y[2:upto])


def _same(a, b, upto=6):
    return len(a) == len(b) and all(_same_one(x, y, upto) for x, y in zip(a, b))


def _run(m, problems, nnratio, check_ori=True, device=False, prevs=None):
    pr, f1, f2, prev = _pack(problems, prevs=prevs)
    return _split(pr, _call(m, pr, f1, f2, prev, nnratio, check_ori, device))


@pytest.fixture(scope="module")
def matcher():
    m = search_init.InitMatcher(64, 2400, 20000)
    yield m
    m.close()


@pytest.fixture(scope="module")
def batches():
    """(check_orientation, nnratio) -> the problems of one call and the restatement's answers: nnratio is an argument of the call, so the hand cases with a ratio of
    their own get calls of their own.  (True, 0.9f): the generated problems, the one at the 2400-key capacity, n1 = 0, n2 = 0, both, and most hand cases.
    (False, 0.9f): the hand case without the check and three generated problems with the check switched off."""
    every = sic.batch_problems()
    groups = {}
    for p in every:
        groups.setdefault((p["check_ori"], float(p["nnratio"])), []).append(p)
    groups[(False, float(sic.NNRATIO))] += [dict(p, name=p["name"] + "_no_ori", check_ori=False) for p in every[:3]]
    main = groups[(True, float(sic.NNRATIO))]
    assert [p["name"] for p in main[:sic.N_GENERATED]] == [p["name"] for p in every[:sic.N_GENERATED]] and len(groups) == 5
    return {k: dict(problems=ps, ref=[r + (int((d["lines"] > sic.CACHE_CAP).sum()),) for r, d in sic.reference_of(ps, "gpu_%s_%s" % k)]) for k, ps in groups.items()}


@pytest.fixture(scope="module")
def first(matcher, batches):
    out = {}
    for (ori, ratio), b in batches.items():
        pr, f1, f2, prev = _pack(b["problems"])
        raw = _call(matcher, pr, f1, f2, prev, ratio, ori)
        out[(ori, ratio)] = dict(pr=pr, raw=raw, res=_split(pr, raw), prev_in=prev)
    return out


MAIN = (True, float(sic.NNRATIO))
OFF = (False, float(sic.NNRATIO))


def test_parity_with_the_restatement(batches, first):
    bad = []
    for key, b in batches.items():
        for p, ref, got in zip(b["problems"], b["ref"], first[key]["res"]):
            ndiff, pdiff = int((got[0] != ref[0]).sum()), int((_bits(got[1]) != _bits(ref[1])).sum())
            print("ori %d ratio %.2f %-26s n1 %4d n2 %4d nmatches %4d (restatement %4d) removed %3d (%3d) displaced %3d (%3d) overflow %2d (%2d), entries that differ: %d, carried "
                  "coordinates that differ: %d" % (key[0], key[1], p["name"], len(p["f1"]["desc"]), len(p["f2"]["desc"]), got[2], ref[2], got[3], ref[3], got[4], ref[4], got[5], ref[5],
                                                   ndiff, pdiff))
            if ndiff or pdiff or got[2:] != ref[2:]:
                bad.append((key, p["name"], ndiff, pdiff, got[2:], ref[2:]))
    assert not bad, bad
    res, g = first[MAIN]["res"], sic.N_GENERATED
    assert res[g - 1][2] > 500 and [r[2:] for r in res[g:g + 3]] == [(0, 0, 0, 0)] * 3
    assert all(r[2] >= 100 and r[3] >= 1 and r[4] >= 5 for r in res[:g]) and sum(r[5] for r in res[:g]) >= 1
    # without the orientation check nothing is removed; the loop is the same, so the displacements are, and the matches of the call with the check are among these
    for j, r in enumerate(first[OFF]["res"][-3:]):
        with_check = res[j]
        assert r[3] == 0 and r[2] == with_check[2] + with_check[3] and r[4] == with_check[4] and np.array_equal(r[0][with_check[0] >= 0], with_check[0][with_check[0] >= 0])


def test_rows_no_problem_owns_keep_their_fill(first):
    for key, f in first.items():
        m12, prev = f["raw"]["matches12"], f["raw"]["prev_matched"]
        owned = np.zeros(len(m12), bool)
        for o, n in zip(f["pr"]["off1"], f["pr"]["n1"]):
            assert not owned[o:o + n].any()
            owned[o:o + n] = True
        assert (~owned).sum() == GAP * (len(f["pr"]) + 1) and (m12[~owned] == FILL).all() and (m12[owned] != FILL).all() and (prev[~owned] == PREV_FILL).all()
        # the carried points of a key without a surviving match are untouched
        lost = owned & (m12 < 0)
        assert np.array_equal(_bits(prev[lost]), _bits(f["prev_in"][lost]))


def test_hand_built_cases_give_their_known_answers(batches, first):
    seen = 0
    for key, b in batches.items():
        for p, got in zip(b["problems"], first[key]["res"]):
            if "expect" not in p:
                continue
            e = p["expect"]
            seen += 1
            assert got[0].tolist() == list(e["m12"]) and got[2:5] == (e["n"], e["removed"], e["displaced"]), p["name"]
            if "prev" in e:
                assert np.array_equal(_bits(got[1]), _bits(np.array(e["prev"], f32))), p["name"]
            if "overflow" in e:
                assert got[5] == e["overflow"], p["name"]
    assert seen == len(sic.hand_cases())


def test_kernel_recovers_the_truth(batches, first):
    for p, got in zip(batches[MAIN]["problems"][:sic.N_GENERATED], first[MAIN]["res"]):
        want, found, false = sic.truth_score(p, got[0])
        assert want >= 100 and found * 10 >= want * 9 and false <= 2, (p["name"], want, found, false)


def test_problems_are_independent(matcher, batches, first):
    for key, b in batches.items():
        ori, ratio = key
        problems, res = b["problems"], first[key]["res"]
        assert _same(_run(matcher, problems[::-1], ratio, ori)[::-1], res)
        order = np.random.default_rng(3).permutation(len(problems))
        assert _same(_run(matcher, [problems[j] for j in order], ratio, ori), [res[j] for j in order])
        singles = range(len(problems)) if key != MAIN else list(range(0, sic.N_GENERATED, 2)) + list(range(sic.N_GENERATED, len(problems), 4))
        for j in singles:
            assert _same(_run(matcher, [problems[j]], ratio, ori), [res[j]]), problems[j]["name"]


def test_host_and_device_entry_points_agree_and_calls_repeat(matcher, batches, first):
    for key, b in batches.items():
        ori, ratio = key
        assert _same(_run(matcher, b["problems"], ratio, ori, device=True), first[key]["res"])
        assert _same(_run(matcher, b["problems"], ratio, ori), first[key]["res"])
    # one problem without keys: no rows at all but the gaps, so on the device path the frames-2 arrays are empty ones, which get a placeholder address
    empty = [dict(batches[MAIN]["problems"][0], name="no_rows", f1=sic.empty_rows(0), f2=sic.empty_rows(0), prev=np.zeros((0, 2), f32))]
    host = _run(matcher, empty, sic.NNRATIO)
    assert len(host) == 1 and host[0][2:] == (0, 0, 0, 0) and len(host[0][0]) == 0
    assert _same(_run(matcher, empty, sic.NNRATIO, device=True), host)


def test_optional_arrays_may_be_left_out(matcher, batches, first):
    """n_removed, n_displaced and n_overflow NULL at the C ABI: the other outputs are those of the full call"""
    pr, f1, f2, prev = _pack(batches[MAIN]["problems"][:2])
    M1 = len(f1["desc"])
    m12, n_matches = np.full(M1, FILL, np.int32), np.full(2, FILL, np.int32)
    r1 = search_init.F1Rows(M1, *[ptr(f1[k]) for k in search_init.ROW_KEYS])
    r2 = search_init.F2Rows(len(f2["desc"]), *[ptr(f2[k]) for k in search_init.ROW_KEYS])
    bnd = np.array(sic.BOUNDS, f32)
    check(matcher.L.oslam_match_search_for_initialization_batch(matcher.h, 2, ptr(pr), C.byref(r1), C.byref(r2), ptr(bnd), float(sic.NNRATIO), 1, ptr(prev), ptr(m12), ptr(n_matches),
                                                                None, None, None))
    for j, (o, n) in enumerate(zip(pr["off1"], pr["n1"])):
        want = first[MAIN]["res"][j]
        assert np.array_equal(m12[o:o + n], want[0]) and np.array_equal(_bits(prev[o:o + n]), _bits(want[1])) and n_matches[j] == want[2]


def test_second_call_starts_from_the_carried_points_of_the_first(matcher, batches, first):
    """the carried points of call 1 are the window centres of call 2 (a window of 30 pixels: a key that kept its own position no longer reaches a flow of 30 to 100
    pixels, a key that was matched finds its keypoint at the centre), as the restatement run twice says"""
    problems = [dict(p, window=30) for p in batches[MAIN]["problems"][:3]]
    res1 = first[MAIN]["res"][:3]
    got = _run(matcher, problems, sic.NNRATIO, prevs=[r[1] for r in res1])
    for p, r1, g in zip(problems, res1, got):
        want = sic.run_problem(p, prev=r1[1])
        own = sic.run_problem(p)
        print(p["name"], "call 2 from the carried points:", want[2], "from the keys' own positions:", own[2])
        assert _same_one(g, want, upto=5) and want[2] >= 100 and own[2] < want[2]


def test_matches_chain_into_the_initializer_on_one_stream(matcher, batches, first):
    """matches12 stays on the device and goes straight into oslam_init_initialize_batch_device on the same stream: the status and the pose are those of the host
    path fed the downloaded matches"""
    import torch
    from object_slam_amd import initializer
    from object_slam_amd._lib import upload
    problems = batches[MAIN]["problems"][:2]
    pr, f1, f2, prev = _pack(problems)
    M1, M2 = len(f1["desc"]), len(f2["desc"])
    xy = lambda f: np.ascontiguousarray(np.stack([f["keysUn"]["x"], f["keysUn"]["y"]], 1), f32)
    keys1, keys2 = xy(f1), xy(f2)
    ipr = initializer.pack_problems(pr["n1"], pr["n2"], problems[0]["scene"]["K"], 1.0, [2, 3], off1=pr["off1"], off2=pr["off2"])
    params = initializer.make_params()
    host_matches = _call(matcher, pr, f1, f2, prev)["matches12"]
    ini = initializer.Initializer(2, max(M1, M2), params.max_iterations)
    try:
        want = ini.initialize_batch(ipr, keys1, host_matches, keys2, params)
        out = dict(R21=np.zeros((2, 9), f32), t21=np.zeros((2, 3), f32), P3D=np.zeros((M1, 3), f32), tri=np.zeros(M1, np.uint8), status=np.zeros((2, 8), np.int32),
                   scores=np.zeros((2, 4), f32))
        ins = dict(pr=pr, k1=f1["keysUn"], d1=f1["desc"], k2=f2["keysUn"], d2=f2["desc"], prev=prev.copy(), m12=np.full(M1, FILL, np.int32), count=np.full(2, FILL, np.int32),
                   ipr=ipr, keys1=keys1, keys2=keys2)
        t = {k: upload(v) for k, v in list(ins.items()) + list(out.items())}
        a = lambda k: t[k].data_ptr()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        stream = C.c_void_p(side.cuda_stream)
        r1, r2 = search_init.F1Rows(M1, a("k1"), a("d1")), search_init.F2Rows(M2, a("k2"), a("d2"))
        bnd = np.array(sic.BOUNDS, f32)
        with torch.cuda.stream(side):
            check(matcher.L.oslam_match_search_for_initialization_batch_device(matcher.h, 2, a("pr"), C.byref(r1), C.byref(r2), ptr(bnd), float(sic.NNRATIO), 1, a("prev"), a("m12"),
                                                                               a("count"), None, None, None, stream))
            check(ini.L.oslam_init_initialize_batch_device(ini.h, 2, a("ipr"), M1, a("keys1"), a("m12"), M2, a("keys2"), C.addressof(params), None, a("R21"), a("t21"), a("P3D"),
                                                           a("tri"), a("status"), a("scores"), None, None, None, None, stream))
        side.synchronize()
        back = lambda k, like: t[k].cpu().numpy()[:like.nbytes].view(like.dtype).reshape(like.shape)
        status = back("status", out["status"])
        print("status", status.tolist(), "host", want["status"].tolist())
        assert np.array_equal(back("m12", ins["m12"]), host_matches)
        assert np.array_equal(status, want["status"]) and (status[:, 2] >= 100).all()
        assert np.array_equal(_bits(back("R21", out["R21"])), _bits(want["R21"].reshape(2, 9))) and np.array_equal(_bits(back("t21", out["t21"])), _bits(want["t21"]))
        assert np.array_equal(_bits(back("scores", out["scores"])), _bits(want["scores"])) and np.array_equal(back("tri", out["tri"]), want["triangulated"])
    finally:
        ini.close()


def test_refusals(matcher, batches, first):
    from object_slam_amd._lib import OSLAM_E_CAPACITY, OSLAM_E_INVALID, OslamError
    problems, res = batches[MAIN]["problems"][:3], first[MAIN]["res"]
    pr, f1, f2, prev = _pack(problems)
    M1, M2 = len(f1["desc"]), len(f2["desc"])

    def neighbours_ok(raw, what):
        for j in (0, 2):
            assert _same([_split(pr, raw)[j]], [res[j]]), what

    with pytest.raises(OslamError) as ei:
        search_init.InitMatcher(4, 2401, 1000)
    assert ei.value.code == OSLAM_E_INVALID
    small, few = search_init.InitMatcher(2, 440, 20000), search_init.InitMatcher(4, 2400, M1 - 1)
    try:
        def refused(what, m, recs, code, device=False, nnratio=sic.NNRATIO):
            """the call raises `code` and leaves every output row as it was"""
            outs = [np.full(M1, FILL, np.int32)] + [np.full(len(recs), FILL, np.int32) for _ in range(4)]
            carried = prev.copy()
            with pytest.raises(OslamError) as ei:
                m.search_batch(recs, f1, f2, sic.BOUNDS, carried, nnratio=nnratio, matches12=outs[0], n_matches=outs[1], n_removed=outs[2], n_displaced=outs[3], n_overflow=outs[4],
                               device=device)
            assert ei.value.code == code, what
            assert all((a == FILL).all() for a in outs) and np.array_equal(_bits(carried), _bits(prev)), what

        def with_field(field, value):
            recs = pr.copy()
            recs[field][1] = value
            return recs

        for device in (False, True):
            refused("three problems, two allowed", small, pr, OSLAM_E_CAPACITY, device)
            refused("more frames-1 rows than max_keys1_total", few, pr, OSLAM_E_CAPACITY, device)
            for value in (0.0, np.nan, -0.5, np.inf):
                refused("nnratio %r" % value, matcher, pr, OSLAM_E_INVALID, device, nnratio=value)
        refused("an F2 of 433 to 510 keys, 440 allowed", small, pr[1:3], OSLAM_E_CAPACITY)
        refused("2401 keys", matcher, with_field("n2", 2401), OSLAM_E_CAPACITY)
        for field in ("n1", "n2"):
            refused("negative " + field, matcher, with_field(field, -1), OSLAM_E_CAPACITY)
        for field, value in (("off1", M1), ("off2", M2), ("off1", -1), ("off2", -1), ("n1", M1 + 1)):
            refused("%s = %d outside" % (field, value), matcher, with_field(field, value), OSLAM_E_INVALID)
        refused("windowSize -1", matcher, with_field("windowSize", -1), OSLAM_E_INVALID)
    finally:
        small.close()
        few.close()
    # the device entry point cannot read the records: a record that does not fit gets -2 and nothing else
    for field, value in (("n1", -1), ("n2", -1), ("n2", 2401), ("off1", M1), ("off2", M2), ("off1", -1), ("n1", M1 + 1), ("windowSize", -1)):
        recs = pr.copy()
        recs[field][1] = value
        raw = _call(matcher, recs, f1, f2, prev, device=True)
        o, n = pr["off1"][1], pr["n1"][1]
        assert raw["n_matches"][1] == -2 and (raw["matches12"][o:o + n] == FILL).all() and np.array_equal(_bits(raw["prev_matched"][o:o + n]), _bits(prev[o:o + n])), (field, value)
        assert raw["n_removed"][1] == FILL and raw["n_displaced"][1] == FILL and raw["n_overflow"][1] == FILL, (field, value)
        neighbours_ok(raw, field)
    # windowSize 0 is taken: the strict window holds nothing
    recs = pr.copy()
    recs["windowSize"][1] = 0
    got = _split(pr, _call(matcher, recs, f1, f2, prev))[1]
    assert (got[0] == -1).all() and got[2:] == (0, 0, 0, 0) and np.array_equal(_bits(got[1]), _bits(prev[pr["off1"][1]:pr["off1"][1] + pr["n1"][1]]))


def _floats(line):
    return np.array([float.fromhex(v) for v in line.split()[1:]], f32)


def _ints(line):
    return np.array(line.split()[1:], np.int64)


def test_adapter_program_matches_the_restatement(tmp_path):
    from object_slam_amd import build
    build.build_hip()
    prog = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adapter_mono_init_program.cc"), "-o", prog,
                           "-L", LIBDIR, "-loslam_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    for tag in sic.SCENARIOS:
        s = sic.make_scenario(tag)
        d = str(tmp_path / tag)
        os.makedirs(d)
        for j, F in enumerate(s["frames"]):
            np.ascontiguousarray(F["keysUn"]).tofile(os.path.join(d, "keys_%d.bin" % j))
            np.ascontiguousarray(F["desc"]).tofile(os.path.join(d, "desc_%d.bin" % j))
        K = s["K"]
        with open(os.path.join(d, "meta.txt"), "w") as f:
            for k, v in dict(n_frames=len(s["frames"]), fx=K[0], fy=K[1], cx=K[2], cy=K[3], minX=sic.BOUNDS[0], minY=sic.BOUNDS[1], maxX=sic.BOUNDS[2], maxY=sic.BOUNDS[3],
                             iterations=200, seed=s["seed"]).items():
                f.write("%s %r\n" % (k, float(v)))
        r = subprocess.run([prog, d], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = [l for l in r.stdout.split("\n") if l]
        events = [l.split()[1] for l in lines if l.startswith("decision ")]
        print(tag, events, [l for l in lines if l.split()[0] in ("search", "nmatches", "triangulated")])
        assert events == s["events"], tag
        # every search, replayed by the restatement from the inputs the program printed
        reference, carried = None, None
        n_searches = 0
        for j, l in enumerate(lines):
            if l == "decision reference":
                reference = int([x for x in lines[:j] if x.startswith("frame ")][-1].split()[1])
                K1 = s["frames"][reference]["keysUn"]
                carried = np.stack([K1["x"], K1["y"]], 1).astype(f32)       # :654-656
            if not l.startswith("search "):
                continue
            n_searches += 1
            a, b = int(l.split()[1]), int(l.split()[2])
            before, n, after, prev_after = _floats(lines[j + 1]).reshape(-1, 2), int(lines[j + 2].split()[1]), _ints(lines[j + 3]), _floats(lines[j + 4]).reshape(-1, 2)
            assert a == reference and np.array_equal(_bits(before), _bits(carried)), tag      # the reference and the carried points are kept from frame to frame
            want = sic.search_for_initialization(s["frames"][a], s["frames"][b], before)
            assert np.array_equal(after, want[0]) and n == want[2] and np.array_equal(_bits(prev_after), _bits(want[1])), (tag, a, b, n, want[2])
            carried = prev_after
            decision = lines[j + 5] if lines[j + 5].startswith("decision ") else lines[-1]
            assert (decision == "decision few_matches") == (n < 100), tag       # :684
            if decision == "decision initialized":
                tri, ini = int(lines[j + 5].split()[1]), _ints(lines[j + 6])
                Tcw = _floats(lines[j + 7]).reshape(4, 4)
                assert lines[j + 5].startswith("triangulated ") and 50 <= tri <= n and tri == (ini >= 0).sum() and np.array_equal(ini[ini >= 0], after[ini >= 0])
                assert np.allclose(Tcw[:3, :3] @ Tcw[:3, :3].T, np.eye(3), atol=1e-4) and abs(np.linalg.norm(Tcw[:3, 3]) - 1.0) < 1e-4 and Tcw[3].tolist() == [0, 0, 0, 1]
        assert n_searches == sum(e in ("few_matches", "failed", "initialized") for e in events)
        if tag == "low_parallax":   # frame 3's windows were centred on frame 2's matches, which lie off the reference's keys
            K1 = s["frames"][0]["keysUn"]
            assert n_searches == 2 and not np.array_equal(before, np.stack([K1["x"], K1["y"]], 1).astype(f32))
