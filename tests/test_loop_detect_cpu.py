"""CPU: the conditions under which tests/test_loop_detect_gpu.py compares the loop detector (include/oslam_hip.h, "LoopClosing::DetectLoop") with the
restatement of tests/loop_detect_common.py element for element.  Conditions, not measurements: that the keyframe stream reaches every branch of
LoopClosing::DetectLoop (src/LoopClosing.cc:104-230), that none of its score comparisons is close enough for a float ulp to turn it, that the set form of
the consistency update the kernel computes equals the reference's nested loops, and that the ctypes mirrors have the sizes of the header's structs."""
import ctypes as C
import os
import subprocess

import keyframe_db_common as kc
import loop_detect_common as lc
from object_slam_amd import loop_detect   # (at import: every test of this file needs the operator's module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_stream_reaches_every_branch():
    steps, expected, ev = lc.revisit_fixture(0)
    assert len(steps) == len(expected) == lc.N_STREAM == 50
    print(dict(ev), "gated", sum(r["gated"] for r in expected), "loops", sum(r["ret"] for r in expected))
    assert sum(r["gated"] for r in expected) == 10                 # mnId < mLastLoopKFid + 10 (:115)
    assert ev["cleared"] >= 1                                      # no candidate (:145-151)
    assert ev["fresh"] >= 1                                        # a group that meets none, at 0 (:204-208)
    assert ev["enough_nonempty"] >= 1 and ev["enough_two_or_more"] >= 1
    assert ev["group_met_by_two_candidates"] >= 1                  # vbConsistentGroup (:189-194)
    assert ev["candidate_meets_two_groups"] >= 1
    assert 1 <= ev["max_groups"] <= loop_detect.MAX_GROUPS
    assert any(r["ret"] for r in expected) and not all(r["ret"] for r in expected if not r["gated"])
    # the derived bound is a connected keyframe's score wherever the keyframe has connections in the database, and 1 where it has none
    assert any(float(r["min_score"]) == 1.0 for r in expected if not r["gated"]) and any(float(r["min_score"]) < 1.0 for r in expected if not r["gated"])


def test_no_comparison_of_the_stream_is_within_the_margin():
    """A score of the device differs from the restatement's by at most one float ulp (tests/test_keyframe_db_gpu.py); 1e-5 relative is ~84 ulp."""
    for seed in (0, 1, 2):   # the seeds tests/test_loop_detect_gpu.py runs
        _, expected, _ = lc.revisit_fixture(seed)
        for r in expected:
            if not r["gated"]:
                assert kc.margin_violations(r["log"], 1e-5) == [], (seed, r["cand"])


def test_the_set_form_equals_the_nested_loops():
    n = n_nonempty = 0
    ev_all = lc.collections.Counter()
    for K in (40, 64, 70, 2048):
        cases, runs = lc.case_fixture(K)
        for case, (run, ev) in zip(cases, runs):
            ev_all.update(ev)
            for step in run:
                conn = lambda k, rows=step["rows"]: rows.get(k, set())   # noqa: E731
                nested, enough_n, _ = lc.update_consistency_nested(step["prev"], step["cands"], conn, case["th"])
                sets, enough_s = lc.update_consistency_sets(step["prev"], step["cands"], conn, case["th"])
                assert nested == sets and enough_n == enough_s, (K, case["name"], step["cands"])
                if step["n_enough"] == lc.REFUSED_CAPACITY:
                    assert len(nested) == case["max_groups"] + 1
                elif step["cands"]:
                    assert step["groups"] == [(sorted(g), c) for g, c in nested] and step["enough"] == enough_n
                n += 1
                n_nonempty += bool(step["prev"]) and bool(step["cands"])
            if case["name"] == "capacity":
                assert [s["n_enough"] for s in run].count(lc.REFUSED_CAPACITY) == 2 and max(len(s["groups"]) for s in run) == case["max_groups"]
            if case["name"] == "branches":
                assert any(len(s["cands"]) != len(set(s["cands"])) for s in run)                            # a repeated id
                assert any(s["cands"] == [] for s in run)
                assert any(K - 1 in g for s in run for g, _ in s["groups"]) and (K - 1) // 32 == (K + 31) // 32 - 1   # the last word
    print(n, n_nonempty, dict(ev_all))
    assert n_nonempty >= 40
    for what in ("fresh", "cleared", "enough_nonempty", "enough_two_or_more", "group_met_by_two_candidates", "candidate_meets_two_groups", "only_overlap_is_itself"):
        assert ev_all[what] >= 1, what


def test_ctypes_mirrors_have_the_sizes_of_the_header(tmp_path):
    pairs = [("oslam_loopdet_conn_t", loop_detect.Conn, loop_detect.CONN_DTYPE), ("oslam_loopdet_update_t", loop_detect.Update, loop_detect.UPDATE_DTYPE)]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "oslam_hip.h"\nint main(void) {\n' + "".join('    printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n, _, _ in pairs)
                   + '    printf("OSLAM_LOOPDET_MAX_GROUPS %d\\n", OSLAM_LOOPDET_MAX_GROUPS);\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    c_sizes = dict((l.split()[0], int(l.split()[1])) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, cls, dtype in pairs:
        assert C.sizeof(cls) == dtype.itemsize == c_sizes[name], (name, C.sizeof(cls), dtype.itemsize, c_sizes[name])
    assert loop_detect.MAX_GROUPS == c_sizes["OSLAM_LOOPDET_MAX_GROUPS"]
