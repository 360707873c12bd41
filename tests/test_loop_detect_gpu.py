"""GPU: the loop detector (include/oslam_hip.h, "LoopClosing::DetectLoop") against the literal restatement of tests/loop_detect_common.py.  Everything discrete
— candidates and their order, the diagnostics row, the enough list, the groups' members, counters and order — is equal element for element, no case left
out.  Scores: conn_score and the derived min_score within 1 float ulp of the restatement (the bound of tests/test_keyframe_db_gpu.py: two summation orders
of a score differ by at most n_common * 2^-52 in fp64, far below half a float ulp); accumulated scores within its 11 ulp.  tests/test_loop_detect_cpu.py
asserts the margin condition that makes the discrete results comparable."""
import os
import subprocess

import numpy as np
import pytest

import keyframe_db_common as kc
import loop_detect_common as lc
import voc_common as V
from object_slam_amd import OslamError, keyframe_db, loop_detect   # (at import: every test of this file needs the operator's module)
from object_slam_amd._lib import OSLAM_E_INVALID
from object_slam_amd.vocabulary import Vocabulary, save_text

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "object_slam_amd")
TREE = V.make_tree(5, 4, 2)   # L1_NORM; the operators read nothing of a vocabulary but its scoring type
SEEDS = (0, 1, 2)
K_STREAM = 70


@pytest.fixture(scope="module")
def voc():
    return Vocabulary.from_arrays(*TREE.arrays())


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


# ---- 1. update_consistency against the restatement ----
def update(det, database, cands, device=False):
    """one update of one database: (n_enough, enough, n_groups)"""
    out = det.update_consistency(*loop_detect.pack_updates([database], [cands]), device=device)
    n = int(out["n_enough"][0])
    assert (out["enough"][0, max(n, 0):] == -1).all()   # nothing is written beyond the count
    return n, out["enough"][0, :max(n, 0)].tolist(), int(out["n_groups"][0])


def replay_case(det, database, case, run, device=False, steps=None):
    for i, ((upd, cands), exp) in enumerate(zip(case["steps"], run)):
        if steps is not None and i not in steps:
            continue
        where = (case["name"], case["K"], "step", i, cands)
        if upd:
            det.set_connected(*loop_detect.pack_connected([database] * len(upd), list(upd), list(upd.values())))
        before = det.get_groups(database)
        n, enough, n_groups = update(det, database, cands, device)
        print(where, "n_enough", n, "enough", enough, "groups", n_groups)
        assert n == exp["n_enough"] and enough == exp["enough"], where
        after = det.get_groups(database)
        assert after == exp["groups"], where
        if n < 0:
            assert after == before and n_groups == -9, where
        else:
            assert n_groups == len(exp["groups"]), where


@pytest.mark.parametrize("K", [40, 64, 70, 2048])
def test_update_consistency_equals_the_restatement(voc, K):
    """K = 40: two words, the last one partial; 64: two full words; 70: three; 2048: one word per lane, max_groups 64, a single database.  The capacity case
    runs with max_groups 4.  Host and device entry points, each on its own detector."""
    cases, runs = lc.case_fixture(K)
    n_db = 1 if K == 2048 else 3
    db = keyframe_db.KeyFrameDatabase(voc, n_db, K, 128, pool_words=1024)
    for case, (run, _) in zip(cases, runs):
        for device in (False, True):
            det = loop_detect.LoopDetector(db, case["max_groups"], case["th"])
            replay_case(det, n_db - 1, case, run, device)
            assert all(det.get_groups(d) == [] for d in range(n_db - 1))   # the other databases' groups are untouched
            det.close()
    db.close()


def test_set_connected_replaces_whole_rows_in_record_order(voc):
    """A keyframe named twice in one call keeps its last row; ids outside 0 .. K - 1 are skipped; a row replaces the one before it entirely."""
    K = 70
    db = keyframe_db.KeyFrameDatabase(voc, 2, K, 128, pool_words=1024)
    det = loop_detect.LoopDetector(db)
    det.set_connected(*loop_detect.pack_connected([1, 0, 1, 1], [5, 5, 5, 6], [[1, 2, 64], [9], [3, K, -1, K + 40, 69], list(range(K))]))
    assert update(det, 1, [5, 6]) == (0, [], 2) and det.get_groups(1) == [([3, 5, 69], 0), (list(range(K)), 0)]
    assert update(det, 0, [5]) == (0, [], 1) and det.get_groups(0) == [([5, 9], 0)]
    det.set_connected(*loop_detect.pack_connected([1], [6], [[]]))
    assert update(det, 1, [6]) == (0, [], 1) and det.get_groups(1) == [([6], 1)]   # its row is empty now: it met the previous group through itself only
    det.close(); db.close()


# ---- 2., 3., 6. detect over the keyframe stream ----
def run_stream(db, det, streams, device=False, cross=False, last_loop_at=None):
    """The streams of len(streams) databases in lockstep, as the caller of DetectLoop does it: rows and covisibility, the gate, detect, add.  Per keyframe a
    list with one dict per database (None while gated).  cross: also the kfdb's own loop query with min_score set to what detect returned."""
    D = list(range(len(streams)))
    out, last = [], 0
    for k in range(len(streams[0])):
        S = [streams[d][k] for d in D]
        kf = S[0]["kf"]
        if last_loop_at and kf == last_loop_at[0]:
            last = last_loop_at[1]
        rows = [(d, x, l) for d in D for x, l in S[d]["rows"]]
        det.set_connected(*loop_detect.pack_connected([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]))
        cv = [(d, x, l) for d in D for x, l in S[d]["covis"]]
        if cv:
            db.set_covisibility(keyframe_db.pack_covisibility([r[0] for r in cv], [r[1] for r in cv], [r[2] for r in cv]))
        res = None
        if not kf < last + 10:   # (:115)
            rec, ids, vals, conn = keyframe_db.pack_queries(D, [(s["ids"], s["vals"]) for s in S], connected=[s["conn"] for s in S])
            o = det.detect(rec, ids, vals, conn, device=device)
            x = None
            if cross:
                rec["min_score"] = o["min_score"]
                x = db.detect_loop_candidates(rec, ids, vals, conn, device=device)
            res = []
            for d in D:
                n, ne = int(o["n_cand"][d]), int(o["n_enough"][d])
                assert 0 <= n <= db.max_keyframes and 0 <= ne <= n
                assert (o["cand"][d, n:] == -1).all() and np.isnan(o["cand_acc"][d, n:]).all() and (o["enough"][d, ne:] == -1).all()
                sl = slice(int(rec["conn_off"][d]), int(rec["conn_off"][d] + rec["n_conn"][d]))
                r = dict(cand=o["cand"][d, :n].tolist(), acc=o["cand_acc"][d, :n].copy(), diag=o["diag"][d].tolist(), conn_score=o["conn_score"][sl].copy(),
                         min_score=o["min_score"][d], enough=o["enough"][d, :ne].tolist(), n_groups=int(o["n_groups"][d]), groups=det.get_groups(d))
                if cross:
                    nx = int(x["n_cand"][d])
                    r["x"] = dict(cand=x["cand"][d, :nx].tolist(), acc=x["cand_acc"][d, :nx].copy(), diag=x["diag"][d].tolist(), conn_score=x["conn_score"][sl].copy())
                res.append(r)
        db.add(*keyframe_db.pack_add(D, [kf] * len(D), [(s["ids"], s["vals"]) for s in S]))
        db.set_covisibility(keyframe_db.pack_covisibility(D, [kf] * len(D), [s["covis_after"][1] for s in S]))
        out.append(res)
    return out


def same_stream(a, b):
    """two runs' outputs, bit for bit"""
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert (ra is None) == (rb is None)
        for x, y in zip(ra or [], rb or []):
            for f in ("cand", "diag", "enough", "n_groups", "groups"):
                assert x[f] == y[f], f
            assert bits(x["acc"]) == bits(y["acc"]) and bits(x["conn_score"]) == bits(y["conn_score"]) and bits(x["min_score"]) == bits(y["min_score"])
    return True


@pytest.fixture(scope="module")
def stream_run(voc):
    """The streams of SEEDS on three databases, run once: (db, det, streams, got).  Tests read `got`; the reset test replays on the handles."""
    streams = [lc.revisit_fixture(s)[0] for s in SEEDS]
    db = keyframe_db.KeyFrameDatabase(voc, len(SEEDS), K_STREAM, 128)
    det = loop_detect.LoopDetector(db)
    got = run_stream(db, det, streams, cross=True)
    yield db, det, streams, got
    det.close(); db.close()


def test_detect_equals_the_restatement_on_the_stream(stream_run):
    _, _, streams, got = stream_run
    n_loops = n_cand = n_conn = 0
    for d, seed in enumerate(SEEDS):
        expected = lc.revisit_fixture(seed)[1]
        for k, (e, res) in enumerate(zip(expected, got)):
            where = ("seed", seed, "keyframe", k)
            assert e["gated"] == (res is None), where
            if res is None:
                continue
            g = res[d]
            print(where, "cand", g["cand"], "diag", g["diag"], "min_score", g["min_score"], "enough", g["enough"], "groups", [(len(x), c) for x, c in g["groups"]],
                  "ulps", ulps(g["min_score"], e["min_score"]).tolist(), ulps(g["conn_score"], e["conn_score"]).tolist(), ulps(g["acc"], e["acc"]).tolist())
            assert g["cand"] == e["cand"] and g["diag"] == e["diag"], where
            assert g["enough"] == e["enough"] and g["groups"] == e["groups"] and g["n_groups"] == len(e["groups"]), where
            assert [float(x) == -1.0 for x in g["conn_score"]] == [float(x) == -1.0 for x in e["conn_score"]], where
            assert (ulps(g["conn_score"], e["conn_score"]) <= 1).all() and ulps(g["min_score"], e["min_score"]) <= 1, where
            assert (ulps(g["acc"], e["acc"]) <= 11).all(), where
            present = g["conn_score"][g["conn_score"] >= 0]
            assert bits(g["min_score"]) == bits(np.float32(min([np.float32(1)] + list(present)))), where   # of the call's own scores, to the bit
            n_loops += len(e["enough"]) > 0
            n_cand += len(e["cand"])
            n_conn += len(present)
    assert n_loops >= 3 * len(SEEDS) and n_cand >= 20 * len(SEEDS) and n_conn >= 100 * len(SEEDS)


def test_detect_is_the_loop_query_at_the_bound_it_returns(stream_run):
    """No tolerance: the kfdb's own query, given the min_score detect derived, returns detect's candidates, scores and diagnostics bit for bit."""
    n = 0
    for res in stream_run[3]:
        for g in res or []:
            x = g["x"]
            assert x["cand"] == g["cand"] and x["diag"] == g["diag"] and bits(x["acc"]) == bits(g["acc"]) and bits(x["conn_score"]) == bits(g["conn_score"])
            n += len(g["cand"])
    assert n >= 20 * len(SEEDS)


def test_reset_clears_rows_and_groups(stream_run):
    db, det, streams, got = stream_run
    assert any(det.get_groups(d) for d in range(len(SEEDS)))
    db.clear(list(range(len(SEEDS))))
    det.reset(list(range(len(SEEDS))))
    assert all(det.get_groups(d) == [] for d in range(len(SEEDS)))
    for d in range(len(SEEDS)):   # keyframe 20 had connections: its row is empty now
        assert update(det, d, [20]) == (0, [], 1) and det.get_groups(d) == [([20], 0)]
    det.reset(list(range(len(SEEDS))))
    assert same_stream(got, run_stream(db, det, streams))


# ---- 4. refusals ----
def test_refusals_change_nothing(voc):
    K = 70
    cases, runs = lc.case_fixture(K)
    case, (run, _) = cases[0], runs[0]
    db = keyframe_db.KeyFrameDatabase(voc, 3, K, 128, pool_words=4096)
    det = loop_detect.LoopDetector(db, case["max_groups"], case["th"])
    replay_case(det, 1, case, run, steps=range(0, 4))
    rng = np.random.default_rng(1)
    vec = kc.l1_vector(rng, np.arange(300), 40)
    unsorted = (vec[0][::-1].copy(), vec[1])
    db.add(*keyframe_db.pack_add([1, 1], [0, 1], [vec, vec]))
    before = [det.get_groups(d) for d in range(3)]
    assert before[1] == run[3]["groups"] and len(before[1]) >= 2

    def malformed():
        rec, cand = loop_detect.pack_updates([1, 2, 1], [[1], [3], [2]])
        yield "two queries on one database", rec, cand, [-2, 1, -2]   # (on the device the valid one in between runs; the restatement's one fresh group)
        rec, cand = loop_detect.pack_updates([1], [[1, K, 2]])
        yield "a candidate id of K", rec, cand, [-2]
        rec, cand = loop_detect.pack_updates([1], [[1, -1]])
        yield "a negative candidate id", rec, cand, [-2]
        rec, cand = loop_detect.pack_updates([1], [[1, 2]])
        rec["cand_off"][0] = 1
        yield "a record outside its array", rec, cand, [-2]
        rec, cand = loop_detect.pack_updates([3], [[1]])
        yield "a database outside the handle", rec, cand, [-2]

    for what, rec, cand, _ in malformed():
        with pytest.raises(OslamError) as ei:
            det.update_consistency(rec, cand)
        assert ei.value.code == OSLAM_E_INVALID, what
        assert [det.get_groups(d) for d in range(3)] == before, what
    for what, rec, cand, want in malformed():   # the device entry point answers per query
        out = det.update_consistency(rec, cand, device=True)
        assert out["n_enough"].tolist() == [w if w < 0 else 0 for w in want], what
        assert [int(x) for x, w in zip(out["n_groups"], want) if w < 0] == [-9] * sum(w < 0 for w in want) and (out["enough"] == -1).all(), what
        assert det.get_groups(1) == before[1] and det.get_groups(0) == before[0], what
    assert det.get_groups(2) == [([3], 0)]
    det.reset([2])
    # a query the kfdb refuses: the host entry point refuses the call, the device one answers -2; the groups stay
    rec, ids, vals, conn = keyframe_db.pack_queries([1], [unsorted], connected=[[0]])
    with pytest.raises(OslamError) as ei:
        det.detect(rec, ids, vals, conn)
    assert ei.value.code == OSLAM_E_INVALID
    out = det.detect(rec, ids, vals, conn, device=True)
    assert out["n_cand"].tolist() == [-2] and out["n_enough"].tolist() == [-2] and out["n_groups"].tolist() == [-9] and np.isnan(out["min_score"]).all()
    rec, ids, vals, conn = keyframe_db.pack_queries([1, 1], [vec, vec], connected=[[0], [0]])
    with pytest.raises(OslamError) as ei:
        det.detect(rec, ids, vals, conn)
    assert ei.value.code == OSLAM_E_INVALID
    assert det.detect(rec, ids, vals, conn, device=True)["n_enough"].tolist() == [-2, -2]
    assert [det.get_groups(d) for d in range(3)] == before
    # the next valid calls give the restatement's results
    replay_case(det, 1, case, run, steps=range(4, len(run)))
    det.close(); db.close()


# ---- 5. bit identity ----
def test_bit_identity_across_batch_compositions_and_entry_points(voc):
    """64 databases of 12 keyframes; the same loop query of every database four times over, so that the groups' counters reach the threshold: as one batch
    of 64 through the host entry point, as one batch through the device entry point, and database 37 (and 0, 63) alone — on handles with the same history."""
    script, _ = kc.identity_fixture()
    adds, covis, loops = script[0][1], script[1][1], script[2][1]
    rng = np.random.default_rng(11)
    rows = [(d, k, rng.choice(12, int(rng.integers(0, 5)), replace=False).tolist()) for d in range(64) for k in range(12)]

    def handles():
        db = keyframe_db.KeyFrameDatabase(voc, 64, 16, 128)
        db.add(*keyframe_db.pack_add([r[0] for r in adds], [r[1] for r in adds], [(r[2], r[3]) for r in adds]))
        db.set_covisibility(keyframe_db.pack_covisibility([r[0] for r in covis], [r[1] for r in covis], [r[2] for r in covis]))
        det = loop_detect.LoopDetector(db)
        det.set_connected(*loop_detect.pack_connected([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]))
        return db, det

    def calls(det, ds, device):
        out = []
        for _ in range(4):
            rec, ids, vals, conn = keyframe_db.pack_queries(ds, [loops[d][1:3] for d in ds], connected=[loops[d][4] for d in ds])
            o = det.detect(rec, ids, vals, conn, device=device)
            out.append({d: tuple(o[f][i].tobytes() for f in ("cand", "cand_acc", "n_cand", "diag", "min_score", "enough", "n_enough", "n_groups"))
                        + (o["conn_score"][rec["conn_off"][i]:rec["conn_off"][i] + rec["n_conn"][i]].tobytes(), repr(det.get_groups(d))) for i, d in enumerate(ds)})
            last = o
        return out, last

    (db_a, det_a), (db_b, det_b), (db_c, det_c) = handles(), handles(), handles()
    all64 = list(range(64))
    host, last = calls(det_a, all64, False)
    assert (last["n_cand"] >= 0).all() and (last["n_cand"] > 0).sum() >= 32 and (last["n_enough"] > 0).sum() >= 32   # 4 calls: counters 0, 1, 2, 3
    dev, _ = calls(det_b, all64, True)
    assert host == dev
    for q in (37, 0, 63):
        alone, _ = calls(det_c, [q], q == 0)
        assert [c[q] for c in host] == [c[q] for c in alone]
    for h in (det_a, det_b, det_c, db_a, db_b, db_c):
        h.close()


# ---- 7. the adapter ----
def _bow(ids, vals):
    return "%d %s" % (len(ids), " ".join("%d %r" % (int(w), float(x)) for w, x in zip(ids, vals)))


def _list(l):
    return "%d %s" % (len(l), " ".join(map(str, l)))


def test_adapter_program_equals_the_python_view(tmp_path, voc):
    """tests/adapter_loop_detect_program.cc, written against include/orb_slam2_adapter.hpp alone: the stream of seed 0 through ORB_SLAM2::LoopClosing::DetectLoop
    with mLastLoopKFid set to 27 before keyframe 30 (what CorrectLoop does, :585): its decisions against the Python view's, the gate included."""
    from object_slam_amd import build
    build.build_hip()
    steps = lc.revisit_fixture(0)[0]
    last_loop_at = (30, 27)
    lines = []
    for s in steps:
        if s["kf"] == last_loop_at[0]:
            lines.append("M %d" % last_loop_at[1])
        lines += ["S %d %s" % (x, _list(l)) for x, l in s["rows"]] + ["V %d %s" % (x, _list(l)) for x, l in s["covis"]]
        lines.append("D %d %s %s %s" % (s["kf"], _bow(s["ids"], s["vals"]), _list(s["conn"]), _list(s["covis_after"][1])))
    (tmp_path / "ops.txt").write_text("\n".join(lines) + "\n")
    save_text(str(tmp_path / "voc.txt"), *TREE.arrays())
    prog = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adapter_loop_detect_program.cc"), "-o", prog,
                           "-L", LIBDIR, "-loslam_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    r = subprocess.run([prog, str(tmp_path), str(K_STREAM), "128"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    db = keyframe_db.KeyFrameDatabase(voc, 1, K_STREAM, 128)
    det = loop_detect.LoopDetector(db)
    got = run_stream(db, det, [steps], last_loop_at=last_loop_at)
    expected = lc.run_revisit(steps, last_loop_at=last_loop_at)[0]
    out = [l for l in r.stdout.split("\n") if l]
    assert len(out) == len(got) == len(steps)
    gated = []
    for line, s, res, e in zip(out, steps, got, expected):
        if res is None:
            want = "D %d 0 gated" % s["kf"]
        else:
            g = res[0]
            want = "D %d %d %s | %s | %.9g | %d" % (s["kf"], len(g["enough"]) > 0, _list(g["enough"]), _list(g["cand"]), g["min_score"], g["n_groups"])
            assert g["enough"] == e["enough"] and g["cand"] == e["cand"]
        assert line.rstrip() == want.rstrip()
        assert (res is None) == e["gated"]
        gated.append(res is None)
    assert gated[:10] == [True] * 10 and gated[10:30] == [False] * 20 and gated[30:37] == [True] * 7 and not any(gated[37:])
    assert sum(len(res[0]["enough"]) > 0 for res in got if res) >= 3
    det.close(); db.close()
