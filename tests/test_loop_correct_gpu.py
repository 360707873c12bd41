"""GPU: the map corrections of LoopClosing (include/oslam_hip.h, "LoopClosing: map corrections") against the restatements of tests/loop_closing_common.py.
status, corrected_ref and reached are exact; doubles and floats are compared at the project's bar (1e-4 relative to max(1, |.|), no exclusions) AND bit for
bit: kernel and restatement run the same sequence of IEEE operations (+ - * / sqrt, no contraction), and the first run showed bit equality.  Batches of
problems of different sizes with rows no problem owns give the same bytes as each problem alone and as the reversed batch, through the host and the
device entry points, run after run."""
import os
import subprocess

import numpy as np
import pytest

import loop_closing_common as lcc
from object_slam_amd import EssentialGraphOptimizer, LoopCorrector, OslamError, essential_graph as eg
from object_slam_amd._lib import OSLAM_E_CAPACITY, OSLAM_E_INVALID
from object_slam_amd.loop_correct import GBA_PROBLEM_DTYPE, PROBLEM_DTYPE

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIBDIR = os.path.join(ROOT, "object_slam_amd")
BAR = 1e-4
FAR = (3000.0, -1500.0, 4000.0)
SPARE_KF, SPARE_PT = 3, 3


@pytest.fixture(scope="module")
def lc():
    h = LoopCorrector(16, 1024, 1 << 16, 1 << 16)
    yield h
    h.close()


def near(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    return bool((np.abs(a - b) <= BAR * np.maximum(1.0, np.abs(b))).all())


def same(a, b):
    """the bar, then the bits"""
    assert near(a, b)
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prop_problems():
    """n_kf = 1 (the current keyframe alone), 2, 40 keyframes of 300 entries over 4000 points shared by up to 5, a keyframe without points, bad points,
    s = 0.5 and 2, poses far from the origin"""
    ps = [lcc.make_prop_problem(1, 1, 20, 30), lcc.make_prop_problem(2, 2, 15, 25, s_G=0.5), lcc.make_prop_problem(3, 40, 300, 4000, share=5, s_G=2.0, empty_kf=7),
          lcc.make_prop_problem(4, 9, 60, 500, centre=FAR), lcc.make_prop_problem(5, 5, 10, 0), lcc.make_prop_problem(6, 3, 33, 100, p_bad=0.5, s_G=0.5, centre=FAR),
          lcc.make_prop_problem(7, 17, 257, 1000, empty_kf=0)]
    fills = []
    for p in ps:
        n, M = len(p["Tiw"]), len(p["P"])
        fills.append(dict(Scorr=np.full((n, 13), 1.5), Snc=np.full((n, 13), -2.5), Tiw=np.full((n, 4, 4), 3.5), P=np.full((M, 3), 7.5), corrected_ref=np.full(M, -9)))
    return ps, [lcc.propagate(p, f) for p, f in zip(ps, fills)]


def _run_prop(lc, ps, device, order=None, spare=(SPARE_KF, SPARE_PT)):
    recs, a = lcc.pack_prop(ps, spare[0], spare[1], order)
    N, M = len(a["Tiw"]), len(a["P"])
    out = lc.propagate(recs, a["Tiw"], a["Scw"], a["kf_entries"], a["entries"], a["P"], a["bad"], Scorr_out=np.full((N, 13), 1.5), Snc_out=np.full((N, 13), -2.5),
                       Tiw_out=np.full((N, 4, 4), 3.5, np.float32), P_out=np.full((M, 3), 7.5, np.float32), corrected_ref=np.full(M, -9, np.int32),
                       status=np.full((len(ps), 4), 77, np.int32), device=device)
    if order is not None:   # status back in the forward order
        st = np.zeros_like(out["status"])
        st[list(order)] = out["status"]
        out["status"] = st
    return recs, out


def _split_prop(ps, out, b, spare=(SPARE_KF, SPARE_PT)):
    ko = spare[0] + sum(len(p["Tiw"]) for p in ps[:b])
    po = spare[1] + sum(len(p["P"]) for p in ps[:b])
    n, M = len(ps[b]["Tiw"]), len(ps[b]["P"])
    return dict(Scorr=out["Scorr"][ko:ko + n], Snc=out["Snc"][ko:ko + n], Tiw=out["Tiw"][ko:ko + n], P=out["P"][po:po + M], corrected_ref=out["corrected_ref"][po:po + M],
                status=out["status"][b])


KEYS_P = ("Scorr", "Snc", "Tiw", "P")


def test_propagate_batch_equals_the_restatement_and_itself(lc, prop_problems):
    ps, refs = prop_problems
    assert len(ps) == 7
    _, host = _run_prop(lc, ps, False)
    for b, r in enumerate(refs):
        g = _split_prop(ps, host, b)
        assert g["status"].tolist() == r["status"].tolist(), b
        np.testing.assert_array_equal(g["corrected_ref"], r["corrected_ref"])
        for k in KEYS_P:
            same(g[k], r[k])
    assert refs[2]["status"][2] > 3000 and refs[2]["status"][3] > 10000 and (np.bincount(np.concatenate([e[e >= 0] for e in ps[2]["entries"]])) >= 4).any()
    # the rows no problem owns keep the fill bytes
    assert (host["Scorr"][:SPARE_KF] == 1.5).all() and (host["Tiw"][:SPARE_KF] == 3.5).all() and (host["P"][:SPARE_PT] == 7.5).all() and (host["corrected_ref"][:SPARE_PT] == -9).all()
    for name, other in (("device", _run_prop(lc, ps, True)[1]), ("reversed", _run_prop(lc, ps, False, order=range(len(ps))[::-1])[1]), ("again", _run_prop(lc, ps, False)[1]),
                        ("reversed device", _run_prop(lc, ps, True, order=range(len(ps))[::-1])[1])):
        for k in KEYS_P + ("corrected_ref", "status"):
            np.testing.assert_array_equal(other[k].view(np.uint8), host[k].view(np.uint8), err_msg="%s %s" % (name, k))
    for b in range(len(ps)):   # every problem alone
        _, one = _run_prop(lc, [ps[b]], bool(b % 2), spare=(0, 0))
        g, w = _split_prop([ps[b]], one, 0, spare=(0, 0)), _split_prop(ps, host, b)
        for k in KEYS_P + ("corrected_ref", "status"):
            np.testing.assert_array_equal(g[k].view(np.uint8), w[k].view(np.uint8), err_msg="alone %d %s" % (b, k))


def test_propagate_truth(lc, prop_problems):
    """what the CPU test demands of the restatement, of the kernel's own output: corrected points are G(P), corrected centres G(Ow)"""
    ps, _ = prop_problems
    _, host = _run_prop(lc, ps, False)
    for b, p in enumerate(ps):
        g = _split_prop(ps, host, b)
        got = g["corrected_ref"] >= 0
        want = lcc.apply_G(p["G"], p["P"][got].astype(np.float64))
        assert (np.linalg.norm(g["P"][got] - want, axis=1) <= BAR * np.maximum(1.0, np.linalg.norm(want, axis=1))).all(), b
        for i in range(len(p["Tiw"])):
            T0, T1 = p["Tiw"][i].astype(np.float64), g["Tiw"][i].astype(np.float64)
            c0, c1 = lcc.apply_G(p["G"], -T0[:3, :3].T @ T0[:3, 3]), -T1[:3, :3].T @ T1[:3, 3]
            assert np.linalg.norm(c1 - c0) <= BAR * max(1.0, np.linalg.norm(c0)), (b, i)


def test_propagate_invalid_problem_leaves_its_rows_and_its_neighbours(lc, prop_problems):
    ps, refs = prop_problems
    _, good = _run_prop(lc, ps[:4], False)
    T = ps[1]["Tiw"].copy()
    T[1, 0, 2] = np.nan
    cases = [dict(Tiw=T), dict(cur=2), dict(Scw=np.concatenate([ps[1]["Scw"][:12], [-1.0]])), dict(entries=[ps[1]["entries"][0], np.array([3, 25], np.int32)])]
    for device in (False, True):
        for c in cases:
            mixed = [ps[0], dict(ps[1], **c), ps[2], ps[3]]
            _, out = _run_prop(lc, mixed, device)
            g = _split_prop(mixed, out, 1)
            assert g["status"].tolist() == [-1, 2, 0, 0]
            assert (g["Scorr"] == 1.5).all() and (g["Snc"] == -2.5).all() and (g["Tiw"] == 3.5).all() and (g["P"] == 7.5).all() and (g["corrected_ref"] == -9).all()
            for b in (0, 2, 3):
                w, o = _split_prop(ps[:4], good, b), _split_prop(mixed, out, b)
                for k in KEYS_P + ("corrected_ref", "status"):
                    np.testing.assert_array_equal(o[k].view(np.uint8), w[k].view(np.uint8))


def test_refusals(lc, prop_problems):
    ps, _ = prop_problems
    recs, a = lcc.pack_prop(ps[:2])
    args = lambda r, **kw: (r, a["Tiw"], a["Scw"], a["kf_entries"], a["entries"], a["P"], a["bad"])
    small = LoopCorrector(1, 2, 16, 16)
    try:
        for device in (False, True):
            with pytest.raises(OslamError) as ei:   # two problems, three keyframes, more entries and points than the handle was created for
                small.propagate(*args(recs), device=device)
            assert ei.value.code == OSLAM_E_CAPACITY
    finally:
        small.close()
    for field, value in (("kf_offset", 2), ("n_kf", -1), ("point_offset", len(a["P"])), ("entry_offset", -1), ("n_entries", len(a["entries"]) + 1)):
        bad = recs.copy()
        bad[1][field] = value
        with pytest.raises(OslamError) as ei:
            lc.propagate(*args(bad))
        assert ei.value.code == OSLAM_E_INVALID, field
        st = np.full((2, 4), 77, np.int32)
        out = lc.propagate(*args(bad), status=st, device=True, P_out=np.full((len(a["P"]), 3), 7.5, np.float32))   # the device entry point marks the record and goes on
        assert out["status"][1].tolist() == [-2, 0, 0, 0] and out["status"][0, 0] == 0, field
    grec, ga = lcc.pack_gba([lcc.make_gba_problem(1, [-1, 0], [1, 0], 5)])
    gb = grec.copy()
    gb[0]["kf_offset"] = 1
    gargs = (ga["parent"], ga["kf_in_ba"], ga["Tcw"], ga["TcwGBA"], ga["P"], ga["PosGBA"], ga["pt_in_ba"], ga["bad"], ga["ref"])
    with pytest.raises(OslamError) as ei:
        lc.update_after_gba(gb, *gargs)
    assert ei.value.code == OSLAM_E_INVALID
    assert lc.update_after_gba(gb, *gargs, device=True)["status"][0].tolist() == [-2, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_compose_scw(lc):
    rng = np.random.default_rng(11)
    n = 9
    Scm = np.zeros((n, 13))
    Tmw = np.zeros((n, 4, 4), np.float32)
    for b in range(n):
        Scm[b] = np.concatenate([lcc.rand_rot(rng).reshape(9), rng.normal(0, 2, 3), [rng.uniform(0.5, 2.0)]])
        Tmw[b] = lcc.rand_poses(rng, 1, FAR if b % 2 else (0, 0, 0))[0]
    Scw, mScw = lc.compose_scw(Scm, Tmw)
    for b in range(n):
        rec, M = lcc.compose_scw(Scm[b], Tmw[b])
        same(Scw[b], rec)
        same(mScw[b], M)
    d = lc.compose_scw(Scm, Tmw, device=True)
    one = lc.compose_scw(Scm[4:5], Tmw[4:5])
    assert np.array_equal(d[0], Scw) and np.array_equal(d[1], mScw) and np.array_equal(one[0][0], Scw[4]) and np.array_equal(one[1][0], mScw[4])


def test_chain_into_the_essential_graph(lc):
    """Scorr_out, Snc_out and corrected_ref of one problem, cast as INTEGRATION.md says (float32, s first), are accepted by OptimizeEssentialGraph and its
    point correction with status 0"""
    p = lcc.make_prop_problem(21, 6, 40, 200)
    recs, a = lcc.pack_prop([p])
    out = lc.propagate(recs, a["Tiw"], a["Scw"], a["kf_entries"], a["entries"], a["P"], a["bad"])
    assert out["status"][0, 0] == 0
    n = 10                                                           # a map of ten keyframes: the six corrected ones are its last six
    rng = np.random.default_rng(2)
    Tall = np.concatenate([lcc.rand_poses(rng, n - 6, (0, 0, 0)), p["Tiw"]])
    to13 = lambda S: np.concatenate([S[:, 12:13], S[:, :12]], 1).astype(np.float32)   # R, t, s (double) -> s, R, t (float)
    Scw = np.concatenate([np.ones((n, 1)), Tall[:, :3, :3].reshape(n, 9), Tall[:, :3, 3]], 1).astype(np.float32)
    Snc = np.zeros((n, 13), np.float32)
    Scw[n - 6:], Snc[n - 6:] = to13(out["Scorr"]), to13(out["Snc"])
    has_nc = np.array([0] * (n - 6) + [1] * 6, np.uint8)
    fixed = np.array([1] + [0] * (n - 1), np.uint8)
    edges = np.array([(k, k - 1, eg.KIND_NORMAL) for k in range(1, n)] + [(n - 6 + p["cur"], 0, eg.KIND_LOOP)], np.int32)
    h = EssentialGraphOptimizer(1, n, len(edges), 4096)
    try:
        pr = eg.pack_problems([n], [len(edges)], [0])
        r = h.optimize_batch(pr, Scw, Snc, has_nc, fixed, edges)
        assert r["status"][0, 0] == 0 and r["status"][0, 1] == n - 1
        ref = np.where(out["corrected_ref"] >= 0, out["corrected_ref"] + (n - 6), -1).astype(np.int32)
        fill = np.full((len(ref), 3), 7.5, np.float32)
        P2 = h.correct_points(pr, Scw, r["Scw"], r["status"], np.zeros(len(ref), np.int32), ref, out["P"], P_out=fill.copy())
        assert np.isfinite(P2).all() and (P2[ref >= 0] != 7.5).any() and (P2[ref < 0] == 7.5).all() and (ref >= 0).sum() > 50
    finally:
        h.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gba_problems():
    ps = [lcc.make_gba_problem(60 + i, parent, in_ba, 150, centre=(FAR if i % 2 else (0, 0, 0))) for i, (_, parent, in_ba, st, _, _) in enumerate(lcc.gba_trees()) if st == 0]
    n = 300                                                             # a map of 300 keyframes, a chain with the last 12 outside the BA, 20 000 points
    ps.append(lcc.make_gba_problem(70, [-1] + list(range(n - 1)), [1] * (n - 12) + [0] * 12, 20000, p_pt_in_ba=0.66))
    ps.append(lcc.make_gba_problem(71, [], [], 0))
    fills = [dict(Tcw=np.full((len(p["parent"]), 4, 4), 3.5), reached=np.full(len(p["parent"]), 9), P=np.full((len(p["P"]), 3), 7.5)) for p in ps]
    return ps, [lcc.update_after_gba(p, f) for p, f in zip(ps, fills)]


def _run_gba(lc, ps, device, order=None, spare=(SPARE_KF, SPARE_PT)):
    recs, a = lcc.pack_gba(ps, spare[0], spare[1], order)
    N, M = len(a["parent"]), len(a["P"])
    out = lc.update_after_gba(recs, a["parent"], a["kf_in_ba"], a["Tcw"], a["TcwGBA"], a["P"], a["PosGBA"], a["pt_in_ba"], a["bad"], a["ref"], Tcw_out=np.full((N, 4, 4), 3.5, np.float32),
                              reached=np.full(N, 9, np.uint8), P_out=np.full((M, 3), 7.5, np.float32), status=np.full((len(ps), 4), 77, np.int32), device=device)
    if order is not None:
        st = np.zeros_like(out["status"])
        st[list(order)] = out["status"]
        out["status"] = st
    return out


def _split_gba(ps, out, b, spare=(SPARE_KF, SPARE_PT)):
    ko = spare[0] + sum(len(p["parent"]) for p in ps[:b])
    po = spare[1] + sum(len(p["P"]) for p in ps[:b])
    n, M = len(ps[b]["parent"]), len(ps[b]["P"])
    return dict(Tcw=out["Tcw"][ko:ko + n], reached=out["reached"][ko:ko + n], P=out["P"][po:po + M], status=out["status"][b])


KEYS_G = ("Tcw", "reached", "P", "status")


def test_gba_batch_equals_the_restatement_and_itself(lc, gba_problems):
    ps, refs = gba_problems
    host = _run_gba(lc, ps, False)
    for b, r in enumerate(refs):
        g = _split_gba(ps, host, b)
        assert g["status"].tolist() == r["status"].tolist(), (b, g["status"], r["status"])
        np.testing.assert_array_equal(g["reached"], r["reached"])
        same(g["Tcw"], r["Tcw"])
        same(g["P"], r["P"])
    big = refs[-2]["status"]
    assert big.tolist()[:2] == [0, 12] and big[3] == 300 and 12000 < big[2] < 20000
    assert (host["Tcw"][:SPARE_KF] == 3.5).all() and (host["reached"][:SPARE_KF] == 9).all() and (host["P"][:SPARE_PT] == 7.5).all()
    rev = range(len(ps))[::-1]
    for name, other in (("device", _run_gba(lc, ps, True)), ("reversed", _run_gba(lc, ps, False, order=rev)), ("again", _run_gba(lc, ps, False)),
                        ("reversed device", _run_gba(lc, ps, True, order=rev))):
        for k in KEYS_G:
            np.testing.assert_array_equal(other[k].view(np.uint8), host[k].view(np.uint8), err_msg="%s %s" % (name, k))
    for b in range(len(ps)):
        one = _run_gba(lc, [ps[b]], bool(b % 2), spare=(0, 0))
        g, w = _split_gba([ps[b]], one, 0, spare=(0, 0)), _split_gba(ps, host, b)
        for k in KEYS_G:
            np.testing.assert_array_equal(g[k].view(np.uint8), w[k].view(np.uint8), err_msg="alone %d %s" % (b, k))


def test_gba_truth_and_refused_maps(lc, gba_problems):
    ps, _ = gba_problems
    host = _run_gba(lc, ps, False)
    for b, p in enumerate(ps):
        g = _split_gba(ps, host, b)
        for k in range(len(p["parent"])):
            want = p["Tcw"][k].astype(np.float64) @ p["Ginv"]
            assert np.abs(g["Tcw"][k][:3, :3] - want[:3, :3]).max() <= BAR and np.linalg.norm(g["Tcw"][k][:3, 3] - want[:3, 3]) <= BAR * max(1.0, np.linalg.norm(want[:3, 3])), (b, k)
        sel = (p["bad"] == 0) & (p["pt_in_ba"] == 0)
        want = lcc.apply_G(p["G"], p["P"][sel].astype(np.float64))
        assert (np.linalg.norm(g["P"][sel] - want, axis=1) <= BAR * np.maximum(1.0, np.linalg.norm(want, axis=1))).all(), b
    # a root outside the BA (either entry point), a cycle and an index out of range (the host entry point, before any launch): status -1, rows untouched, neighbours unchanged
    trees = {name: (parent, in_ba) for name, parent, in_ba, *_ in lcc.gba_trees()}
    root = lcc.make_gba_problem(80, *trees["root_outside_ba"], 40)
    cyc = lcc.make_gba_problem(81, *trees["unreachable"], 40)
    oob = lcc.make_gba_problem(82, [-1, 0, 3], [1, 1, 1], 40)
    selfp = lcc.make_gba_problem(83, [-1, 1], [1, 1], 10)
    for device, extra in ((False, [root, cyc, oob, selfp]), (True, [root])):
        mixed = [ps[0]] + extra + [ps[1]]
        out = _run_gba(lc, mixed, device)
        for b in range(1, 1 + len(extra)):
            g = _split_gba(mixed, out, b)
            assert g["status"].tolist() == [-1, 0, 0, 0] and (g["Tcw"] == 3.5).all() and (g["reached"] == 9).all() and (g["P"] == 7.5).all(), (device, b)
        for b, src in ((0, 0), (len(mixed) - 1, 1)):
            g, w = _split_gba(mixed, out, b), _split_gba(ps, host, src)
            for k in KEYS_G:
                np.testing.assert_array_equal(g[k].view(np.uint8), w[k].view(np.uint8))
    only = _run_gba(lc, [cyc], False, spare=(0, 0))   # every problem refused: nothing is launched
    assert only["status"][0].tolist() == [-1, 0, 0, 0] and (only["Tcw"] == 3.5).all() and (only["P"] == 7.5).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_adapter_program_equals_the_ctypes_path(lc, tmp_path):
    from object_slam_amd import BowMatcher, KP_DTYPE, build
    build.build_hip()
    prog = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adapter_loop_correct_program.cc"), "-o", prog,
                           "-L", LIBDIR, "-loslam_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    tok = {}
    for l in r.stdout.split("\n"):
        if l:
            tok.setdefault(l.split()[0], []).append(l.split()[1:])
    f = lambda key: np.array([int(v, 16) for v in tok[key][0]], np.uint64).astype(np.uint32).view(np.float32)
    d = lambda key: np.array([int(v, 16) for v in tok[key][0]], np.uint64).view(np.float64)
    i = lambda key, dt=np.int32: np.array([int(v) for v in tok[key][0]], dt)
    # SearchByBoW(KF1, KF2)
    sides = []
    for key in ("bow1", "bow2"):
        rows = tok[key]
        k = np.zeros(len(rows), KP_DTYPE)
        k["angle"] = np.array([int(row[0], 16) for row in rows], np.uint64).astype(np.uint32).view(np.float32)
        sides.append((k, np.array([[int(v) for v in row[3:]] for row in rows], np.uint8), np.array([int(row[2]) for row in rows], np.uint8), np.array([int(row[1]) for row in rows], np.uint32)))
    bm = BowMatcher(2400)
    try:
        nm, m = bm.SearchByBoWKF(*sides[0], *sides[1], nnratio=0.75, checkOri=True)
    finally:
        bm.close()
    np.testing.assert_array_equal(m, i("match12"))
    assert nm == int(tok["nmatches"][0][0]) and nm >= 5
    rnm, rm = lcc.search_by_bow_kf(*sides[0], *sides[1], nnratio=0.75, checkOri=True)
    assert rnm == nm and np.array_equal(rm, m)
    # mg2oScw
    Scw, mScw = lc.compose_scw(d("Scm"), f("Tmw"))
    np.testing.assert_array_equal(Scw[0], d("Scw"))
    np.testing.assert_array_equal(mScw[0].reshape(-1), f("mScw"))
    # propagation
    Tiw, P, ptr, mp = f("prop_Tiw").reshape(-1, 4, 4), f("prop_P").reshape(-1, 3), i("prop_ptr"), i("prop_mp")
    n, M = len(Tiw), len(P)
    recs = np.zeros(1, PROBLEM_DTYPE)
    recs[0] = (n, 0, int(tok["prop_cur"][0][0]), M, 0, len(mp), 0, 0)
    out = lc.propagate(recs, Tiw, d("Scw"), np.stack([ptr[:-1], np.diff(ptr)], 1), mp, P, i("prop_bad", np.uint8), P_out=P.copy())
    assert out["status"][0, 0] == 0 and out["status"][0, 2] > 10
    np.testing.assert_array_equal(out["Scorr"].reshape(-1), d("prop_Scorr"))
    np.testing.assert_array_equal(out["Snc"].reshape(-1), d("prop_Snc"))
    np.testing.assert_array_equal(out["Tiw"].reshape(-1), f("prop_Tout"))
    np.testing.assert_array_equal(out["P"].reshape(-1), f("prop_Pout"))
    np.testing.assert_array_equal(out["corrected_ref"], i("prop_ref"))
    # the map update after global BA
    Tcw, Pg = f("gba_Tcw").reshape(-1, 4, 4), f("gba_P").reshape(-1, 3)
    grec = np.zeros(1, GBA_PROBLEM_DTYPE)
    grec[0]["n_kf"], grec[0]["n_points"] = len(Tcw), len(Pg)
    g = lc.update_after_gba(grec, i("gba_parent"), i("gba_in_ba", np.uint8), Tcw, f("gba_Tg"), Pg, f("gba_Pg"), i("gba_pin", np.uint8), i("gba_bad", np.uint8), i("gba_ref"), P_out=Pg.copy())
    assert g["status"][0].tolist()[:2] == [0, 3] and g["status"][0, 3] == 5
    np.testing.assert_array_equal(g["Tcw"].reshape(-1), f("gba_Tout"))
    np.testing.assert_array_equal(g["reached"], i("gba_reached", np.uint8))
    np.testing.assert_array_equal(g["P"].reshape(-1), f("gba_Pout"))
