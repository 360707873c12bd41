"""GPU: the pose-consuming kernels at world poses far from the identity (tests/gauge_common.py): every existing parity input is moved by a rigid motion
of the world, so the poses the kernels receive have a trace <= 0 and csrc/se3_math.h quat_from_R leaves its first body (tests/test_far_pose_cpu.py counts
which bodies each table reaches, and shows that the reference decides every case: same flags as on the unmoved problem).  HIP against the reference on the
same moved input with the assertions and tolerances of the operator's own test file, and the 3 x 3 rotation block within 1e-4 absolute (its entries are
at most 1: the same bar, which a translation of some metres cannot dilute)."""
import numpy as np
import pytest

import essential_graph_common as egc
import gauge_common as gc
import sim3_opt_common as soc
from batch_common import LS2, SF
from lm_trace import compare_lm_traces

pytestmark = pytest.mark.gpu
RTOL = 1e-4


def _rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def _rot_close(T, oT):
    T, oT = np.asarray(T, np.float64).reshape(-1, 4, 4), np.asarray(oT, np.float64).reshape(-1, 4, 4)
    return float(np.abs(T[:, :3, :3] - oT[:, :3, :3]).max()) <= RTOL


# ---- PoseOptimization ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pose_handles():
    from object_slam_amd import PoseOptimizer
    small, big = PoseOptimizer(max_points=2048), PoseOptimizer(max_points=6000)    # LDS-staged edges / edges read from global memory
    yield small, big
    small.close()
    big.close()


def _pose_check(oracle, handles, q, what):
    small, big = handles
    args = gc.pose_args(q)
    n, T, outl, st = small.PoseOptimization(*args)
    nb, Tb, ob, _ = big.PoseOptimization(*args)
    on, oT, ooutl, ost = oracle.pose_optimization(*args)
    assert _rel(T, oT) <= RTOL and _rot_close(T, oT), (what, T, oT)
    np.testing.assert_array_equal(outl, ooutl)
    assert n == on, what
    assert nb == n and np.array_equal(ob, outl) and np.array_equal(Tb, T), what      # same arithmetic, only the source of the operands differs
    return st, ost


@pytest.mark.parametrize("seed,N,g", gc.POSE_CASES)
def test_pose_optimization_far_pose_matches_oracle(oracle, pose_handles, seed, N, g):
    q, _, _ = gc.pose_case(seed, N, g)
    st, ost = _pose_check(oracle, pose_handles, q, (seed, N, g))
    assert 4 <= st[0] <= 40 and st[0] <= st[1] <= 400, (st, ost)


@pytest.mark.parametrize("seed,N,g", gc.POSE_FEW)
def test_pose_optimization_far_pose_fewer_than_ten_edges(oracle, pose_handles, seed, N, g):
    """< 10 edges: a single round (reference src/Optimizer.cc:440)"""
    q, _, _ = gc.pose_case(seed, N, g, few=True)
    st, ost = _pose_check(oracle, pose_handles, q, (seed, N, g))
    assert 1 <= st[0] <= 10, (st, ost)


def test_pose_optimization_far_pose_batch_of_mixed_bodies(oracle, pose_handles):
    """one optimize_batch_device call whose 8 elements start in different bodies (a gauge per element): each element equals its single call bit for bit,
    and the oracle within the bar"""
    import ctypes as C

    import torch

    from object_slam_amd import PoseOptimizer
    probs = [gc.pose_case(seed, 400, g)[0] for seed, g in gc.POSE_BATCH]
    B, N = len(probs), 400
    assert {gc.quat_branch(p["Tcw"]) for p in probs} == {0, 1, 2, 3}
    t = lambda k, dt: torch.from_numpy(np.stack([p[k] for p in probs]).astype(dt)).cuda()
    Tcw, Xw, obs, inv, has = t("Tcw", np.float32), t("Xw", np.float32), t("obs", np.float32), t("invSigma2", np.float32), t("has_mp", np.uint8)
    po = PoseOptimizer(max_points=N, max_batch=B)
    po.optimize_batch_device(B, N, None, N, Tcw.data_ptr(), Xw.data_ptr(), obs.data_ptr(), inv.data_ptr(), has.data_ptr(), probs[0]["K"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    dT, dO, dN, dS = po.results_device()
    Tout = np.zeros((B, 16), np.float32); outl = np.zeros((B, N), np.uint8); ninl = np.zeros(B, np.int32)
    hip = C.CDLL("libamdhip64.so")
    for dst, src, nbytes in ((Tout, dT, Tout.nbytes), (outl, dO, outl.nbytes), (ninl, dN, ninl.nbytes)):
        assert hip.hipMemcpy(dst.ctypes.data_as(C.c_void_p), C.c_void_p(src), C.c_size_t(nbytes), 2) == 0
    single = PoseOptimizer(max_points=N)
    for b, p in enumerate(probs):
        on, oT, ooutl, _ = oracle.pose_optimization(*gc.pose_args(p))
        assert ninl[b] == on and _rel(Tout[b].reshape(4, 4), oT) <= RTOL and _rot_close(Tout[b], oT), gc.POSE_BATCH[b]
        np.testing.assert_array_equal(outl[b], ooutl)
        n1, T1, o1, _ = single.PoseOptimization(*gc.pose_args(p))
        assert n1 == ninl[b] and np.array_equal(o1, outl[b]) and np.array_equal(T1, Tout[b].reshape(4, 4)), gc.POSE_BATCH[b]
    po.close()
    single.close()


@pytest.mark.parametrize("seed,N,g", gc.POSE_TRACE)
def test_pose_optimization_far_pose_lm_schedule_matches_oracle(oracle, pose_handles, seed, N, g):
    q, _, _ = gc.pose_case(seed, N, g)
    assert gc.quat_branch(q["Tcw"]) != 0
    po = pose_handles[0]
    args = gc.pose_args(q)
    (n, T, outl, st), th = po.lm_trace(lambda: po.PoseOptimization(*args))
    (on, oT, ooutl, ost), to = oracle.lm_trace(lambda: oracle.pose_optimization(*args))
    assert len(th) == st[1] and len(to) == ost[1]
    compared, undecidable = compare_lm_traces(th, to)
    assert compared >= 8, (compared, undecidable, len(th), len(to))
    if undecidable == 0:
        assert st == ost, (st, ost)
    assert n == on and np.array_equal(outl, ooutl)


@pytest.mark.parametrize("seed,g", gc.SEMANTIC_CASES)
def test_pose_optimization2_far_pose_matches_oracle(oracle, seed, g):
    from object_slam_amd import PoseOptimizer
    q, _, _ = gc.semantic_case(seed, g)
    po = PoseOptimizer(max_points=1024)
    n, T, outl, nsem = po.PoseOptimization2(q)
    on, oT, ooutl, onsem = oracle.pose_optimization2(q)
    assert nsem == onsem and nsem > 20, (nsem, onsem)
    assert _rel(T, oT) <= RTOL and _rot_close(T, oT)
    np.testing.assert_array_equal(outl, ooutl)
    assert n == on
    po.close()


# ---- LocalBundleAdjustment / BundleAdjustment ------------------------------------------------------------------------------------------------------
_lba_ref = {}


def _lba_oracle(oracle, shape, g):
    if (shape, g) not in _lba_ref:
        _lba_ref[(shape, g)] = oracle.local_bundle_adjustment(*gc.lba_args(gc.lba_case(shape, g)[0]))
    return _lba_ref[(shape, g)]


def _lba_compare(a, o):
    po, xo, er, st = a
    opo, oxo, oer, ost = o
    assert _rel(po, opo) <= RTOL and _rot_close(po, opo)
    assert _rel(xo, oxo) <= RTOL
    np.testing.assert_array_equal(er, oer)
    assert st[0] == ost[0] and st[2] == ost[2], (st, ost)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape,g", gc.LBA_CASES)
def test_lba_far_pose_matches_oracle(oracle, shape, g, mode):
    """the three layouts convert the input poses at three places (lba.hip's one-block kernel, k_w_init of the wide layout, lba_win.inc of the window
    layout); the wide layout with both Schur implementations"""
    from object_slam_amd import LocalBundleAdjuster
    q, _, _ = gc.lba_case(shape, g)
    o = _lba_oracle(oracle, shape, g)
    ba = LocalBundleAdjuster(max_keyframes=16, max_points=1024, max_edges=8192)
    ba.set_mode(mode)
    _lba_compare(ba.LocalBundleAdjustment(*gc.lba_args(q)), o)
    if mode == 1:
        for schur in (0, 1):
            ba.set_schur(schur)
            _lba_compare(ba.LocalBundleAdjustment(*gc.lba_args(q)), o)
    ba.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_lba_far_pose_batch_of_windows(oracle, mode):
    """oslam_lba_optimize_batch: the windows of one launch sit in different gauges, two of them with keyframes in different bodies"""
    from object_slam_amd import LocalBundleAdjuster
    probs = [gc.lba_case(shape, g)[0] for shape, g in gc.LBA_BATCH]
    ba = LocalBundleAdjuster(max_keyframes=16, max_points=1024, max_edges=8192, max_batch=len(probs))
    ba.set_mode(mode)
    res = ba.LocalBundleAdjustmentBatch(probs, probs[0]["K"])
    for (shape, g), r in zip(gc.LBA_BATCH, res):
        _lba_compare(r, _lba_oracle(oracle, shape, g))
    ba.close()


@pytest.mark.parametrize("shape,g", gc.LBA_TRACE)
def test_lba_far_pose_lm_schedule_matches_oracle(oracle, shape, g):
    from object_slam_amd import LocalBundleAdjuster
    q, _, _ = gc.lba_case(shape, g)
    args = gc.lba_args(q)
    ba = LocalBundleAdjuster(max_keyframes=16, max_points=1024, max_edges=8192)
    a, th = ba.lm_trace(lambda: ba.LocalBundleAdjustment(*args))
    o, to = oracle.lm_trace(lambda: oracle.local_bundle_adjustment(*args))
    assert len(th) == a[3][1] + a[3][3] and len(to) == o[3][1] + o[3][3]
    compared, undecidable = compare_lm_traces(th, to)
    assert compared >= 4, (compared, undecidable, len(th), len(to))
    if undecidable == 0:
        assert tuple(a[3]) == tuple(o[3]), (a[3], o[3])
    ba.close()


@pytest.mark.parametrize("wide,robust,its,g", gc.BA_CASES)
def test_bundle_adjustment_far_pose_matches_oracle(oracle, wide, robust, its, g):
    from object_slam_amd import LocalBundleAdjuster
    q, _, _ = gc.ba_case(robust, g)
    ba = LocalBundleAdjuster(max_keyframes=16, max_points=1024, max_edges=8192)
    ba.set_mode(wide)
    po, xo = ba.BundleAdjustment(*gc.lba_args(q), its, robust)
    opo, oxo = oracle.bundle_adjustment(*gc.lba_args(q), its, robust)
    assert _rel(po, opo) <= RTOL and _rot_close(po, opo)
    err = np.abs(xo - oxo).max(axis=1) / max(1.0, np.abs(oxo).max())
    assert err.max() <= RTOL, np.sort(err)[-3:]
    ba.close()


# ---- OptimizeSim3 ------------------------------------------------------------------------------------------------------------------------------
def test_sim3_far_rotation_matches_the_restatement():
    """R12 at 150 degrees about x, y and z, fixed and free scale, in one batch: status (return value, count, nBad), surviving pairs, S12 within 1e-4
    relative (rotation block 1e-4 absolute) against the restatement summing in the kernel's order and forward, and the accept / reject sequence over the
    trials every summation order of the restatement decides alike (test_far_pose_cpu.py: at least three per problem; later trials of a converged run have a
    rho of rounding noise, tests/sim3_opt_common.py PARITY_SPECS)."""
    from object_slam_amd import sim3_opt
    problems, refs = [], []
    for case in gc.SIM3_CASES:
        p, r = gc.sim3_references(case)
        problems.append(p)
        refs.append(r)
    arrays, counts = soc.concat_batch(problems)
    n = len(problems)
    pr = sim3_opt.pack_problems(counts, [p["K1"] for p in problems], [p["K2"] for p in problems], [p["s12"] for p in problems], np.stack([p["R12"] for p in problems]).reshape(n, 3, 3),
                                np.stack([p["t12"] for p in problems]).reshape(n, 3), [p["fix_scale"] for p in problems], [p["th2"] for p in problems])
    opt = sim3_opt.Sim3Optimizer(16, 2048)
    M = len(arrays["invSigma2_1"])
    out = opt.optimize_batch(pr, arrays["X3Dc1"], arrays["X3Dc2"], arrays["obs1"], arrays["obs2"], arrays["invSigma2_1"], arrays["invSigma2_2"], S12=np.full((n, 13), -7.25, np.float64),
                             inliers=np.full(M, 0x5A, np.uint8), status=np.full((n, 4), -77, np.int32), trace=True)
    opt.close()
    for j, (p, (fwd, rev, wav)) in enumerate(zip(problems, refs)):
        st, S = out["status"][j], out["S12"][j]
        inl = out["inliers"][pr["offset"][j]:pr["offset"][j] + pr["count"][j]]
        assert st[:3].tolist() == [wav["ret"], wav["count"], wav["nBad"]] and np.array_equal(inl, wav["inliers"]), p["name"]
        assert wav["written"] and (S != -7.25).any(), p["name"]
        for r in (wav, fwd):
            d = float((np.abs(S - r["S12"]) / np.maximum(1.0, np.abs(r["S12"]))).max())
            assert d <= RTOL and np.abs(S[:9] - r["S12"][:9]).max() <= RTOL, (p["name"], d)
        k = gc.decided_prefix((fwd, rev, wav))
        n_tr = int(out["trace_n"][j])
        assert k >= 3 and n_tr >= k and out["trace"][j, :k, 4].tolist() == [t[4] for t in wav["trace"][:k]], (p["name"], k, n_tr)
        print("%-22s body %d ret %d nBad %d trials %d (restatement %d), %d decided trials compared" % (p["name"], gc.quat_branch(p["R12"]), st[0], st[2], n_tr, wav["trials"], k))


# ---- OptimizeEssentialGraph --------------------------------------------------------------------------------------------------------------------
def test_essential_graph_ring_about_x_and_z_matches_the_restatement():
    """tests/test_essential_graph_gpu.py::test_parity_with_the_restatement and its decisive-trial comparison on rings whose axis is x and z (bodies 1 and
    3), and on a ring in a moved world (all four bodies); then the point correction (float output of an fp64 map: 1e-6 relative) with the moved Sim3s."""
    from object_slam_amd import essential_graph as eg
    problems = [gc.ring_case(*c)[0] for c in gc.RING_CASES]
    ref = [egc.optimize_essential_graph(p) for p in problems]
    rev = [egc.optimize_essential_graph(p, "reversed") for p in problems]
    arrays, n_kf, n_ed = egc.concat_batch(problems)
    pr = eg.pack_problems(n_kf, n_ed, [p["fix_scale"] for p in problems])
    N = len(arrays["fixed"])
    opt = eg.EssentialGraphOptimizer(16, 256, 1024, 8192)
    out = opt.optimize_batch(pr, arrays["Scw"], arrays["Snc"], arrays["has_nc"], arrays["fixed"], arrays["edges"], Scw_out=np.full((N, 13), -7.25), Tcw_out=np.full((N, 4, 4), -3.5, np.float32),
                             status=np.full((len(pr), 4), -77, np.int32), trace=True)
    rel = lambda a, b: float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())
    for j, (p, r, rv, rec) in enumerate(zip(problems, ref, rev, pr)):
        o, n = rec["kf_offset"], rec["n_kf"]
        st, S, T = out["status"][j], out["Scw"][o:o + n], out["Tcw"][o:o + n]
        assert st[:3].tolist() == r["status"][:3].tolist(), p["name"]
        assert rel(S, r["Scw"]) <= RTOL and rel(T.astype(np.float64), r["Tcw"].astype(np.float64)) <= RTOL, p["name"]
        assert np.abs(S[:, :9] - r["Scw"][:, :9]).max() <= RTOL and np.abs(T[:, :3, :3].astype(np.float64) - r["Tcw"][:, :3, :3]).max() <= RTOL, p["name"]
        dec = egc.decisive_trials(r, rv)
        n_tr = int(out["trace_n"][j])
        tr = out["trace"][j, :n_tr]
        compared = 0
        for k, d in enumerate(dec):
            if not d:
                continue
            assert k < n_tr and tr[k, 4] == r["trace"][k][4] and abs(tr[k, 3] - r["trace"][k][3]) <= 1e-9 * r["trace"][k][3], (p["name"], k)
            compared += 1
        assert compared >= 1, p["name"]
        print("%-22s bodies %s status %s compared %d trials" % (p["name"], sorted(set(gc.ring_branches(p))), st.tolist(), compared))
    # correct_points
    rng = np.random.default_rng(3)
    pp = np.repeat(np.arange(len(pr), dtype=np.int32), 40)
    ref_kf = np.concatenate([rng.integers(-1, rec["n_kf"], 40) for rec in pr]).astype(np.int32)
    P = rng.uniform(-5, 5, (len(pp), 3)).astype(np.float32)
    fill = np.full_like(P, np.float32(-3.5))
    got = opt.correct_points(pr, arrays["Scw"], out["Scw"], out["status"], pp, ref_kf, P, P_out=fill.copy())
    worst = 0.0
    for j, rec in enumerate(pr):
        sel = pp == j
        o, n = rec["kf_offset"], rec["n_kf"]
        want = egc.correct_points(arrays["Scw"][o:o + n], out["Scw"][o:o + n], ref_kf[sel], P[sel], P_out=fill[sel])
        assert (got[sel][ref_kf[sel] < 0] == np.float32(-3.5)).all()
        worst = max(worst, rel(got[sel].astype(np.float64), want.astype(np.float64)))
    assert (ref_kf < 0).any() and worst <= 1e-6, worst
    opt.close()


# ---- the float kernels that read the rows of Tcw / Twc: bit-exact where the existing test is ---------------------------------------------------
@pytest.mark.parametrize("th", [1.0, 3.0])
@pytest.mark.parametrize("g", ["ry175", "rx170", "cyclic"])
def test_is_in_frustum_far_pose(oracle, g, th):
    """Frame::isInFrustum with negative diagonal entries in Tcw, a camera centre metres from the origin and (ry175, rx170) a view direction along -z; M = 2000
    with 400 points exactly on predicted-level boundaries"""
    from object_slam_amd import MapPointBatch, QUERY_DTYPE
    args = gc.frustum_case(g) + (th,)
    got = MapPointBatch().isInFrustum(*args)
    ref = oracle.is_in_frustum(*args)
    assert 0.05 * 2000 < int((ref["flags"] & 1).sum()) < 0.9 * 2000
    for f in QUERY_DTYPE.names:
        assert np.array_equal(got[f], ref[f]), f
    assert np.array_equal(got.view(np.uint8), ref.view(np.uint8))


@pytest.mark.parametrize("seed,stereo_frac,baseline,g", gc.TRI_CASES)
def test_triangulate_far_pose(oracle, seed, stereo_frac, baseline, g):
    """accept flags identical, positions <= 1e-5 relative (tests/test_triangulate_gpu.py), Tcw and Twc of both keyframes moved"""
    from object_slam_amd import MapPointBatch
    from object_slam_amd.mappoint import make_tri_kf
    c = gc.tri_case(seed, stereo_frac, baseline, g)
    T1, W1, a1 = c["kf1"]
    k1 = make_tri_kf(T1, W1, c["cam8"], *a1)
    k2 = [make_tri_kf(T2, W2, c["cam8"], *a) for T2, W2, a, _, _ in c["pairs"]]
    matches = [(i1, i2) for _, _, _, i1, i2 in c["pairs"]]
    ratio = np.float32(1.5) * np.float32(1.2)
    ok, x = MapPointBatch().triangulate(k1, k2, matches, SF, LS2, ratio)
    refs = [oracle.triangulate((T1, W1, c["cam8"]) + a1, (T2, W2, c["cam8"]) + a, i1, i2, SF, LS2, ratio) for T2, W2, a, i1, i2 in c["pairs"]]
    ref_ok, ref_x = np.concatenate([r[0] for r in refs]), np.concatenate([r[1] for r in refs])
    assert len(ok) == len(ref_ok) == 300 and np.array_equal(ok, ref_ok)
    sel = ok.astype(bool)
    assert 20 < int(sel.sum()) < 290
    rel = np.abs(x[sel] - ref_x[sel]).max(1) / np.maximum(np.abs(ref_x[sel]).max(1), 1e-3)
    assert rel.max() <= 1e-5, rel.max()
    assert not x[~sel].any()


@pytest.mark.parametrize("g", ["ry175", "r111_130"])
def test_last_frame_projection_far_pose(oracle, g):
    """tests/test_matcher_gpu.py::test_last_frame_projection_on_extracted_frames with the world moved: Tlw and Tcw alike, the map points with them.  The
    queries k_project_last writes equal the oracle's bit for bit, the matches follow."""
    from object_slam_amd import ORBextractor, ORBmatcher, synth
    frames, offs = synth.make_stream(40, 640, 480, seed=9)
    ex = ORBextractor(1000, 1.2, 8, 20, 7, 640, 480)
    kl, dl = ex(frames[10])
    kc, dc = ex(frames[13])
    sf = ex.GetScaleFactors()
    fx = fy = 520.0
    cx, cy, bf, b = 320.0, 240.0, 40.0, 40.0 / 520.0
    Z0 = 2.0
    du, dv = (offs[13] - offs[10]).astype(np.float64)
    G = gc.gauge(g)
    Xw = gc.move_points(np.stack([(kl["x"] - cx) * Z0 / fx, (kl["y"] - cy) * Z0 / fy, np.full(len(kl), Z0)], 1), G)
    T = np.eye(4)
    T[0, 3], T[1, 3] = -du * Z0 / fx, -dv * Z0 / fy
    Tlw, Tcw = gc.move_poses(np.eye(4), G), gc.move_poses(T, G)
    assert gc.quat_branch(Tlw) != 0 and gc.quat_branch(Tcw) != 0
    rng = np.random.default_rng(1)
    has_mp = ((rng.random(len(kl)) < 0.9).astype(np.uint8)) | ((rng.random(len(kl)) < 0.7).astype(np.uint8) << 1)
    uRc = (kc["x"] - bf / Z0).astype(np.float32)
    bounds = (0.0, 0.0, 640.0, 480.0)
    for th, mono in ((15.0, False), (7.0, False), (15.0, True)):
        m = ORBmatcher(0.9, True, max_keypoints=1200, max_queries=1200)
        nm, qm, qd, km = m.search_last_frame(kc, uRc, dc, None, bounds, Xw, has_mp, kl, dl, Tcw, Tlw, (fx, fy, cx, cy, bf, b), sf, th, mono)
        oq = oracle.project_last_frame(Xw, has_mp, kl, dl, Tcw, Tlw, (fx, fy, cx, cy, bf, b), bounds, sf, th, mono)
        gq = m.debug_queries(len(kl), q_stride=1200)
        for f in ("u", "v", "ur", "radius", "minLevel", "maxLevel", "flags", "angle"):
            np.testing.assert_array_equal(gq[f], oq[f], err_msg=f)
        np.testing.assert_array_equal(gq["desc"][oq["flags"] & 1 == 1], oq["desc"][oq["flags"] & 1 == 1])
        onm, oqm, oqd, okm = oracle.search_by_projection(kc, uRc, dc, None, bounds, oq, 0.9, False, True)
        np.testing.assert_array_equal(qm, oqm)
        np.testing.assert_array_equal(qd, oqd)
        np.testing.assert_array_equal(km, okm)
        assert nm == onm and nm > 300, nm
        m.close()
    ex.close()
