"""GPU parity of the batch-of-sequences entry points of include/oslam_hip.h that the driver runs (matchers, BoW, stereo, pose optimisation), called
through the C ABI with torch tensors as device memory, on a non-default stream.  One launch covers a heterogeneous batch — counts {stride, 17, 0, 1,
stride / 2} read from a device array, a stride below the handle's capacity — and every test asserts, per element: parity with the oracle run on that
element alone (the criterion of the single-frame test of the operation), and independence of the batch (bitwise the same result when the element runs
alone with batch = 1 on the same handle and when the batch order is reversed).  tests/test_batch_frame_mappoint_gpu.py holds the entry points with
caller-owned outputs."""
import ctypes as C

import numpy as np
import pytest

from batch_common import (B, REV, SCALE, TUM1_D, TUM1_K, batch_counts, bow_pair, dev, fetch, match_frames, match_results, rand_frame, rand_queries, side_stream,
                          upload_frames, vp)
from object_slam_amd import KP_DTYPE, QUERY_DTYPE, synth
from object_slam_amd._lib import OSLAM_E_CAPACITY, check, lib
from object_slam_amd.matcher import BowJob, BowResident, Camera, MatchLast, feature_vector

pytestmark = pytest.mark.gpu

KS, QS, MAX_KPS, MAX_Q = 640, 1024, 2400, 4096    # strides of the batch / capacity of the handle
K_CACHE_CAP = 48                                   # kCacheCap of csrc/matcher.hip: a query with more gate-passing candidates replays uncached
PLAIN = (0.0, 0.0, 640.0, 480.0)
NNRATIO = 0.8
INV_SIGMA2 = (1.0 / (SCALE * SCALE)).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------------------------------------
# matcher
# --------------------------------------------------------------------------------------------------------------------------------------------

def _gate_passing(oracle, e, bounds):
    """Candidates per query that pass the window, level, blocked and uRight gates of SearchByProjection (what the kernel caches), on the CPU."""
    nk, nq = e["nk"], e["nq"]
    k, uR, bl, q = e["k"][:nk], e["uR"][:nk], e["blocked"][:nk], e["q"][:nq]
    out = np.zeros(nq, np.int64)
    for j in range(nq):
        if not q["flags"][j] & 1:
            continue
        idx = oracle.features_in_area(k, bounds, float(q["u"][j]), float(q["v"][j]), float(q["radius"][j]), int(q["minLevel"][j]), int(q["maxLevel"][j]))
        far = (uR[idx] > 0) & (np.abs(q["ur"][j] - uR[idx]) > q["radius"][j])
        out[j] = int(((bl[idx] == 0) & ~far).sum())
    return out


def _match_elements():
    rng = np.random.default_rng(4242)
    nk, nq = batch_counts(KS), batch_counts(QS)
    els = []
    for b in range(B):
        k, uR, desc = rand_frame(rng, KS, clustered=(b == 0))          # rows are valid up to the stride: the counts alone limit what is read
        n = max(int(nk[b]), 1)
        q = rand_queries(rng, k[:n], uR[:n], desc[:n], QS, 0.08)
        els.append(dict(k=k, uR=uR, desc=desc, blocked=(rng.random(KS) < 0.1).astype(np.uint8), q=q, nk=int(nk[b]), nq=int(nq[b])))
    # the clustered element: some queries search every level in a window that spans a whole cluster -> more than kCacheCap candidates
    q0 = els[0]["q"]
    q0["minLevel"][:16] = 0
    q0["maxLevel"][:16] = 7
    q0["radius"][:16] = 90.0
    q0["flags"][:16] |= 1
    return els


def _search(L, h, stream, D, row0, batch, bounds, mode, nk_const=None, nq_const=None):
    f = match_frames(D, row0, KS, bounds, nk_const)
    d_q = vp(D["q"], row0 * QS * QUERY_DTYPE.itemsize)
    d_nq = vp(D["nq"], row0 * 4) if nq_const is None else None
    s = C.c_void_p(stream.cuda_stream)
    if mode == "fuse":
        check(L.oslam_match_fuse_batch_device(h, C.byref(f), d_q, QS, d_nq, nq_const or 0, batch, C.c_void_p(INV_SIGMA2.ctypes.data), 8, s))
    else:
        use_ratio, check_ori = mode
        check(L.oslam_match_search_batch_device(h, C.byref(f), d_q, QS, d_nq, nq_const or 0, batch, C.c_float(NNRATIO), int(use_ratio), int(check_ori), 100, s))
    stream.synchronize()
    return match_results(L, h, batch, QS, KS)


def _same_element(got, i, want, j, nq, nk, fuse=False):
    """Row i of one result equals row j of another, over the element's own counts (bitwise: these are integers)."""
    assert got["nm"][i] == want["nm"][j]
    assert np.array_equal(got["qm"][i, :nq], want["qm"][j, :nq]) and np.array_equal(got["qd"][i, :nq], want["qd"][j, :nq])
    if not fuse:
        assert np.array_equal(got["km"][i, :nk], want["km"][j, :nk])


@pytest.fixture(scope="module")
def match_env():
    L = lib()
    h = C.c_void_p()
    check(L.oslam_matcher_create(C.byref(h), B, MAX_KPS, MAX_Q, 0))
    els = _match_elements()
    env = dict(L=L, h=h, els=els, D=upload_frames(els), Drev=upload_frames([els[b] for b in REV]), stream=side_stream())
    yield env
    L.oslam_matcher_destroy(h)


EUROC_K = (458.654, 457.296, 367.215, 248.375)                       # reference Examples/Monocular/EuRoC.yaml:8-16
EUROC_D = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)


def _undistorted_bounds(K, D):
    """mnMinX .. mnMaxY of a distorted 640 x 480 camera (Frame::ComputeImageBounds): every direct matcher test used the plain rectangle."""
    from object_slam_amd import FrameOps
    return tuple(float(v) for v in FrameOps().ComputeImageBounds(640, 480, K, D))


def _check_independence(run, els, fuse=False, counts=("nq", "nk")):
    """run(D-key, row0, batch) -> results.  Element b of the batch == the element alone (batch = 1, same handle) == its row in the reversed batch."""
    full = run("D", 0, B)
    rev = run("Drev", 0, B)
    alone = [run("D", b, 1) for b in range(B)]
    for b in range(B):
        nq, nk = els[b][counts[0]], els[b][counts[1]]
        _same_element(rev, int(np.where(REV == b)[0][0]), full, b, nq, nk, fuse)
        _same_element(alone[b], 0, full, b, nq, nk, fuse)
    return full, rev, alone


@pytest.mark.parametrize("use_ratio,check_ori,rect", [(True, False, "plain"), (False, True, "tum1"), (True, True, "euroc")])
def test_search_batch_device(oracle, match_env, use_ratio, check_ori, rect):
    """oslam_match_search_batch_device + oslam_match_results_device: both settings of the single-frame test, the second on the undistorted TUM1
    rectangle, and both gates together on the undistorted EuRoC rectangle; element 0 is clustered and holds queries beyond the candidate cache."""
    L, h, els, stream = match_env["L"], match_env["h"], match_env["els"], match_env["stream"]
    bounds = {"plain": PLAIN, "tum1": _undistorted_bounds(TUM1_K, TUM1_D), "euroc": _undistorted_bounds(EUROC_K, EUROC_D)}[rect]
    if rect == "tum1":    # TUM1's k1 > 0 pulls the corners inwards: minima above 0, keypoints left of / above the grid
        assert bounds[0] > 5 and bounds[1] > 5 and bounds[2] < 635 and bounds[3] < 475, bounds
    if rect == "euroc":   # k1 < 0 pushes them outwards: negative minima, the grid starts outside the image
        assert bounds[0] < -5 and bounds[1] < -5 and bounds[2] > 645 and bounds[3] > 485, bounds
    ncand = _gate_passing(oracle, els[0], bounds)
    assert int((ncand > K_CACHE_CAP).sum()) >= 4, np.sort(ncand)[-8:]                      # the uncached replay path really runs
    assert [e["nk"] for e in els] == [KS, 17, 0, 1, KS // 2] and [e["nq"] for e in els] == [QS, 17, 0, 1, QS // 2] and KS < MAX_KPS and QS < MAX_Q
    run = lambda key, row0, batch: _search(L, h, stream, match_env[key], row0, batch, bounds, (use_ratio, check_ori))
    got, _, _ = _check_independence(run, els)
    for b, e in enumerate(els):
        nk, nq = e["nk"], e["nq"]
        onm, oqm, oqd, okm = oracle.search_by_projection(e["k"][:nk], e["uR"][:nk], e["desc"][:nk], e["blocked"][:nk], bounds, e["q"][:nq], NNRATIO, use_ratio, check_ori)
        np.testing.assert_array_equal(got["qm"][b, :nq], oqm, err_msg="element %d" % b)
        np.testing.assert_array_equal(got["qd"][b, :nq], oqd, err_msg="element %d" % b)
        np.testing.assert_array_equal(got["km"][b, :nk], okm, err_msg="element %d" % b)     # [batch][kp_stride]: a [batch][max_keypoints] reader fails here for b > 0
        assert got["nm"][b] == onm
    assert got["nm"][0] > 50 and got["nm"][4] > 50 and got["nm"][2] == 0, got["nm"]
    # the counts as constants: the same results as the same counts in device arrays
    import torch
    c17 = dict(match_env["D"], nk=dev(np.full(B, 17, np.int32)), nq=dev(np.full(B, 17, np.int32)))
    torch.cuda.synchronize()
    a = _search(L, h, stream, c17, 0, B, bounds, (use_ratio, check_ori))
    c = _search(L, h, stream, match_env["D"], 0, B, bounds, (use_ratio, check_ori), nk_const=17, nq_const=17)
    for b in range(B):
        _same_element(c, b, a, b, 17, 17)


def test_fuse_batch_device(oracle, match_env):
    L, h, els, stream = match_env["L"], match_env["h"], match_env["els"], match_env["stream"]
    bounds = _undistorted_bounds(EUROC_K, EUROC_D)
    assert bounds[0] < -5 and bounds[1] < -5 and bounds[2] > 645 and bounds[3] > 485, bounds    # negative minima: the grid starts outside the image
    fels = []
    for e in els:                                                      # the windows of Fuse: th * scale of the predicted level (tests/test_matcher_gpu.py)
        q = e["q"].copy()
        q["radius"] = (3.0 * SCALE[np.clip(q["maxLevel"], 0, 7)]).astype(np.float32)
        fels.append(dict(e, q=q))
    env = dict(D=upload_frames(fels), Drev=upload_frames([fels[b] for b in REV]))
    import torch
    torch.cuda.synchronize()
    run = lambda key, row0, batch: _search(L, h, stream, env[key], row0, batch, bounds, "fuse")
    got, _, _ = _check_independence(run, fels, fuse=True)
    for b, e in enumerate(fels):
        nk, nq = e["nk"], e["nq"]
        onf, oqm, oqd = oracle.fuse_search(e["k"][:nk], e["uR"][:nk], e["desc"][:nk], bounds, e["q"][:nq], INV_SIGMA2)
        np.testing.assert_array_equal(got["qm"][b, :nq], oqm, err_msg="element %d" % b)
        np.testing.assert_array_equal(got["qd"][b, :nq], oqd, err_msg="element %d" % b)
        assert got["nm"][b] == onf
    assert got["nm"][0] > 10 and got["nm"][4] > 10, got["nm"]
    c17 = dict(env["D"], nk=dev(np.full(B, 17, np.int32)), nq=dev(np.full(B, 17, np.int32)))
    torch.cuda.synchronize()
    a = _search(L, h, stream, c17, 0, B, bounds, "fuse")
    c = _search(L, h, stream, env["D"], 0, B, bounds, "fuse", nk_const=17, nq_const=17)
    for b in range(B):
        _same_element(c, b, a, b, 17, 17, fuse=True)


def test_search_refuses_a_stride_above_the_capacity(match_env):
    """One rule for kp_stride: 1 .. max_keypoints of the handle.  Above it the call fails with OSLAM_E_CAPACITY before anything is launched."""
    L, h, D = match_env["L"], match_env["h"], match_env["D"]
    for stride in (MAX_KPS + 1, MAX_KPS * 64, MAX_KPS * 64 + 1):
        f = match_frames(D, 0, KS, PLAIN)
        f.kp_stride = stride
        rc = L.oslam_match_search_batch_device(h, C.byref(f), vp(D["q"]), QS, vp(D["nq"]), 0, 1, C.c_float(NNRATIO), 1, 0, 100, None)
        assert rc == OSLAM_E_CAPACITY, (stride, rc)
        assert b"kp_stride" in L.oslam_last_error()
        rc = L.oslam_match_fuse_batch_device(h, C.byref(f), vp(D["q"]), QS, vp(D["nq"]), 0, 1, C.c_void_p(INV_SIGMA2.ctypes.data), 8, None)
        assert rc == OSLAM_E_CAPACITY, (stride, rc)
    f = match_frames(D, 0, KS, PLAIN, nk_const=0)
    f.kp_stride = MAX_KPS                                              # the bound itself is accepted (no keypoints, no queries: nothing is read)
    assert L.oslam_match_search_batch_device(h, C.byref(f), vp(D["q"]), QS, None, 0, 1, C.c_float(NNRATIO), 1, 0, 100, None) == 0
    import torch
    torch.cuda.synchronize()


CAM = (520.908620, 521.007327, 325.141442, 249.701764, 40.0, 40.0 / 520.908620)


def _last_elements(els):
    """A last frame per element whose map points project near the element's current keypoints, with its own Tcw / Tlw: Tlw = Tcw (no forward / backward
    motion), the camera moved forward, and backward, by more than the baseline (the three level gates of src/ORBmatcher.cc:1377-1392)."""
    rng = np.random.default_rng(777)
    fx, fy, cx, cy = CAM[:4]
    nl = batch_counts(KS)
    out = []
    for b, e in enumerate(els):
        n = max(e["nk"], 1)
        src = rng.integers(0, n, KS)
        Tcw = synth.make_T(rng.normal(0, 0.05, 3), rng.normal(0, 0.2, 3)).astype(np.float32)
        z = rng.uniform(1.0, 5.0, KS)
        u = e["k"]["x"][src] + rng.normal(0, 2, KS)
        v = e["k"]["y"][src] + rng.normal(0, 2, KS)
        Xc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
        Xc[::37, 2] *= -1                                              # behind the camera
        Xw = ((Xc - Tcw[:3, 3].astype(np.float64)) @ Tcw[:3, :3].astype(np.float64)).astype(np.float32)
        keys = np.zeros(KS, KP_DTYPE)
        keys["octave"] = np.clip(e["k"]["octave"][src] + rng.integers(-1, 2, KS), 0, 7)
        keys["angle"] = (e["k"]["angle"][src] + rng.normal(0, 10, KS)) % 360
        mp_desc = e["desc"][src] ^ np.packbits(rng.random((KS, 256)) < 0.06, axis=1, bitorder="little")
        has_mp = (rng.random(KS) < 0.9).astype(np.uint8) | ((rng.random(KS) < 0.7).astype(np.uint8) << 1)
        Tlw = Tcw.copy()
        Tlw[2, 3] += (0.0, 0.5, -0.5, 0.0, -0.5)[b]                     # tlc.z = Tlw.z - Tcw.z for equal rotations: > b forward, < -b backward
        out.append(dict(Xw=Xw, has_mp=has_mp, keys=keys, mp_desc=mp_desc, Tcw=Tcw, Tlw=Tlw, nl=int(nl[b])))
    return out


def test_project_last_batch_device_then_search(oracle, match_env):
    """oslam_match_project_last_batch_device fills the handle's query buffer for every element from its own Tcw / Tlw; the search that follows reads it
    (d_queries = NULL) with the counts the projection left on the device."""
    L, h, els, stream = match_env["L"], match_env["h"], match_env["els"], match_env["stream"]
    bounds = PLAIN
    last = _last_elements(els)
    assert CAM[5] < 0.4      # the +-0.5 m steps above exceed the baseline
    def up(order):
        st = lambda f: np.stack([last[b][f] for b in order])
        return dict(Xw=dev(st("Xw")), has_mp=dev(st("has_mp")), keys=dev(st("keys")), mp_desc=dev(st("mp_desc")), Tcw=dev(st("Tcw")), Tlw=dev(st("Tlw")),
                    nl=dev(np.array([last[b]["nl"] for b in order], np.int32)))
    import torch
    ld = dict(D=up(range(B)), Drev=up(REV))
    ld["c17"] = dict(ld["D"], nl=dev(np.full(B, 17, np.int32)))
    cur_env = dict(D=match_env["D"], Drev=match_env["Drev"], c17=match_env["D"])
    torch.cuda.synchronize()
    cam = Camera(*[float(x) for x in CAM])
    sf = np.ascontiguousarray(SCALE)
    s = C.c_void_p(stream.cuda_stream)

    def run(key, row0, batch, nl_const=None):
        D, Ld = cur_env[key], ld[key]
        cur = match_frames(D, row0, KS, bounds)
        ml = MatchLast()
        ml.Xw, ml.has_mp = Ld["Xw"].data_ptr() + row0 * KS * 12, Ld["has_mp"].data_ptr() + row0 * KS
        ml.keys, ml.mp_desc, ml.kp_stride = Ld["keys"].data_ptr() + row0 * KS * KP_DTYPE.itemsize, Ld["mp_desc"].data_ptr() + row0 * KS * 32, KS
        if nl_const is None:
            ml.n_kps, ml.n_kps_const = Ld["nl"].data_ptr() + row0 * 4, -1
        else:
            ml.n_kps, ml.n_kps_const = None, nl_const
        check(L.oslam_match_project_last_batch_device(h, C.byref(ml), vp(Ld["Tcw"], row0 * 64), vp(Ld["Tlw"], row0 * 64), C.byref(cam), C.byref(cur),
                                                      C.c_void_p(sf.ctypes.data), 8, C.c_float(15.0), 0, batch, s))
        pq, pn = C.c_void_p(), C.c_void_p()
        check(L.oslam_match_results_device(h, None, None, None, None, C.byref(pq), C.byref(pn)))
        check(L.oslam_match_search_batch_device(h, C.byref(cur), None, KS, pn, 0, batch, C.c_float(0.9), 0, 1, 100, s))
        stream.synchronize()
        r = match_results(L, h, batch, KS, KS)
        r["queries"] = fetch(L, pq, batch * KS, QUERY_DTYPE).reshape(batch, KS)
        r["n_queries"] = fetch(L, pn, batch, np.int32)
        return r

    lels = [dict(nq=l["nl"], nk=e["nk"]) for l, e in zip(last, els)]
    got, rev, alone = _check_independence(run, lels)
    gates = set()
    for b, (l, e) in enumerate(zip(last, els)):
        nl, nk = l["nl"], e["nk"]
        oq = oracle.project_last_frame(l["Xw"][:nl], l["has_mp"][:nl], l["keys"][:nl], l["mp_desc"][:nl], l["Tcw"], l["Tlw"], CAM, bounds, SCALE, 15.0, False)
        gq = got["queries"][b, :nl]
        assert got["n_queries"][b] == nl
        for f in ("u", "v", "ur", "radius", "minLevel", "maxLevel", "flags", "angle"):
            np.testing.assert_array_equal(gq[f], oq[f], err_msg="%s of element %d" % (f, b))
        act = oq["flags"] & 1 == 1
        np.testing.assert_array_equal(gq["desc"][act], oq["desc"][act])
        assert np.array_equal(rev["queries"][int(np.where(REV == b)[0][0]), :nl].view(np.uint8), gq.view(np.uint8)) and np.array_equal(alone[b]["queries"][0, :nl].view(np.uint8), gq.view(np.uint8))
        if act.any():
            gates.add("fwd" if (oq["maxLevel"][act] == -1).all() else "bwd" if (oq["minLevel"][act] == 0).all() and (oq["maxLevel"][act] == l["keys"]["octave"][:nl][act]).all() else "none")
        onm, oqm, oqd, okm = oracle.search_by_projection(e["k"][:nk], e["uR"][:nk], e["desc"][:nk], e["blocked"][:nk], bounds, oq, 0.9, False, True)
        np.testing.assert_array_equal(got["qm"][b, :nl], oqm, err_msg="element %d" % b)
        np.testing.assert_array_equal(got["qd"][b, :nl], oqd, err_msg="element %d" % b)
        np.testing.assert_array_equal(got["km"][b, :nk], okm, err_msg="element %d" % b)
        assert got["nm"][b] == onm
    assert gates == {"fwd", "bwd", "none"}, gates                       # every element really used its own Tlw
    assert got["nm"][0] > 100 and got["nm"][4] > 50, got["nm"]
    # the last frame's counts as a constant
    a, c = run("D", 0, B, nl_const=17), run("c17", 0, B)
    for b in range(B):
        _same_element(a, b, c, b, 17, els[b]["nk"])
    # the same two calls through ORBmatcher.project_last_batch_device / search_batch_device on a handle of their own
    from object_slam_amd import ORBmatcher
    m = ORBmatcher(0.9, True, max_keypoints=MAX_KPS, max_queries=MAX_Q, max_batch=B)
    D, Ld = cur_env["D"], ld["D"]
    cur = match_frames(D, 0, KS, bounds)
    ml = MatchLast()
    ml.Xw, ml.has_mp, ml.keys, ml.mp_desc, ml.kp_stride = Ld["Xw"].data_ptr(), Ld["has_mp"].data_ptr(), Ld["keys"].data_ptr(), Ld["mp_desc"].data_ptr(), KS
    ml.n_kps, ml.n_kps_const = Ld["nl"].data_ptr(), -1
    m.project_last_batch_device(ml, Ld["Tcw"].data_ptr(), Ld["Tlw"].data_ptr(), CAM, cur, SCALE, 15.0, False, B, stream.cuda_stream)
    pn = C.c_void_p()
    check(L.oslam_match_results_device(m.h, None, None, None, None, None, C.byref(pn)))
    m.search_batch_device(cur, None, KS, pn.value, 0, B, False, True, stream.cuda_stream)
    for b, (l, e) in enumerate(zip(last, els)):
        nm, qm, qd, km, _ = m.fetch(b, KS, l["nl"], KS, e["nk"], stream.cuda_stream)
        assert nm == got["nm"][b] and np.array_equal(qm, got["qm"][b, :l["nl"]]) and np.array_equal(qd, got["qd"][b, :l["nl"]]) and np.array_equal(km, got["km"][b, :e["nk"]]), b
    m.close()


# --------------------------------------------------------------------------------------------------------------------------------------------
# BoW matchers
# --------------------------------------------------------------------------------------------------------------------------------------------

F12 = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
SIGMA2 = (SCALE * SCALE).astype(np.float32)
GUARD = 8          # sentinel words behind every match array


def _bow_jobs():
    """(triangulation, N1, N2, nodes): SearchByBoW and SearchForTriangulation mixed, an empty side 1, a job whose FeatureVectors share no node."""
    rng = np.random.default_rng(31)
    spec = [(1, 640, 640, 40), (1, 17, 30, 3), (0, 0, 50, 5), (0, 1, 1, 1), (1, 320, 400, 20), (0, 200, 150, 12), (0, 640, 600, 60)]
    jobs = []
    for i, (tri, N1, N2, nn) in enumerate(spec):
        k1, uR1, d1, node1, k2, uR2, d2, node2 = bow_pair(rng, max(N1, 1), N2, nn)
        if N1 == 0:
            k1, uR1, d1, node1 = k1[:0], uR1[:0], d1[:0], node1[:0]
        if i == 5:
            node2 = node2 + 1000
        jobs.append(dict(tri=tri, k1=k1, uR1=uR1, d1=d1, node1=node1, k2=k2, uR2=uR2, d2=d2, node2=node2, flag1=(rng.random(N1) < (0.4 if tri else 0.8)).astype(np.uint8),
                         mp2=(rng.random(N2) < 0.4).astype(np.uint8), F12=(F12 + rng.normal(0, 1e-7, (3, 3))).astype(np.float32), ratio=(0.7, 0.9)[i % 2], ori=i % 3 != 2))
    return jobs


def _bow_reference(oracle, j):
    if j["tri"]:
        return oracle.search_for_triangulation(j["k1"], j["d1"], j["uR1"], j["flag1"], j["node1"], j["k2"], j["d2"], j["uR2"], j["mp2"], j["node2"], j["F12"], 700.0, 240.0,
                                               SCALE, SIGMA2, False, j["ori"])
    return oracle.search_by_bow(j["k1"], j["d1"], j["flag1"], j["node1"], j["k2"], j["d2"], j["node2"], j["ratio"], j["ori"])


def _bow_struct(j, keep, resident=(False, False)):
    """The job struct over host arrays; a resident side gets ZEROED host keypoints / descriptors / uRight, so a kernel that read them would not match."""
    job = BowJob()
    a = lambda x, dt: keep.append(np.ascontiguousarray(x, dt)) or keep[-1]
    blank = lambda x, dt: keep.append(np.zeros_like(np.ascontiguousarray(x, dt))) or keep[-1]
    qi, qn, _, _, _ = feature_vector(j["node1"])
    _, _, nodes, start, items = feature_vector(j["node2"])
    s1, s2 = job.s1, job.s2
    pick1, pick2 = (blank if resident[0] else a), (blank if resident[1] else a)
    s1.N, s1.keys, s1.desc, s1.uRight, s1.flag = len(j["k1"]), pick1(j["k1"], KP_DTYPE).ctypes.data, pick1(j["d1"], np.uint8).ctypes.data, pick1(j["uR1"], np.float32).ctypes.data, a(j["flag1"], np.uint8).ctypes.data
    s1.nq, s1.q_idx, s1.q_node = len(qi), a(qi, np.int32).ctypes.data, a(qn, np.uint32).ctypes.data
    s2.N, s2.keys, s2.desc, s2.uRight, s2.has_mp = len(j["k2"]), pick2(j["k2"], KP_DTYPE).ctypes.data, pick2(j["d2"], np.uint8).ctypes.data, pick2(j["uR2"], np.float32).ctypes.data, (a(j["mp2"], np.uint8).ctypes.data if j["tri"] else None)
    s2.nNodes, s2.nodes, s2.start, s2.items = len(nodes), a(nodes, np.uint32).ctypes.data, a(start, np.int32).ctypes.data, a(items, np.int32).ctypes.data
    job.triangulation, job.nnratio, job.checkOri = j["tri"], j["ratio"], int(j["ori"])
    job.F12[:] = [float(v) for v in j["F12"].reshape(-1)]
    job.ex, job.ey = 700.0, 240.0
    nout = s1.N if j["tri"] else s2.N
    out = a(np.full(nout + GUARD, -1, np.int32), np.int32)             # 0xFF bytes
    job.match, job.nmatches = out.ctypes.data, 12345
    return job, out, nout


def _run_bow(L, h, jobs, res_spec=None, res_dev=None):
    keep, structs, outs = [], [], []
    for i, j in enumerate(jobs):
        r = res_spec[i] if res_spec else (False, False)
        st, out, nout = _bow_struct(j, keep, r)
        structs.append(st); outs.append((out, nout))
    arr = (BowJob * len(jobs))(*structs)
    sf, s2 = np.ascontiguousarray(SCALE), np.ascontiguousarray(SIGMA2)
    if res_spec is None:
        check(L.oslam_match_bow_batch(h, len(jobs), arr, C.c_void_p(sf.ctypes.data), C.c_void_p(s2.ctypes.data), 8))
    else:
        res = (BowResident * len(jobs))()
        for i, (r1, r2) in enumerate(res_spec):
            if r1:
                res[i].d_keys1, res[i].d_desc1, res[i].d_uRight1 = [t.data_ptr() for t in res_dev[i][0]]
            if r2:
                res[i].d_keys2, res[i].d_desc2, res[i].d_uRight2 = [t.data_ptr() for t in res_dev[i][1]]
        check(L.oslam_match_bow_batch_resident(h, len(jobs), arr, res, C.c_void_p(sf.ctypes.data), C.c_void_p(s2.ctypes.data), 8))
    got = []
    for i, (out, nout) in enumerate(outs):
        assert (out[nout:] == -1).all()                                 # nothing behind match [nout]
        got.append((arr[i].nmatches, out[:nout].copy()))
    return got


@pytest.fixture(scope="module")
def bow_env(oracle):
    L = lib()
    h = C.c_void_p()
    check(L.oslam_bow_create(C.byref(h), MAX_KPS, 0))
    jobs = _bow_jobs()
    assert len(jobs[2]["k1"]) == 0 and jobs[2]["tri"] == 0                                # the s1.N = 0 job
    assert len(np.intersect1d(jobs[5]["node1"], jobs[5]["node2"])) == 0                    # the job whose nodes do not intersect
    assert all(len(np.intersect1d(j["node1"], j["node2"])) for i, j in enumerate(jobs) if i not in (2, 5))
    yield dict(L=L, h=h, jobs=jobs, ref=[_bow_reference(oracle, j) for j in jobs])
    L.oslam_bow_destroy(h)


def _check_bow(got, ref, order=None):
    for i, (nm, m) in enumerate(got):
        onm, om = ref[i if order is None else order[i]]
        np.testing.assert_array_equal(m, om, err_msg="job %d" % i)
        assert nm == onm, (i, nm, onm)


def test_bow_batch(bow_env):
    L, h, jobs, ref = bow_env["L"], bow_env["h"], bow_env["jobs"], bow_env["ref"]
    got = _run_bow(L, h, jobs)
    _check_bow(got, ref)
    assert ref[5][0] == 0 and ref[2][0] == 0 and ref[0][0] > 5 and ref[4][0] > 5 and ref[6][0] > 5, [r[0] for r in ref]
    order = list(range(len(jobs)))[::-1]
    rev = _run_bow(L, h, [jobs[i] for i in order])
    for i, o in enumerate(order):                                       # independence: reversed order and every job alone
        assert rev[i][0] == got[o][0] and np.array_equal(rev[i][1], got[o][1])
    for i, j in enumerate(jobs):
        (nm, m), = _run_bow(L, h, [j])
        assert nm == got[i][0] and np.array_equal(m, got[i][1])


def test_bow_batch_resident(bow_env):
    """All six resident pointers (job 0), side 2 only (job 4), none (the host fallback, every other job) in ONE call; the host arrays of a resident
    side are zeroed, so the result proves which memory the kernel read."""
    L, h, jobs, ref = bow_env["L"], bow_env["h"], bow_env["jobs"], bow_env["ref"]
    spec = [(True, True), (False, False), (False, False), (False, False), (False, True), (False, False), (False, False)]
    assert jobs[0]["tri"] and jobs[4]["tri"]                             # triangulation reads uRight of both sides: all six pointers matter
    res_dev = [((dev(j["k1"]), dev(j["d1"]), dev(j["uR1"])), (dev(j["k2"]), dev(j["d2"]), dev(j["uR2"]))) if any(s) else None for j, s in zip(jobs, spec)]
    import torch
    torch.cuda.synchronize()                                            # "the resident arrays must be complete when the call is made"
    got = _run_bow(L, h, jobs, spec, res_dev)
    _check_bow(got, ref)
    order = list(range(len(jobs)))[::-1]
    rev = _run_bow(L, h, [jobs[i] for i in order], [spec[i] for i in order], [res_dev[i] for i in order])
    for i, o in enumerate(order):
        assert rev[i][0] == got[o][0] and np.array_equal(rev[i][1], got[o][1])
    for i in (0, 4):
        (nm, m), = _run_bow(L, h, [jobs[i]], [spec[i]], [res_dev[i]])
        assert nm == got[i][0] and np.array_equal(m, got[i][1])


# --------------------------------------------------------------------------------------------------------------------------------------------
# stereo
# --------------------------------------------------------------------------------------------------------------------------------------------

SW, SH, SNF, SLEVELS = 320, 240, 300, 5          # the golden fixture's extractor configuration
SBF = 47.9
SB = SBF / 458.6


def _stereo_pairs():
    disps = (9, 21, 4, 9)
    L, R = [], []
    for i, d in enumerate(disps):
        canvas = synth.make_canvas(SW + 100, SH + 32, seed=60 + i)
        L.append(np.ascontiguousarray(canvas[10:10 + SH, 40:40 + SW]))
        r = np.ascontiguousarray(canvas[10:10 + SH, 40 + d:40 + d + SW])
        rng = np.random.default_rng(60 + i)
        R.append(np.clip(r.astype(np.int32) + rng.integers(-2, 3, r.shape), 0, 255).astype(np.uint8))
    R[3] = np.full((SH, SW), 90, np.uint8)                               # a blank right image: no right keypoints
    assert len(set(disps[:3])) == 3
    return np.stack(L), np.stack(R)


def test_stereo_match_batch_device(oracle):
    """oslam_stereo_match_batch_device + oslam_stereo_results_device on four pairs extracted by extract_batch_device on two handles: pair b must read
    keypoints b AND pyramid b of both extractors."""
    import torch
    from object_slam_amd import ORBextractor
    Lb = lib()
    imL, imR = _stereo_pairs()
    NP = len(imL)
    exL, exR = (ORBextractor(SNF, 1.2, SLEVELS, 20, 7, SW, SH, max_batch=NP) for _ in range(2))
    cap = exL.cap
    h = C.c_void_p()
    check(Lb.oslam_stereo_create(C.byref(h), NP, MAX_KPS, 0))
    assert cap < MAX_KPS                                                 # kp_stride below the handle's capacity
    stream = side_stream()
    s = stream.cuda_stream

    def run(order):
        dL, dR = dev(imL[order]), dev(imR[order])
        torch.cuda.synchronize()
        n = len(order)
        exL.extract_batch_device(dL.data_ptr(), n, SW, SW * SH, s)
        exR.extract_batch_device(dR.data_ptr(), n, SW, SW * SH, s)
        kpL, deL, nL, stL = exL.results_device()
        kpR, deR, nR, stR = exR.results_device()
        check(Lb.oslam_stereo_match_batch_device(h, exL.h, exR.h, n, cap, C.c_void_p(kpL), C.c_void_p(deL), C.c_void_p(nL), 0, C.c_void_p(kpR), C.c_void_p(deR), C.c_void_p(nR), 0,
                                                 SLEVELS, C.c_float(SBF), C.c_float(SB), C.c_void_p(s)))
        stream.synchronize()
        pu, pd, pn = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(Lb.oslam_stereo_results_device(h, C.byref(pu), C.byref(pd), C.byref(pn)))
        r = dict(uR=fetch(Lb, pu, n * cap, np.float32).reshape(n, cap), dep=fetch(Lb, pd, n * cap, np.float32).reshape(n, cap), nm=fetch(Lb, pn, n, np.int32),
                 nL=fetch(Lb, C.c_void_p(nL), n, np.int32), nR=fetch(Lb, C.c_void_p(nR), n, np.int32))
        assert fetch(Lb, C.c_void_p(stL), 1, np.int32)[0] == 0 and fetch(Lb, C.c_void_p(stR), 1, np.int32)[0] == 0
        r["keys"] = [(exL.fetch(b), exR.fetch(b)) for b in range(n)]
        return r

    got = run(np.arange(NP))
    rev = run(np.arange(NP)[::-1].copy())
    assert got["nR"][3] == 0 and (got["nR"][:3] > 50).all() and (got["nL"] > 50).all(), (got["nL"], got["nR"])
    assert len(set(got["nL"].tolist())) > 1                             # unequal counts
    disps = []
    for b in range(NP):
        oL, oR = oracle.OrbExtractor(SNF, 1.2, SLEVELS, 20, 7), oracle.OrbExtractor(SNF, 1.2, SLEVELS, 20, 7)
        okL, odL = oL.extract(imL[b])
        okR, odR = oR.extract(imR[b])
        (kL, dL), (kR, dR) = got["keys"][b]
        assert kL.tobytes() == okL.tobytes() and kR.tobytes() == okR.tobytes() and dL.tobytes() == odL.tobytes()
        n = len(okL)
        assert got["nL"][b] == n and got["nR"][b] == len(okR)
        ouR, odep, on = oracle.stereo_matches(oL, oR, okL, odL, okR, odR, SBF, SB, with_count=True)
        assert np.array_equal(got["uR"][b, :n].view(np.uint32), ouR.view(np.uint32)), b
        assert np.array_equal(got["dep"][b, :n].view(np.uint32), odep.view(np.uint32)), b
        # n_matched counts the matches BEFORE the median-SAD cut: the oracle's vDistIdx.size().  The cut keeps every match whose SAD is at most the
        # median (element n_matched / 2 of the sorted list) unless the median is 0, so: kept <= n_matched, and kept >= n_matched / 2 + 1.
        assert got["nm"][b] == on, (b, got["nm"][b], on)
        kept = int((ouR >= 0).sum())
        assert kept <= got["nm"][b] and (kept == 0 or kept >= got["nm"][b] // 2 + 1), (b, kept, got["nm"][b])
        if len(okR) == 0:
            assert got["nm"][b] == 0 and kept == 0
        else:
            assert kept > 30, (b, kept)
            m = ouR >= 0
            disps.append(float(np.median(okL["x"][m] - ouR[m])))
        # independence: the reversed batch and the pair alone (extracted alone: batch = 1 on the same three handles)
        rb = NP - 1 - b
        alone = run(np.array([b]))
        for other, row in ((rev, rb), (alone, 0)):
            assert other["nL"][row] == n and other["nm"][row] == got["nm"][b]
            assert np.array_equal(other["uR"][row, :n].view(np.uint32), got["uR"][b, :n].view(np.uint32)) and np.array_equal(other["dep"][row, :n].view(np.uint32), got["dep"][b, :n].view(np.uint32))
    assert all(abs(d - w) < 0.6 for d, w in zip(disps, (9, 21, 4))), disps
    # the counts as constants agree with the same counts in device arrays: on the three pairs that have right keypoints, so that every row read
    # below the constant was written by this extraction
    NC = 3
    dL, dR = dev(imL[:NC]), dev(imR[:NC])
    torch.cuda.synchronize()
    exL.extract_batch_device(dL.data_ptr(), NC, SW, SW * SH, s)
    exR.extract_batch_device(dR.data_ptr(), NC, SW, SW * SH, s)
    kpL, deL, nL, _ = exL.results_device()
    kpR, deR, nR, _ = exR.results_device()
    nmin = int(min(got["nL"][:NC].min(), got["nR"][:NC].min()))
    assert nmin > 50
    cn = dev(np.full(NC, nmin, np.int32))
    torch.cuda.synchronize()
    res = []
    for counts in ((C.c_void_p(cn.data_ptr()), 0), (None, nmin)):
        check(Lb.oslam_stereo_match_batch_device(h, exL.h, exR.h, NC, cap, C.c_void_p(kpL), C.c_void_p(deL), counts[0], counts[1], C.c_void_p(kpR), C.c_void_p(deR), counts[0], counts[1],
                                                 SLEVELS, C.c_float(SBF), C.c_float(SB), C.c_void_p(s)))
        stream.synchronize()
        pu, pd, pn = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(Lb.oslam_stereo_results_device(h, C.byref(pu), C.byref(pd), C.byref(pn)))
        res.append((fetch(Lb, pu, NC * cap, np.float32).reshape(NC, cap)[:, :nmin].copy(), fetch(Lb, pd, NC * cap, np.float32).reshape(NC, cap)[:, :nmin].copy(), fetch(Lb, pn, NC, np.int32)))
    for x, y in zip(*res):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    Lb.oslam_stereo_destroy(h)
    exL.close(); exR.close()


# --------------------------------------------------------------------------------------------------------------------------------------------
# pose optimisation
# --------------------------------------------------------------------------------------------------------------------------------------------

PS, PMAX = 600, 1024
RTOL = 1e-4          # tests/test_poseopt_gpu.py


def _rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def test_pose_optimize_batch_device_with_device_counts(oracle):
    """oslam_pose_optimize_batch_device with d_n = {stride, 17, 0, 1, stride / 2} and stride < max_points: elements 2 and 3 have fewer than three
    correspondences (pose untouched, 0 inliers)."""
    import torch
    L = lib()
    n = batch_counts(PS)
    probs = [synth.make_pose_problem(300 + b, N=PS, outlier_frac=(0.1, 0.0, 0.2, 0.2, 0.3)[b]) for b in range(B)]
    for b in (2, 3):
        assert int(probs[b]["has_mp"][:n[b]].sum()) < 3                  # fewer than 3 correspondences
    for b in (0, 1, 4):
        assert int(probs[b]["has_mp"][:n[b]].sum()) >= 10
    h = C.c_void_p()
    check(L.oslam_poseopt_create(C.byref(h), B, PMAX, 0))
    K5 = np.asarray(probs[0]["K"], np.float32)
    stream = side_stream()

    def up(order):
        t = lambda k, dt: dev(np.stack([probs[b][k] for b in order]).astype(dt))
        return dict(T=t("Tcw", np.float32), Xw=t("Xw", np.float32), obs=t("obs", np.float32), inv=t("invSigma2", np.float32), has=t("has_mp", np.uint8), n=dev(n[list(order)]))

    def run(D, row0, batch, n_const=None):
        check(L.oslam_pose_optimize_batch_device(h, batch, PS, vp(D["n"], row0 * 4) if n_const is None else None, n_const or 0, vp(D["T"], row0 * 64), vp(D["Xw"], row0 * PS * 12),
                                                 vp(D["obs"], row0 * PS * 12), vp(D["inv"], row0 * PS * 4), vp(D["has"], row0 * PS), C.c_void_p(K5.ctypes.data), C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        pT, pO, pN = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(L.oslam_poseopt_results_device(h, C.byref(pT), C.byref(pO), C.byref(pN), None))
        return dict(T=fetch(L, pT, batch * 16, np.float32).reshape(batch, 4, 4), outl=fetch(L, pO, batch * PS, np.uint8).reshape(batch, PS), ninl=fetch(L, pN, batch, np.int32))

    D, Drev = up(range(B)), up(REV)
    torch.cuda.synchronize()
    got, rev = run(D, 0, B), run(Drev, 0, B)
    for b, p in enumerate(probs):
        nb = int(n[b])
        on, oT, ooutl, _ = oracle.pose_optimization(p["Tcw"], p["Xw"][:nb], p["obs"][:nb], p["invSigma2"][:nb], p["has_mp"][:nb], p["K"])
        assert got["ninl"][b] == on, (b, got["ninl"][b], on)
        assert _rel(got["T"][b], oT) <= RTOL, (b, got["T"][b], oT)
        np.testing.assert_array_equal(got["outl"][b, :nb], ooutl, err_msg="element %d" % b)
        if b in (2, 3):
            assert on == 0 and np.array_equal(got["T"][b], p["Tcw"].astype(np.float32).reshape(4, 4)) and not got["outl"][b, :nb].any()
        alone = run(D, b, 1)
        for other, row in ((rev, int(np.where(REV == b)[0][0])), (alone, 0)):
            assert other["ninl"][row] == got["ninl"][b] and np.array_equal(other["outl"][row, :nb], got["outl"][b, :nb])
            assert np.array_equal(other["T"][row].view(np.uint32), got["T"][b].view(np.uint32)), b
    assert got["ninl"][0] > 200 and got["ninl"][4] > 100, got["ninl"]
    c17 = dict(D, n=dev(np.full(B, 17, np.int32)))
    torch.cuda.synchronize()
    a, c = run(c17, 0, B), run(D, 0, B, n_const=17)
    assert np.array_equal(a["T"].view(np.uint32), c["T"].view(np.uint32)) and np.array_equal(a["ninl"], c["ninl"]) and np.array_equal(a["outl"][:, :17], c["outl"][:, :17])
    L.oslam_poseopt_destroy(h)
