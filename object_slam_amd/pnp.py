"""ctypes view of the PnP solver (include/oslam_hip.h, "PnP solver"): ORB_SLAM2::PnPsolver (src/PnPsolver.cc, EPnP inside RANSAC) for batches of
independent problems, the numerical operator of Tracking::Relocalization (src/Tracking.cc:1650-1676).

`ransac_params` (SetRansacParameters) and `draw` (the counter-based generator and the swap-with-back rule) run on the host.  `PnPsolver.ransac_batch`
and `PnPsolver.epnp` run the gfx950 kernels (no CPU fallback: creating a PnPsolver fails without a device); the module-level `ransac_batch` and `epnp`
create a solver of the right size for one call.
"""
import ctypes as C

import numpy as np

from ._lib import Handle, check, device_call, lib, optptr, ptr

REFERENCE_PARAMS = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991)   # src/Tracking.cc:1660


class Params(C.Structure):       # oslam_pnp_params_t
    _fields_ = [("probability", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("min_set", C.c_int32), ("epsilon", C.c_float),
                ("th2", C.c_float), ("reserved", C.c_int32)]


class Problem(C.Structure):      # oslam_pnp_problem_t
    _fields_ = [("count", C.c_int32), ("offset", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("seed", C.c_uint32),
                ("reserved", C.c_int32)]


class Ransac(C.Structure):       # oslam_pnp_ransac_t
    _fields_ = [("min_inliers", C.c_int32), ("epsilon", C.c_float), ("iterations", C.c_int32), ("no_more", C.c_int32)]


PROBLEM_DTYPE = np.dtype([("count", "<i4"), ("offset", "<i4"), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("seed", "<u4"), ("reserved", "<i4")])
KIND_NONE, KIND_REFINED, KIND_BEST = 0, 1, 2


def _bind(L):
    if getattr(L, "_oslam_pnp_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int
    L.oslam_pnp_ransac_params.argtypes = [i32, C.c_double, i32, i32, i32, C.c_float, vp]
    L.oslam_pnp_draw.argtypes = [C.c_uint32, i32, i32, vp]
    L.oslam_pnp_create.argtypes = [C.POINTER(vp), i32, i32, i32]
    L.oslam_pnp_destroy.argtypes = [vp]
    L.oslam_pnp_destroy.restype = None
    L.oslam_pnp_ransac_batch.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.oslam_pnp_ransac_batch_device.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.oslam_pnp_epnp.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L._oslam_pnp_bound = True
    return L


def make_params(**kw):
    p = dict(REFERENCE_PARAMS, **kw)
    return Params(p["probability"], p["min_inliers"], p["max_iterations"], p["min_set"], p["epsilon"], p["th2"], 0)


def ransac_params(N, probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5):
    """SetRansacParameters (src/PnPsolver.cc:121-157): dict(min_inliers, epsilon, iterations, no_more) for N correspondences.  Host only."""
    out = Ransac()
    check(_bind(lib()).oslam_pnp_ransac_params(int(N), probability, min_inliers, max_iterations, min_set, epsilon, C.addressof(out)))
    return dict(min_inliers=out.min_inliers, epsilon=out.epsilon, iterations=out.iterations, no_more=bool(out.no_more))


def draw(seed, iteration, N):
    """The four correspondence indices iteration `iteration` of a problem with N correspondences draws from `seed`.  Host only."""
    out = np.zeros(4, np.int32)
    check(_bind(lib()).oslam_pnp_draw(int(seed) & 0xffffffff, int(iteration), int(N), ptr(out)))
    return out


def pack_problems(counts, K4, seeds, offsets=None):
    counts = np.asarray(counts, np.int32)
    n = len(counts)
    pr = np.zeros(n, PROBLEM_DTYPE)
    pr["count"] = counts
    pr["offset"] = np.concatenate([[0], np.cumsum(counts)[:-1]]) if offsets is None and n else (offsets if n else 0)
    K4 = np.broadcast_to(np.asarray(K4, np.float32), (n, 4))
    pr["fx"], pr["fy"], pr["cx"], pr["cy"] = K4[:, 0], K4[:, 1], K4[:, 2], K4[:, 3]
    pr["seed"] = np.asarray(seeds, np.uint32)
    return pr


class PnPsolver(Handle):
    """A handle for up to max_problems problems with max_correspondences correspondences in all and params.max_iterations <= max_iterations."""

    def __init__(self, max_problems=1024, max_correspondences=1 << 17, max_iterations=300):
        super().__init__(_bind(lib()), "oslam_pnp", max_problems, max_correspondences, max_iterations)

    def ransac_batch(self, problems, P3Dw, P2D, sigma2, params=None, samples=None, iter_inliers=False, Tcw=None, inliers=None, device=False):
        """problems: PROBLEM_DTYPE array (pack_problems); P3Dw [M, 3], P2D [M, 2], sigma2 [M] float32; samples None or int32 [n, max_iterations, 4].
        Returns dict(Tcw [n, 4, 4] float32, inliers [M] uint8, status [n, 4] int32 = kind, nInliers, iterations run, chosen iteration[, iter_inliers
        [n, max_iterations]]).  Tcw / inliers given by the caller are written in place: a problem without a pose keeps what they held.
        device=True goes through oslam_pnp_ransac_batch_device on a side stream, over torch tensors."""
        params = params or make_params()
        problems = np.ascontiguousarray(problems, PROBLEM_DTYPE)
        P3Dw = np.ascontiguousarray(P3Dw, np.float32).reshape(-1, 3)
        P2D = np.ascontiguousarray(P2D, np.float32).reshape(-1, 2)
        sigma2 = np.ascontiguousarray(sigma2, np.float32).reshape(-1)
        n, M, its = len(problems), len(sigma2), params.max_iterations
        assert len(P3Dw) == M and len(P2D) == M
        if samples is not None:
            samples = np.ascontiguousarray(samples, np.int32)
            assert samples.shape == (n, its, 4)
        Tcw = np.zeros((n, 4, 4), np.float32) if Tcw is None else Tcw
        inliers = np.zeros(M, np.uint8) if inliers is None else inliers
        assert Tcw.dtype == np.float32 and Tcw.size == 16 * n and Tcw.flags.c_contiguous and inliers.dtype == np.uint8 and inliers.size == M and inliers.flags.c_contiguous
        status = np.zeros((n, 4), np.int32)
        itc = np.full((n, its), -1, np.int32) if iter_inliers else None
        args = lambda a: (self.h, n, a(problems), M, a(P3Dw), a(P2D), a(sigma2), C.addressof(params), a(samples), a(Tcw), a(inliers), a(status), a(itc))
        if not device:
            check(self.L.oslam_pnp_ransac_batch(*args(optptr)))
        else:
            with device_call((problems, P3Dw, P2D, sigma2, samples, Tcw, inliers, status, itc), outputs=(Tcw, inliers, status, itc)) as (addr, stream):
                check(self.L.oslam_pnp_ransac_batch_device(*args(addr), stream))
        out = dict(Tcw=Tcw.reshape(n, 4, 4), inliers=inliers, status=status)
        if iter_inliers:
            out["iter_inliers"] = itc
        return out

    def epnp(self, counts, P3Dw, P2D, K4, offsets=None):
        """compute_pose (src/PnPsolver.cc:477-525) for sets of counts[s] >= 4 correspondences: (R [n, 3, 3], t [n, 3], err [n]) in float64."""
        counts = np.ascontiguousarray(counts, np.int32)
        n = len(counts)
        offsets = np.ascontiguousarray(np.concatenate([[0], np.cumsum(counts)[:-1]]) if offsets is None else offsets, np.int32)
        P3Dw = np.ascontiguousarray(P3Dw, np.float32).reshape(-1, 3)
        P2D = np.ascontiguousarray(P2D, np.float32).reshape(-1, 2)
        assert len(P3Dw) == len(P2D)
        K4 = np.ascontiguousarray(K4, np.float32)
        R, t, err = np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros(n)
        check(self.L.oslam_pnp_epnp(self.h, n, ptr(counts), ptr(offsets), len(P3Dw), ptr(P3Dw), ptr(P2D), ptr(K4), ptr(R), ptr(t), ptr(err)))
        return R, t, err


def ransac_batch(problems, P3Dw, P2D, sigma2, params=None, **kw):
    params = params or make_params()
    s = PnPsolver(max(1, len(problems)), max(1, len(np.asarray(sigma2).reshape(-1))), params.max_iterations)
    try:
        return s.ransac_batch(problems, P3Dw, P2D, sigma2, params, **kw)
    finally:
        s.close()


def epnp(counts, P3Dw, P2D, K4, offsets=None):
    s = PnPsolver(max(1, len(counts)), max(1, len(np.asarray(P3Dw).reshape(-1, 3))), 1)
    try:
        return s.epnp(counts, P3Dw, P2D, K4, offsets)
    finally:
        s.close()
