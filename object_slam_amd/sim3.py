"""ctypes view of the Sim3 solver (include/oslam_hip.h, "Sim3 solver"): ORB_SLAM2::Sim3Solver (src/Sim3Solver.cc, Horn's closed form inside RANSAC)
for batches of independent problems, the numerical operator of LoopClosing::ComputeSim3 (src/LoopClosing.cc:232-343).

`ransac_params` (SetRansacParameters) and `draw` (the counter-based generator and the swap-with-back rule) run on the host.
`Sim3Solver.iterate_batch` is iterate(n_iterations) of every problem on the gfx950 kernels (no CPU fallback: creating a Sim3Solver fails without a
device); the state records it takes and returns make later calls resume.  The module-level `iterate_batch` creates a solver of the right size for one call.
"""
import ctypes as C

import numpy as np

from ._lib import Handle, check, device_call, lib, optptr, ptr

REFERENCE_PARAMS = dict(probability=0.99, min_inliers=20, max_iterations=300)   # src/LoopClosing.cc:276


class Params(C.Structure):       # oslam_sim3_params_t
    _fields_ = [("probability", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32)]


class Problem(C.Structure):      # oslam_sim3_problem_t
    _fields_ = [("count", C.c_int32), ("offset", C.c_int32), ("fx1", C.c_float), ("fy1", C.c_float), ("cx1", C.c_float), ("cy1", C.c_float), ("fx2", C.c_float),
                ("fy2", C.c_float), ("cx2", C.c_float), ("cy2", C.c_float), ("seed", C.c_uint32), ("fix_scale", C.c_int32)]


class State(C.Structure):        # oslam_sim3_state_t
    _fields_ = [("iterations_done", C.c_int32), ("best_inliers", C.c_int32), ("best_iteration", C.c_int32), ("R", C.c_float * 9), ("t", C.c_float * 3), ("s", C.c_float)]


class Ransac(C.Structure):       # oslam_sim3_ransac_t
    _fields_ = [("iterations", C.c_int32), ("no_more", C.c_int32)]


PROBLEM_DTYPE = np.dtype([("count", "<i4"), ("offset", "<i4"), ("fx1", "<f4"), ("fy1", "<f4"), ("cx1", "<f4"), ("cy1", "<f4"), ("fx2", "<f4"), ("fy2", "<f4"),
                          ("cx2", "<f4"), ("cy2", "<f4"), ("seed", "<u4"), ("fix_scale", "<i4")])
STATE_DTYPE = np.dtype([("iterations_done", "<i4"), ("best_inliers", "<i4"), ("best_iteration", "<i4"), ("R", "<f4", (3, 3)), ("t", "<f4", (3,)), ("s", "<f4")])


def _bind(L):
    if getattr(L, "_oslam_sim3_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int
    L.oslam_sim3_ransac_params.argtypes = [i32, C.c_double, i32, i32, vp]
    L.oslam_sim3_draw.argtypes = [C.c_uint32, i32, i32, vp]
    L.oslam_sim3_create.argtypes = [C.POINTER(vp), i32, i32, i32]
    L.oslam_sim3_destroy.argtypes = [vp]
    L.oslam_sim3_destroy.restype = None
    L.oslam_sim3_iterate_batch.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.oslam_sim3_iterate_batch_device.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L._oslam_sim3_bound = True
    return L


def make_params(**kw):
    p = dict(REFERENCE_PARAMS, **kw)
    return Params(p["probability"], p["min_inliers"], p["max_iterations"])


def ransac_params(N, probability=0.99, min_inliers=20, max_iterations=300):
    """SetRansacParameters (src/Sim3Solver.cc:114-138): dict(iterations, no_more) for N correspondences.  Host only."""
    out = Ransac()
    check(_bind(lib()).oslam_sim3_ransac_params(int(N), probability, min_inliers, max_iterations, C.addressof(out)))
    return dict(iterations=out.iterations, no_more=bool(out.no_more))


def draw(seed, iteration, N):
    """The three correspondence indices iteration `iteration` of a problem with N correspondences draws from `seed`.  Host only."""
    out = np.zeros(3, np.int32)
    check(_bind(lib()).oslam_sim3_draw(int(seed) & 0xffffffff, int(iteration), int(N), ptr(out)))
    return out


def pack_problems(counts, K1, K2, seeds, fix_scale, offsets=None):
    """PROBLEM_DTYPE records; K1, K2 = (fx, fy, cx, cy) of the two cameras, one for all problems or one per problem."""
    counts = np.asarray(counts, np.int32)
    n = len(counts)
    pr = np.zeros(n, PROBLEM_DTYPE)
    pr["count"] = counts
    pr["offset"] = np.concatenate([[0], np.cumsum(counts)[:-1]]) if offsets is None and n else (offsets if n else 0)
    K1 = np.broadcast_to(np.asarray(K1, np.float32), (n, 4))
    K2 = np.broadcast_to(np.asarray(K2, np.float32), (n, 4))
    pr["fx1"], pr["fy1"], pr["cx1"], pr["cy1"] = K1[:, 0], K1[:, 1], K1[:, 2], K1[:, 3]
    pr["fx2"], pr["fy2"], pr["cx2"], pr["cy2"] = K2[:, 0], K2[:, 1], K2[:, 2], K2[:, 3]
    pr["seed"] = np.asarray(seeds, np.uint32)
    pr["fix_scale"] = np.asarray(fix_scale, np.int32)
    return pr


def fresh_states(n):
    """n state records of solvers that have not iterated yet."""
    st = np.zeros(n, STATE_DTYPE)
    st["best_iteration"] = -1
    return st


class Sim3Solver(Handle):
    """A handle for up to max_problems problems with max_correspondences correspondences in all and params.max_iterations <= max_iterations."""

    def __init__(self, max_problems=1024, max_correspondences=1 << 17, max_iterations=300):
        super().__init__(_bind(lib()), "oslam_sim3", max_problems, max_correspondences, max_iterations)

    def iterate_batch(self, problems, states, X3Dc1, X3Dc2, sigma2_1, sigma2_2, n_iterations, params=None, samples=None, iter_inliers=False, hypotheses=False, T12=None,
                      inliers=None, device=False):
        """iterate(n_iterations) of every problem.  problems: PROBLEM_DTYPE array (pack_problems); states: STATE_DTYPE array (fresh_states), updated IN PLACE;
        X3Dc1, X3Dc2 [M, 3], sigma2_1, sigma2_2 [M] float32; samples None or int32 [n, max_iterations, 3].  Returns dict(T12 [n, 4, 4] float32, inliers [M]
        uint8, status [n, 4] int32 = returned, nInliers, iterations run, no_more, states[, iter_inliers [n, max_iterations] int32, -1 where not run in this
        call][, hypotheses [n, max_iterations, 13] float32, NaN where not run]).  T12 / inliers given by the caller are written in place: a problem without a
        Sim3 keeps what they held.  device=True goes through oslam_sim3_iterate_batch_device on a side stream, over torch tensors."""
        params = params or make_params()
        problems = np.ascontiguousarray(problems, PROBLEM_DTYPE)
        assert states.dtype == STATE_DTYPE and states.flags.c_contiguous and len(states) == len(problems)
        X3Dc1 = np.ascontiguousarray(X3Dc1, np.float32).reshape(-1, 3)
        X3Dc2 = np.ascontiguousarray(X3Dc2, np.float32).reshape(-1, 3)
        sigma2_1 = np.ascontiguousarray(sigma2_1, np.float32).reshape(-1)
        sigma2_2 = np.ascontiguousarray(sigma2_2, np.float32).reshape(-1)
        n, M, its = len(problems), len(sigma2_1), params.max_iterations
        assert len(X3Dc1) == M and len(X3Dc2) == M and len(sigma2_2) == M
        if samples is not None:
            samples = np.ascontiguousarray(samples, np.int32)
            assert samples.shape == (n, its, 3)
        T12 = np.zeros((n, 4, 4), np.float32) if T12 is None else T12
        inliers = np.zeros(M, np.uint8) if inliers is None else inliers
        assert T12.dtype == np.float32 and T12.size == 16 * n and T12.flags.c_contiguous and inliers.dtype == np.uint8 and inliers.size == M and inliers.flags.c_contiguous
        status = np.zeros((n, 4), np.int32)
        itc = np.full((n, its), -1, np.int32) if iter_inliers else None
        hyp = np.full((n, its, 13), np.nan, np.float32) if hypotheses else None
        args = lambda a: (self.h, n, a(problems), a(states), M, a(X3Dc1), a(X3Dc2), a(sigma2_1), a(sigma2_2), C.addressof(params), int(n_iterations), a(samples), a(T12),
                          a(inliers), a(status), a(itc), a(hyp))
        if not device:
            check(self.L.oslam_sim3_iterate_batch(*args(optptr)))
        else:
            with device_call((problems, states, X3Dc1, X3Dc2, sigma2_1, sigma2_2, samples, T12, inliers, status, itc, hyp),
                             outputs=(T12, inliers, status, states, itc, hyp)) as (addr, stream):
                check(self.L.oslam_sim3_iterate_batch_device(*args(addr), stream))
        out = dict(T12=T12.reshape(n, 4, 4), inliers=inliers, status=status, states=states)
        if iter_inliers:
            out["iter_inliers"] = itc
        if hypotheses:
            out["hypotheses"] = hyp
        return out


def iterate_batch(problems, states, X3Dc1, X3Dc2, sigma2_1, sigma2_2, n_iterations, params=None, **kw):
    params = params or make_params()
    s = Sim3Solver(max(1, len(problems)), max(1, len(np.asarray(sigma2_1).reshape(-1))), params.max_iterations)
    try:
        return s.iterate_batch(problems, states, X3Dc1, X3Dc2, sigma2_1, sigma2_2, n_iterations, params, **kw)
    finally:
        s.close()
