"""ctypes view of OptimizeSim3 (include/oslam_hip.h, "OptimizeSim3"): Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241) for batches of independent
problems, the optimisation LoopClosing::ComputeSim3 runs on the matches SearchBySim3 has completed (src/LoopClosing.cc:327, th2 = 10).

`Sim3Optimizer.optimize_batch` is one launch of the gfx950 kernel over all problems (no CPU fallback: creating a Sim3Optimizer fails without a device).
A problem is a run of rows of the packed per-correspondence arrays; `pack_problems` builds the records that name them.
"""
import ctypes as C

import numpy as np

from ._lib import Handle, check, device_call, lib, optptr

REFERENCE_TH2 = 10.0   # src/LoopClosing.cc:327
TRACE_ROWS = 150       # OSLAM_SIM3_OPT_TRACE_ROWS


class Problem(C.Structure):      # oslam_sim3_opt_problem_t
    _fields_ = [("count", C.c_int32), ("offset", C.c_int32), ("fx1", C.c_float), ("fy1", C.c_float), ("cx1", C.c_float), ("cy1", C.c_float), ("fx2", C.c_float),
                ("fy2", C.c_float), ("cx2", C.c_float), ("cy2", C.c_float), ("s12", C.c_float), ("R12", C.c_float * 9), ("t12", C.c_float * 3), ("th2", C.c_float),
                ("fix_scale", C.c_int32)]


PROBLEM_DTYPE = np.dtype([("count", "<i4"), ("offset", "<i4"), ("fx1", "<f4"), ("fy1", "<f4"), ("cx1", "<f4"), ("cy1", "<f4"), ("fx2", "<f4"), ("fy2", "<f4"),
                          ("cx2", "<f4"), ("cy2", "<f4"), ("s12", "<f4"), ("R12", "<f4", (3, 3)), ("t12", "<f4", (3,)), ("th2", "<f4"), ("fix_scale", "<i4")])


def _bind(L):
    if getattr(L, "_oslam_sim3_opt_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int
    L.oslam_sim3_opt_create.argtypes = [C.POINTER(vp), i32, i32, i32]
    L.oslam_sim3_opt_destroy.argtypes = [vp]
    L.oslam_sim3_opt_destroy.restype = None
    L.oslam_optimize_sim3_batch.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.oslam_optimize_sim3_batch_device.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L._oslam_sim3_opt_bound = True
    return L


def pack_problems(counts, K1, K2, s12, R12, t12, fix_scale, th2=REFERENCE_TH2, offsets=None):
    """PROBLEM_DTYPE records; K1, K2 = (fx, fy, cx, cy) of the two cameras, one for all problems or one per problem (so s12, R12, t12, fix_scale, th2).  offsets defaults to consecutive rows."""
    counts = np.asarray(counts, np.int32).reshape(-1)
    n = len(counts)
    pr = np.zeros(n, PROBLEM_DTYPE)
    pr["count"] = counts
    pr["offset"] = (np.concatenate([[0], np.cumsum(np.maximum(counts, 0))[:-1]]) if n else 0) if offsets is None else np.asarray(offsets, np.int32)
    K1 = np.broadcast_to(np.asarray(K1, np.float32), (n, 4))
    K2 = np.broadcast_to(np.asarray(K2, np.float32), (n, 4))
    pr["fx1"], pr["fy1"], pr["cx1"], pr["cy1"] = K1[:, 0], K1[:, 1], K1[:, 2], K1[:, 3]
    pr["fx2"], pr["fy2"], pr["cx2"], pr["cy2"] = K2[:, 0], K2[:, 1], K2[:, 2], K2[:, 3]
    pr["s12"] = np.asarray(s12, np.float32)
    pr["R12"] = np.broadcast_to(np.asarray(R12, np.float32), (n, 3, 3))
    pr["t12"] = np.broadcast_to(np.asarray(t12, np.float32), (n, 3))
    pr["th2"] = np.asarray(th2, np.float32)
    pr["fix_scale"] = np.asarray(fix_scale, np.int32)
    return pr


class Sim3Optimizer(Handle):
    """A handle for up to max_problems problems with max_correspondences correspondences in all."""

    def __init__(self, max_problems=1024, max_correspondences=1 << 17, device=0):
        super().__init__(_bind(lib()), "oslam_sim3_opt", max_problems, max_correspondences, device)

    def optimize_batch(self, problems, X3Dc1, X3Dc2, obs1, obs2, invSigma2_1, invSigma2_2, S12=None, inliers=None, status=None, trace=False, device=False):
        """OptimizeSim3 of every problem.  problems: PROBLEM_DTYPE array (pack_problems); X3Dc1, X3Dc2 [M, 3], obs1, obs2 [M, 2], invSigma2_1, invSigma2_2 [M]
        float32.  Returns dict(S12 [n, 13] float64 = R row-major, t, s; inliers [M] uint8; status [n, 4] int32 = returned (or -1, -2), nCorrespondences, nBad
        of the first pass, 256 * LM iterations + LM trials[, trace [n, 150, 6] float64 = F before, F of the trial, rho, lambda, accepted, first trial of an
        optimize call; trace_n [n] int32]).  S12 / inliers / status given by the caller are written in place: what the call does not write keeps what it held.
        device=True goes through oslam_optimize_sim3_batch_device on a side stream, over torch tensors."""
        problems = np.ascontiguousarray(problems, PROBLEM_DTYPE)
        f32 = lambda a, w: np.ascontiguousarray(a, np.float32).reshape((-1, w) if w else (-1,))
        X3Dc1, X3Dc2, obs1, obs2, invSigma2_1, invSigma2_2 = f32(X3Dc1, 3), f32(X3Dc2, 3), f32(obs1, 2), f32(obs2, 2), f32(invSigma2_1, 0), f32(invSigma2_2, 0)
        n, M = len(problems), len(invSigma2_1)
        assert len(X3Dc1) == M and len(X3Dc2) == M and len(obs1) == M and len(obs2) == M and len(invSigma2_2) == M
        S12 = np.zeros((n, 13), np.float64) if S12 is None else S12
        inliers = np.zeros(M, np.uint8) if inliers is None else inliers
        status = np.zeros((n, 4), np.int32) if status is None else status
        assert S12.dtype == np.float64 and S12.size == 13 * n and S12.flags.c_contiguous and inliers.dtype == np.uint8 and inliers.size == M and inliers.flags.c_contiguous
        assert status.dtype == np.int32 and status.size == 4 * n and status.flags.c_contiguous
        tr = np.zeros((n, TRACE_ROWS, 6), np.float64) if trace else None
        tn = np.zeros(n, np.int32) if trace else None
        args = lambda a: (self.h, n, a(problems), M, a(X3Dc1), a(X3Dc2), a(obs1), a(obs2), a(invSigma2_1), a(invSigma2_2), a(S12), a(inliers), a(status), a(tr), a(tn))
        if not device:
            check(self.L.oslam_optimize_sim3_batch(*args(optptr)))
        else:
            with device_call((problems, X3Dc1, X3Dc2, obs1, obs2, invSigma2_1, invSigma2_2, S12, inliers, status, tr, tn), outputs=(S12, inliers, status, tr, tn)) as (addr, stream):
                check(self.L.oslam_optimize_sim3_batch_device(*args(addr), stream))
        out = dict(S12=S12.reshape(n, 13), inliers=inliers, status=status.reshape(n, 4))
        if trace:
            out["trace"], out["trace_n"] = tr, tn
        return out


def optimize_batch(problems, X3Dc1, X3Dc2, obs1, obs2, invSigma2_1, invSigma2_2, **kw):
    s = Sim3Optimizer(max(1, len(problems)), max(1, len(np.asarray(invSigma2_1).reshape(-1))))
    try:
        return s.optimize_batch(problems, X3Dc1, X3Dc2, obs1, obs2, invSigma2_1, invSigma2_2, **kw)
    finally:
        s.close()
