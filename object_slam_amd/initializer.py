"""ctypes view of the Initializer (include/oslam_hip.h, "Initializer"): ORB_SLAM2::Initializer::Initialize (src/Initializer.cc:44-121: homography and
fundamental-matrix RANSAC, model selection, ReconstructH / ReconstructF) for batches of independent problems, the numerical operator of
Tracking::MonocularInitialization (src/Tracking.cc:661, :695).

`draw` (the counter-based generator and the swap-with-back rule, eight draws) runs on the host.  `Initializer.initialize_batch` runs the gfx950 kernels
(no CPU fallback: creating an Initializer fails without a device); the module-level `initialize_batch` creates a handle of the right size for one call.
"""
import ctypes as C

import numpy as np

from ._lib import Handle, check, device_call, lib, optptr, ptr

REFERENCE_PARAMS = dict(max_iterations=200, min_parallax=1.0, min_triangulated=50)   # src/Tracking.cc:661, src/Initializer.cc:116-118
MODEL_NONE, MODEL_H, MODEL_F = 0, 1, 2


class Params(C.Structure):       # oslam_init_params_t
    _fields_ = [("max_iterations", C.c_int32), ("min_parallax", C.c_float), ("min_triangulated", C.c_int32), ("reserved", C.c_int32)]


class Problem(C.Structure):      # oslam_init_problem_t
    _fields_ = [("n1", C.c_int32), ("off1", C.c_int32), ("n2", C.c_int32), ("off2", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("sigma", C.c_float), ("seed", C.c_uint32), ("reserved", C.c_int32 * 2)]


PARAMS_DTYPE = np.dtype([("max_iterations", "<i4"), ("min_parallax", "<f4"), ("min_triangulated", "<i4"), ("reserved", "<i4")])
PROBLEM_DTYPE = np.dtype([("n1", "<i4"), ("off1", "<i4"), ("n2", "<i4"), ("off2", "<i4"), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("sigma", "<f4"),
                          ("seed", "<u4"), ("reserved", "<i4", (2,))])


def _bind(L):
    if getattr(L, "_oslam_init_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int
    L.oslam_init_draw.argtypes = [C.c_uint32, i32, i32, vp]
    L.oslam_init_create.argtypes = [C.POINTER(vp), i32, i32, i32]
    L.oslam_init_destroy.argtypes = [vp]
    L.oslam_init_destroy.restype = None
    L.oslam_init_initialize_batch.argtypes = [vp, i32, vp, i32, vp, vp, i32] + [vp] * 13
    L.oslam_init_initialize_batch_device.argtypes = [vp, i32, vp, i32, vp, vp, i32] + [vp] * 14
    L.oslam_init_set_timing.argtypes = [vp, i32]
    L.oslam_init_last_kernel_ms.argtypes = [vp, vp]
    L._oslam_init_bound = True
    return L


def make_params(**kw):
    p = dict(REFERENCE_PARAMS, **kw)
    return Params(p["max_iterations"], p["min_parallax"], p["min_triangulated"], 0)


def draw(seed, iteration, N):
    """The eight indices of the compacted match list iteration `iteration` of a problem with N matches draws from `seed`.  Host only."""
    out = np.zeros(8, np.int32)
    check(_bind(lib()).oslam_init_draw(int(seed) & 0xffffffff, int(iteration), int(N), ptr(out)))
    return out


def pack_problems(n1, n2, K4, sigma, seeds, off1=None, off2=None):
    """PROBLEM_DTYPE records; K4 = (fx, fy, cx, cy) and sigma, one for all problems or one per problem."""
    n1, n2 = np.asarray(n1, np.int32), np.asarray(n2, np.int32)
    n = len(n1)
    pr = np.zeros(n, PROBLEM_DTYPE)
    starts = lambda c: np.concatenate([[0], np.cumsum(c)[:-1]]) if n else 0
    pr["n1"], pr["n2"] = n1, n2
    pr["off1"] = starts(n1) if off1 is None else off1
    pr["off2"] = starts(n2) if off2 is None else off2
    K4 = np.broadcast_to(np.asarray(K4, np.float32), (n, 4))
    pr["fx"], pr["fy"], pr["cx"], pr["cy"] = K4[:, 0], K4[:, 1], K4[:, 2], K4[:, 3]
    pr["sigma"] = np.asarray(sigma, np.float32)
    pr["seed"] = np.asarray(seeds, np.uint32)
    return pr


class Initializer(Handle):
    """A handle for up to max_problems problems with max_keys keys per packed array and params.max_iterations <= max_iterations."""

    def __init__(self, max_problems=1024, max_keys=1 << 17, max_iterations=200):
        super().__init__(_bind(lib()), "oslam_init", max_problems, max_keys, max_iterations)

    def set_timing(self, on=True):
        check(self.L.oslam_init_set_timing(self.h, int(bool(on))))

    def last_kernel_ms(self):
        """(hypothesis kernel, reconstruction kernel) milliseconds of the last call, from the events set_timing switches on"""
        ms = np.zeros(2, np.float32)
        check(self.L.oslam_init_last_kernel_ms(self.h, ptr(ms)))
        return float(ms[0]), float(ms[1])

    def initialize_batch(self, problems, keys1, matches12, keys2, params=None, samples=None, dumps=False, R21=None, t21=None, P3D=None, triangulated=None, device=False):
        """problems: PROBLEM_DTYPE array (pack_problems); keys1 [M1, 2], keys2 [M2, 2] float32, matches12 [M1] int32; samples None or int32
        [n, max_iterations, 8].  Returns dict(R21 [n, 3, 3], t21 [n, 3], P3D [M1, 3] float32, triangulated [M1] uint8, status [n, 8] int32 = returned, model,
        N, nGood, motion, best H iteration, best F iteration, nsimilar / secondBestGood, scores [n, 4] float32 = SH, SF, RH, parallax[, with dumps=True:
        iter_scores [n, its, 2], hypotheses [n, its, 2, 3, 3] float32 (NaN where not run), iter_inliers [n, its, 2] int32 (-1 where not run), match_inliers
        [M1, 2] uint8]).  R21 / t21 / P3D / triangulated given by the caller are written in place: a problem that does not return keeps what they held.
        device=True goes through oslam_init_initialize_batch_device on a side stream, over torch tensors."""
        params = params or make_params()
        problems = np.ascontiguousarray(problems, PROBLEM_DTYPE)
        keys1 = np.ascontiguousarray(keys1, np.float32).reshape(-1, 2)
        keys2 = np.ascontiguousarray(keys2, np.float32).reshape(-1, 2)
        matches12 = np.ascontiguousarray(matches12, np.int32).reshape(-1)
        n, M1, M2, its = len(problems), len(keys1), len(keys2), params.max_iterations
        assert len(matches12) == M1
        if samples is not None:
            samples = np.ascontiguousarray(samples, np.int32)
            assert samples.shape == (n, its, 8)
        R21 = np.zeros((n, 3, 3), np.float32) if R21 is None else R21
        t21 = np.zeros((n, 3), np.float32) if t21 is None else t21
        P3D = np.zeros((M1, 3), np.float32) if P3D is None else P3D
        triangulated = np.zeros(M1, np.uint8) if triangulated is None else triangulated
        for a, dt, size in ((R21, np.float32, 9 * n), (t21, np.float32, 3 * n), (P3D, np.float32, 3 * M1), (triangulated, np.uint8, M1)):
            assert a.dtype == dt and a.size == size and a.flags.c_contiguous
        status = np.zeros((n, 8), np.int32)
        scores = np.zeros((n, 4), np.float32)
        # (what is not run: the NaN of all bits set, which is what the host entry point leaves there)
        isc = np.full((n, its, 2), -1, np.int32).view(np.float32) if dumps else None
        hyp = np.full((n, its, 2, 3, 3), -1, np.int32).view(np.float32) if dumps else None
        iin = np.full((n, its, 2), -1, np.int32) if dumps else None
        min_ = np.zeros((M1, 2), np.uint8) if dumps else None
        args = lambda a: (self.h, n, a(problems), M1, a(keys1), a(matches12), M2, a(keys2), C.addressof(params), a(samples), a(R21), a(t21), a(P3D), a(triangulated), a(status),
                          a(scores), a(isc), a(hyp), a(iin), a(min_))
        if not device:
            check(self.L.oslam_init_initialize_batch(*args(optptr)))
        else:
            with device_call((problems, keys1, matches12, keys2, samples, R21, t21, P3D, triangulated, status, scores, isc, hyp, iin, min_),
                             outputs=(R21, t21, P3D, triangulated, status, scores, isc, hyp, iin, min_)) as (addr, stream):
                check(self.L.oslam_init_initialize_batch_device(*args(addr), stream))
        out = dict(R21=R21.reshape(n, 3, 3), t21=t21.reshape(n, 3), P3D=P3D.reshape(M1, 3), triangulated=triangulated, status=status, scores=scores)
        if dumps:
            out.update(iter_scores=isc, hypotheses=hyp, iter_inliers=iin, match_inliers=min_)
        return out


def initialize_batch(problems, keys1, matches12, keys2, params=None, **kw):
    params = params or make_params()
    s = Initializer(max(1, len(problems)), max(1, len(np.asarray(keys1).reshape(-1, 2)), len(np.asarray(keys2).reshape(-1, 2))), params.max_iterations)
    try:
        return s.initialize_batch(problems, keys1, matches12, keys2, params, **kw)
    finally:
        s.close()
