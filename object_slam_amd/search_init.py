"""ctypes view of the initialisation search (include/oslam_hip.h, "Initialisation search"): ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched,
vnMatches12, windowSize) (src/ORBmatcher.cc:405-520), which Tracking::MonocularInitialization runs with ORBmatcher(0.9, true) and windowSize = 100
(src/Tracking.cc:680-681), for batches of independent problems: one per sequence that is still initialising.

`InitMatcher.search_batch` is one launch of the gfx950 kernel over all problems (no CPU fallback: creating an InitMatcher fails without a device).  Frames
are rows of two flat arrays; `pack_problems` builds the records that name them.  matches12 has the layout `initializer.Initializer.initialize_batch` takes.
An operator: the driver does not call it.
"""
import ctypes as C

import numpy as np

from ._lib import KP_DTYPE, Handle, check, device_call, lib, optptr, ptr
from ._proj_common import _consecutive, _pack

MAX_KEYPOINTS = 2400
NNRATIO, WINDOW_SIZE = 0.9, 100   # src/Tracking.cc:680-681


class Problem(C.Structure):    # oslam_init_match_problem_t
    _fields_ = [("n1", C.c_int32), ("off1", C.c_int32), ("n2", C.c_int32), ("off2", C.c_int32), ("windowSize", C.c_int32), ("reserved", C.c_int32)]


class F1Rows(C.Structure):     # oslam_init_match_f1_rows_t
    _fields_ = [("n_rows", C.c_int32), ("keysUn", C.c_void_p), ("desc", C.c_void_p)]


class F2Rows(C.Structure):     # oslam_init_match_f2_rows_t
    _fields_ = [("n_rows", C.c_int32), ("keysUn", C.c_void_p), ("desc", C.c_void_p)]


PROBLEM_DTYPE = np.dtype([("n1", "<i4"), ("off1", "<i4"), ("n2", "<i4"), ("off2", "<i4"), ("windowSize", "<i4"), ("reserved", "<i4")])
ROW_KEYS = ("keysUn", "desc")
_ROW_TYPES = dict(keysUn=(KP_DTYPE, ()), desc=(np.uint8, (32,)))


def _bind(L):
    if getattr(L, "_oslam_init_match_bound", False):
        return L
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    L.oslam_init_match_create.argtypes = [C.POINTER(vp), i32, i32, i32, i32]
    L.oslam_init_match_destroy.argtypes = [vp]
    L.oslam_init_match_destroy.restype = None
    L.oslam_match_search_for_initialization_batch.argtypes = [vp, i32, vp, vp, vp, vp, f32, i32] + [vp] * 6
    L.oslam_match_search_for_initialization_batch_device.argtypes = [vp, i32, vp, vp, vp, vp, f32, i32] + [vp] * 7
    L.oslam_init_match_last_phase_ticks.argtypes = [vp, vp]
    L._oslam_init_match_bound = True
    return L


def pack_problems(n1, n2, window_size=WINDOW_SIZE, off1=None, off2=None):
    """PROBLEM_DTYPE records.  off1 / off2 default to consecutive rows, n1 / n2 per problem in the order given."""
    n1, n2 = np.asarray(n1, np.int32).reshape(-1), np.asarray(n2, np.int32).reshape(-1)
    pr = np.zeros(len(n1), PROBLEM_DTYPE)
    pr["n1"], pr["n2"], pr["windowSize"] = n1, n2, np.asarray(window_size, np.int32)
    pr["off1"] = _consecutive(n1) if off1 is None else np.asarray(off1, np.int32)
    pr["off2"] = _consecutive(n2) if off2 is None else np.asarray(off2, np.int32)
    return pr


def pack_rows(rows):
    """The two per-key arrays of `rows` (a dict with ROW_KEYS) as contiguous arrays of the ABI's types."""
    return _pack(rows, ROW_KEYS, _ROW_TYPES, "key")


class InitMatcher(Handle):
    """A handle for up to max_problems problems whose F2 has up to max_keypoints <= 2400 keys; max_keys1_total bounds the frames-1 rows of one call."""

    def __init__(self, max_problems=1024, max_keypoints=MAX_KEYPOINTS, max_keys1_total=1 << 20, device=0):
        super().__init__(_bind(lib()), "oslam_init_match", max_problems, max_keypoints, max_keys1_total, device)

    def last_phase_ticks(self):
        """shader-clock ticks of workgroup 0 of the last call: (staging, candidate search, sequential replay, histogram and outputs)"""
        t = np.zeros(4, np.int64)
        check(self.L.oslam_init_match_last_phase_ticks(self.h, ptr(t)))
        return tuple(int(v) for v in t)

    def search_batch(self, problems, frames1, frames2, bounds, prev_matched, nnratio=NNRATIO, check_orientation=True, matches12=None, n_matches=None, n_removed=None,
                     n_displaced=None, n_overflow=None, device=False):
        """SearchForInitialization of every problem.  problems: PROBLEM_DTYPE array (pack_problems); frames1 / frames2: dicts of the per-key arrays (ROW_KEYS);
        bounds = (mnMinX, mnMinY, mnMaxX, mnMaxY); prev_matched: float32 [n_rows1, 2], vbPrevMatched, written in place for the surviving matches.  Returns
        dict(prev_matched, matches12 [n_rows1] int32, n_matches, n_removed, n_displaced, n_overflow [n_problems] int32); arrays given by the caller are written
        in place (rows the call does not write keep what they held).  device=True goes through the _device entry point on a side stream, over torch tensors."""
        problems, frames1, frames2 = np.ascontiguousarray(problems, PROBLEM_DTYPE), pack_rows(frames1), pack_rows(frames2)
        n, M1 = len(problems), len(frames1["desc"])
        assert prev_matched.dtype == np.float32 and prev_matched.size == 2 * M1 and prev_matched.flags.c_contiguous
        matches12 = np.full(M1, -1, np.int32) if matches12 is None else matches12
        counts = [np.zeros(n, np.int32) if o is None else o for o in (n_matches, n_removed, n_displaced, n_overflow)]
        outs = [prev_matched, matches12] + counts
        for o, size in zip(outs[1:], [M1, n, n, n, n]):
            assert o.dtype == np.int32 and o.size == size and o.flags.c_contiguous
        bnd = np.ascontiguousarray(bounds, np.float32).reshape(4)

        def args(a):
            r1 = F1Rows(M1, *[a(frames1[k]) for k in ROW_KEYS])   # (byref keeps the structs alive until the call has returned)
            r2 = F2Rows(len(frames2["desc"]), *[a(frames2[k]) for k in ROW_KEYS])
            return (self.h, n, a(problems), C.byref(r1), C.byref(r2), ptr(bnd), float(nnratio), int(bool(check_orientation))) + tuple(a(o) for o in outs)
        if not device:
            check(self.L.oslam_match_search_for_initialization_batch(*args(optptr)))
        else:
            with device_call([problems] + outs + [frames1[k] for k in ROW_KEYS] + [frames2[k] for k in ROW_KEYS], outputs=tuple(outs)) as (addr, stream):
                check(self.L.oslam_match_search_for_initialization_batch_device(*args(addr), stream))
        return dict(prev_matched=prev_matched, matches12=matches12, n_matches=counts[0], n_removed=counts[1], n_displaced=counts[2], n_overflow=counts[3])
