"""ctypes view of SearchBySim3 (include/oslam_hip.h, "SearchBySim3"): ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1102-1326) for batches of independent
keyframe pairs, the matching step LoopClosing::ComputeSim3 runs on every Sim3 a solver returns (src/LoopClosing.cc:324, th = 7.5).

`Sim3Matcher.search_batch` is one launch of the gfx950 kernel over all pairs (no CPU fallback: creating a Sim3Matcher fails without a device).  Keyframes
are rows of flat per-keypoint arrays; `pack_pairs` builds the pair records that name them.
"""
import ctypes as C

import numpy as np

from ._lib import KP_DTYPE, Handle, check, device_call, lib, optptr, ptr
from ._proj_common import _camera_args, _consecutive, _pack, _rows_of

MAX_KEYPOINTS = 2400
REFERENCE_TH = 7.5   # src/LoopClosing.cc:324


class Pair(C.Structure):       # oslam_sim3_pair_t
    _fields_ = [("n1", C.c_int32), ("off1", C.c_int32), ("n2", C.c_int32), ("off2", C.c_int32), ("out_off", C.c_int32), ("s12", C.c_float), ("R12", C.c_float * 9),
                ("t12", C.c_float * 3), ("T1w", C.c_float * 16), ("T2w", C.c_float * 16), ("th", C.c_float)]


class Rows(C.Structure):       # oslam_sim3_match_rows_t
    _fields_ = [("n_rows", C.c_int32), ("keysUn", C.c_void_p), ("desc", C.c_void_p), ("has_mp", C.c_void_p), ("Xw", C.c_void_p), ("mp_desc", C.c_void_p),
                ("maxDistance", C.c_void_p), ("minDistance", C.c_void_p)]


PAIR_DTYPE = np.dtype([("n1", "<i4"), ("off1", "<i4"), ("n2", "<i4"), ("off2", "<i4"), ("out_off", "<i4"), ("s12", "<f4"), ("R12", "<f4", (3, 3)), ("t12", "<f4", (3,)),
                       ("T1w", "<f4", (4, 4)), ("T2w", "<f4", (4, 4)), ("th", "<f4")])
ROW_KEYS = ("keysUn", "desc", "has_mp", "Xw", "mp_desc", "maxDistance", "minDistance")
_ROW_TYPES = dict(keysUn=(KP_DTYPE, ()), desc=(np.uint8, (32,)), has_mp=(np.uint8, ()), Xw=(np.float32, (3,)), mp_desc=(np.uint8, (32,)), maxDistance=(np.float32, ()),
                  minDistance=(np.float32, ()))


def _bind(L):
    if getattr(L, "_oslam_sim3_match_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int
    L.oslam_sim3_match_create.argtypes = [C.POINTER(vp), i32, i32, i32]
    L.oslam_sim3_match_destroy.argtypes = [vp]
    L.oslam_sim3_match_destroy.restype = None
    L.oslam_match_search_by_sim3_batch.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp, i32, C.c_float, vp, vp]
    L.oslam_match_search_by_sim3_batch_device.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp, i32, C.c_float, vp, vp, vp]
    L._oslam_sim3_match_bound = True
    return L


def pack_pairs(n1, off1, n2, off2, s12, R12, t12, T1w, T2w, th=REFERENCE_TH, out_off=None):
    """PAIR_DTYPE records.  out_off defaults to consecutive output rows, n1 per pair in the order given."""
    n1 = np.asarray(n1, np.int32).reshape(-1)
    n = len(n1)
    pr = np.zeros(n, PAIR_DTYPE)
    pr["n1"], pr["off1"], pr["n2"], pr["off2"] = n1, np.asarray(off1, np.int32), np.asarray(n2, np.int32), np.asarray(off2, np.int32)
    pr["out_off"] = _consecutive(n1) if out_off is None else np.asarray(out_off, np.int32)
    pr["s12"] = np.asarray(s12, np.float32)
    pr["R12"] = np.asarray(R12, np.float32).reshape(n, 3, 3)
    pr["t12"] = np.asarray(t12, np.float32).reshape(n, 3)
    pr["T1w"] = np.asarray(T1w, np.float32).reshape(n, 4, 4)
    pr["T2w"] = np.asarray(T2w, np.float32).reshape(n, 4, 4)
    pr["th"] = np.asarray(th, np.float32)
    return pr


def pack_rows(rows):
    """The seven per-keypoint arrays of `rows` (a dict with ROW_KEYS) as contiguous arrays of the ABI's types."""
    return _pack(rows, ROW_KEYS, _ROW_TYPES, "keypoint")


class Sim3Matcher(Handle):
    """A handle for up to max_pairs pairs of keyframes with up to max_keypoints (<= 2400) keypoints each."""

    def __init__(self, max_pairs=1024, max_keypoints=MAX_KEYPOINTS, device=0):
        super().__init__(_bind(lib()), "oslam_sim3_match", max_pairs, max_keypoints, device)

    def search_batch(self, pairs, rows, cam, bounds, scale_factors, log_scale_factor, matched_in=None, match12=None, n_found=None, n_out=None, device=False):
        """SearchBySim3 of every pair.  pairs: PAIR_DTYPE array (pack_pairs); rows: dict of the per-keypoint arrays (ROW_KEYS); cam = (fx, fy, cx, cy);
        bounds = (mnMinX, mnMinY, mnMaxX, mnMaxY); matched_in None or int32 [n_out].  Returns dict(match12 [n_out] int32, n_found [n_pairs] int32); match12 /
        n_found given by the caller are written in place (rows the call does not write keep what they held).  device=True goes through
        oslam_match_search_by_sim3_batch_device on a side stream, over torch tensors."""
        pairs = np.ascontiguousarray(pairs, PAIR_DTYPE)
        rows = pack_rows(rows)
        n, n_rows = len(pairs), len(rows["has_mp"])
        if n_out is None:
            n_out = len(match12) if match12 is not None else len(matched_in) if matched_in is not None else _rows_of(pairs, "n1", "out_off")
        if matched_in is not None:
            matched_in = np.ascontiguousarray(matched_in, np.int32)
            assert matched_in.size == n_out
        match12 = np.full(n_out, -1, np.int32) if match12 is None else match12
        n_found = np.zeros(n, np.int32) if n_found is None else n_found
        assert match12.dtype == np.int32 and match12.size == n_out and match12.flags.c_contiguous and n_found.dtype == np.int32 and n_found.size == n and n_found.flags.c_contiguous
        camera, bnd, sf = _camera_args(cam, bounds, scale_factors)
        def args(a):
            r = Rows(n_rows, *[a(rows[k]) for k in ROW_KEYS])   # (byref keeps r alive until the call has returned)
            return (self.h, n, a(pairs), C.byref(r), n_out, a(matched_in), C.addressof(camera), ptr(bnd), ptr(sf), len(sf), float(log_scale_factor), a(match12), a(n_found))
        if not device:
            check(self.L.oslam_match_search_by_sim3_batch(*args(optptr)))
        else:
            with device_call([pairs, matched_in, match12, n_found] + [rows[k] for k in ROW_KEYS], outputs=(match12, n_found)) as (addr, stream):
                check(self.L.oslam_match_search_by_sim3_batch_device(*args(addr), stream))
        return dict(match12=match12, n_found=n_found)
