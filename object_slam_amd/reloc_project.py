"""ctypes view of the relocalisation projection operator (include/oslam_hip.h, "Relocalisation projection"): ORBmatcher::SearchByProjection(CurrentFrame, pKF,
sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1472-1599), which Tracking::Relocalization runs twice per candidate keyframe whose optimised pose has 10 to 49
inliers (src/Tracking.cc:1717 with (10, 100), :1731 with (3, 64)), for batches of independent problems: one per (lost frame, candidate keyframe).

`RelocProjector.search_batch` is one launch of the gfx950 kernel over all problems (no CPU fallback: creating a RelocProjector fails without a device).
Frames and keyframe map-point slots are rows of flat arrays; `pack_problems` builds the records that name them.  An operator: the driver does not relocalise.
"""
import ctypes as C

import numpy as np

from ._lib import KP_DTYPE, Handle, check, device_call, lib, optptr, ptr
from ._proj_common import _camera_args, _pack, _problem_head, _rows_of

MAX_KEYPOINTS = 2400
COARSE, FINE = (10.0, 100), (3.0, 64)   # (th, ORBdist) of src/Tracking.cc:1717 and :1731


class Problem(C.Structure):    # oslam_reloc_proj_problem_t
    _fields_ = [("n_kp", C.c_int32), ("kp_off", C.c_int32), ("n_pts", C.c_int32), ("pt_off", C.c_int32), ("kp_out_off", C.c_int32), ("pt_out_off", C.c_int32),
                ("Tcw", C.c_float * 16), ("th", C.c_float), ("ORBdist", C.c_int32)]


class FrameRows(C.Structure):  # oslam_reloc_proj_frame_rows_t
    _fields_ = [("n_rows", C.c_int32), ("keysUn", C.c_void_p), ("desc", C.c_void_p), ("has_mp", C.c_void_p)]


class PtRows(C.Structure):     # oslam_reloc_proj_pt_rows_t
    _fields_ = [("n_rows", C.c_int32), ("Xw", C.c_void_p), ("desc", C.c_void_p), ("maxDistance", C.c_void_p), ("minDistance", C.c_void_p), ("kf_angle", C.c_void_p)]


PROBLEM_DTYPE = np.dtype([("n_kp", "<i4"), ("kp_off", "<i4"), ("n_pts", "<i4"), ("pt_off", "<i4"), ("kp_out_off", "<i4"), ("pt_out_off", "<i4"), ("Tcw", "<f4", (4, 4)),
                          ("th", "<f4"), ("ORBdist", "<i4")])
FRAME_KEYS = ("keysUn", "desc", "has_mp")
PT_KEYS = ("Xw", "desc", "maxDistance", "minDistance", "kf_angle")
_FRAME_TYPES = dict(keysUn=(KP_DTYPE, ()), desc=(np.uint8, (32,)), has_mp=(np.uint8, ()))
_PT_TYPES = dict(Xw=(np.float32, (3,)), desc=(np.uint8, (32,)), maxDistance=(np.float32, ()), minDistance=(np.float32, ()), kf_angle=(np.float32, ()))


def _bind(L):
    if getattr(L, "_oslam_reloc_proj_bound", False):
        return L
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    L.oslam_reloc_proj_create.argtypes = [C.POINTER(vp), i32, i32, i32, i32]
    L.oslam_reloc_proj_destroy.argtypes = [vp]
    L.oslam_reloc_proj_destroy.restype = None
    L.oslam_match_search_by_projection_reloc_batch.argtypes = [vp, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, i32, f32, i32, vp, vp, vp, vp]
    L.oslam_match_search_by_projection_reloc_batch_device.argtypes = [vp, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, i32, f32, i32, vp, vp, vp, vp, vp]
    L._oslam_reloc_proj_bound = True
    return L


def pack_problems(n_kp, kp_off, n_pts, pt_off, Tcw, th, orb_dist, kp_out_off=None, pt_out_off=None):
    """PROBLEM_DTYPE records.  kp_out_off / pt_out_off default to consecutive output rows, n_kp / n_pts per problem in the order given."""
    pr = _problem_head(PROBLEM_DTYPE, n_kp, kp_off, n_pts, pt_off, kp_out_off, pt_out_off)
    pr["Tcw"] = np.asarray(Tcw, np.float32).reshape(len(pr), 4, 4)
    pr["th"], pr["ORBdist"] = np.asarray(th, np.float32), np.asarray(orb_dist, np.int32)
    return pr


def pack_frame_rows(rows):
    """The three per-keypoint arrays of `rows` (a dict with FRAME_KEYS) as contiguous arrays of the ABI's types."""
    return _pack(rows, FRAME_KEYS, _FRAME_TYPES, "keypoint")


def pack_pt_rows(rows):
    """The five per-slot arrays of `rows` (a dict with PT_KEYS) as contiguous arrays of the ABI's types."""
    return _pack(rows, PT_KEYS, _PT_TYPES, "point")


class RelocProjector(Handle):
    """A handle for up to max_problems problems of one frame (up to max_keypoints <= 2400 keypoints) and the map-point slots of one keyframe each;
    max_points_total bounds the point rows and the skip rows of one call."""

    def __init__(self, max_problems=1024, max_keypoints=MAX_KEYPOINTS, max_points_total=1 << 20, device=0):
        super().__init__(_bind(lib()), "oslam_reloc_proj", max_problems, max_keypoints, max_points_total, device)

    def search_batch(self, problems, frame, pts, cam, bounds, scale_factors, log_scale_factor, check_orientation=True, skip=None, matched=None, n_matches=None,
                     n_removed=None, n_passes=None, n_pt_out=None, n_kp_out=None, device=False):
        """SearchByProjection of every problem.  problems: PROBLEM_DTYPE array (pack_problems); frame: dict of the per-keypoint arrays (FRAME_KEYS; has_mp =
        mvpMapPoints[i] != NULL on entry); pts: dict of the per-slot arrays (PT_KEYS); cam = (fx, fy, cx, cy); bounds = (mnMinX, mnMinY, mnMaxX, mnMaxY); skip
        None or uint8 [n_pt_out].  Returns dict(matched [n_kp_out] int32, n_matches, n_removed, n_passes [n_problems] int32); arrays given by the caller are
        written in place (rows the call does not write keep what they held).  device=True goes through the _device entry point on a side stream, over torch
        tensors."""
        problems, frame, pts = np.ascontiguousarray(problems, PROBLEM_DTYPE), pack_frame_rows(frame), pack_pt_rows(pts)
        n = len(problems)
        if n_pt_out is None:
            n_pt_out = len(skip) if skip is not None else _rows_of(problems, "n_pts", "pt_out_off")
        if n_kp_out is None:
            n_kp_out = len(matched) if matched is not None else _rows_of(problems, "n_kp", "kp_out_off")
        matched = np.full(n_kp_out, -1, np.int32) if matched is None else matched
        n_matches = np.zeros(n, np.int32) if n_matches is None else n_matches
        n_removed = np.zeros(n, np.int32) if n_removed is None else n_removed
        n_passes = np.zeros(n, np.int32) if n_passes is None else n_passes
        if skip is not None:
            skip = np.ascontiguousarray(skip, np.uint8)
            assert skip.size == n_pt_out
        outs = [matched, n_matches, n_removed, n_passes]
        for o, size in zip(outs, [n_kp_out, n, n, n]):
            assert o.dtype == np.int32 and o.size == size and o.flags.c_contiguous
        camera, bnd, sf = _camera_args(cam, bounds, scale_factors)

        def args(a):
            rf = FrameRows(len(frame["has_mp"]), *[a(frame[k]) for k in FRAME_KEYS])   # (byref keeps the structs alive until the call has returned)
            rp = PtRows(len(pts["Xw"]), *[a(pts[k]) for k in PT_KEYS])
            return ((self.h, n, a(problems), C.byref(rf), C.byref(rp), n_pt_out, a(skip), n_kp_out, C.addressof(camera), ptr(bnd), ptr(sf), len(sf), float(log_scale_factor),
                     int(bool(check_orientation))) + tuple(a(o) for o in outs))
        if not device:
            check(self.L.oslam_match_search_by_projection_reloc_batch(*args(optptr)))
        else:
            with device_call([problems, skip] + outs + [frame[k] for k in FRAME_KEYS] + [pts[k] for k in PT_KEYS], outputs=tuple(outs)) as (addr, stream):
                check(self.L.oslam_match_search_by_projection_reloc_batch_device(*args(addr), stream))
        return dict(matched=matched, n_matches=n_matches, n_removed=n_removed, n_passes=n_passes)
