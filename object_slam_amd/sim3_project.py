"""ctypes view of the Sim3 projection operators (include/oslam_hip.h, "Sim3 projection"): ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
(src/ORBmatcher.cc:290-403), which LoopClosing::ComputeSim3 runs over mvpLoopMapPoints before it accepts a loop (src/LoopClosing.cc:376, th = 10), and
ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:977-1100), which LoopClosing::SearchAndFuse runs once per corrected keyframe
(src/LoopClosing.cc:588-614, th = 4), for batches of independent problems.

`Sim3Projector.search_batch` and `.fuse_batch` are one launch of the gfx950 kernel over all problems (no CPU fallback: creating a Sim3Projector fails
without a device).  Keyframes and candidate points are rows of flat arrays; `pack_problems` builds the records that name them.
"""
import ctypes as C

import numpy as np

from ._lib import KP_DTYPE, Handle, check, device_call, lib, optptr, ptr
from ._proj_common import _camera_args, _pack, _problem_head, _rows_of

MAX_KEYPOINTS = 2400
SEARCH_TH, FUSE_TH = 10.0, 4.0   # src/LoopClosing.cc:376, :600
ACCEPT_MATCHES = 40              # src/LoopClosing.cc:386
FUSE_OCCUPANT, FUSE_ADDED = -2, -3


class Problem(C.Structure):    # oslam_sim3_proj_problem_t
    _fields_ = [("n_kp", C.c_int32), ("kp_off", C.c_int32), ("n_pts", C.c_int32), ("pt_off", C.c_int32), ("kp_out_off", C.c_int32), ("pt_out_off", C.c_int32),
                ("Scw", C.c_float * 16), ("th", C.c_float)]


class KfRows(C.Structure):     # oslam_sim3_proj_kf_rows_t
    _fields_ = [("n_rows", C.c_int32), ("keysUn", C.c_void_p), ("desc", C.c_void_p), ("state", C.c_void_p)]


class PtRows(C.Structure):     # oslam_sim3_proj_pt_rows_t
    _fields_ = [("n_rows", C.c_int32), ("Xw", C.c_void_p), ("normal", C.c_void_p), ("desc", C.c_void_p), ("maxDistance", C.c_void_p), ("minDistance", C.c_void_p)]


PROBLEM_DTYPE = np.dtype([("n_kp", "<i4"), ("kp_off", "<i4"), ("n_pts", "<i4"), ("pt_off", "<i4"), ("kp_out_off", "<i4"), ("pt_out_off", "<i4"), ("Scw", "<f4", (4, 4)),
                          ("th", "<f4")])
KF_KEYS = ("keysUn", "desc", "state")
PT_KEYS = ("Xw", "normal", "desc", "maxDistance", "minDistance")
_KF_TYPES = dict(keysUn=(KP_DTYPE, ()), desc=(np.uint8, (32,)), state=(np.uint8, ()))
_PT_TYPES = dict(Xw=(np.float32, (3,)), normal=(np.float32, (3,)), desc=(np.uint8, (32,)), maxDistance=(np.float32, ()), minDistance=(np.float32, ()))


def _bind(L):
    if getattr(L, "_oslam_sim3_proj_bound", False):
        return L
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    L.oslam_sim3_proj_create.argtypes = [C.POINTER(vp), i32, i32, i32, i32]
    L.oslam_sim3_proj_destroy.argtypes = [vp]
    L.oslam_sim3_proj_destroy.restype = None
    L.oslam_match_search_by_projection_sim3_batch.argtypes = [vp, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, i32, f32, vp, vp, vp]
    L.oslam_match_search_by_projection_sim3_batch_device.argtypes = [vp, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, i32, f32, vp, vp, vp, vp]
    L.oslam_match_fuse_sim3_batch.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, i32, f32, vp, vp, vp]
    L.oslam_match_fuse_sim3_batch_device.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, i32, f32, vp, vp, vp, vp]
    L._oslam_sim3_proj_bound = True
    return L


def pack_problems(n_kp, kp_off, n_pts, pt_off, Scw, th, kp_out_off=None, pt_out_off=None):
    """PROBLEM_DTYPE records.  kp_out_off / pt_out_off default to consecutive output rows, n_kp / n_pts per problem in the order given."""
    pr = _problem_head(PROBLEM_DTYPE, n_kp, kp_off, n_pts, pt_off, kp_out_off, pt_out_off)
    pr["Scw"] = np.asarray(Scw, np.float32).reshape(len(pr), 4, 4)
    pr["th"] = np.asarray(th, np.float32)
    return pr


def pack_kf_rows(rows):
    """The three per-keypoint arrays of `rows` (a dict with KF_KEYS) as contiguous arrays of the ABI's types."""
    return _pack(rows, KF_KEYS, _KF_TYPES, "keypoint")


def pack_pt_rows(rows):
    """The five per-point arrays of `rows` (a dict with PT_KEYS) as contiguous arrays of the ABI's types."""
    return _pack(rows, PT_KEYS, _PT_TYPES, "point")


class Sim3Projector(Handle):
    """A handle for up to max_problems problems of one keyframe (up to max_keypoints <= 2400 keypoints) and a list of candidate points each; max_points_total
    bounds the point rows and the per-problem-point rows (skip, fused_kp, replace) of one call."""

    def __init__(self, max_problems=1024, max_keypoints=MAX_KEYPOINTS, max_points_total=1 << 20, device=0):
        super().__init__(_bind(lib()), "oslam_sim3_proj", max_problems, max_keypoints, max_points_total, device)

    def _call(self, fuse, problems, kf, pts, cam, bounds, scale_factors, log_scale_factor, skip, n_pt_out, n_kp_out, outs, device):
        """outs: the int32 output arrays in the ABI's order (None for an optional one left out); they are written in place"""
        n = len(problems)
        if skip is not None:
            skip = np.ascontiguousarray(skip, np.uint8)
            assert skip.size == n_pt_out
        for o, size in zip(outs, ([n_pt_out, n_pt_out, n] if fuse else [n_kp_out, n, n])):
            assert o is None or (o.dtype == np.int32 and o.size == size and o.flags.c_contiguous)
        camera, bnd, sf = _camera_args(cam, bounds, scale_factors)
        name = "oslam_match_fuse_sim3_batch" if fuse else "oslam_match_search_by_projection_sim3_batch"

        def args(a):
            rk = KfRows(len(kf["state"]), *[a(kf[k]) for k in KF_KEYS])   # (byref keeps the structs alive until the call has returned)
            rp = PtRows(len(pts["Xw"]), *[a(pts[k]) for k in PT_KEYS])
            return ((self.h, n, a(problems), C.byref(rk), C.byref(rp), n_pt_out, a(skip)) + (() if fuse else (n_kp_out,))
                    + (C.addressof(camera), ptr(bnd), ptr(sf), len(sf), float(log_scale_factor)) + tuple(a(o) for o in outs))
        if not device:
            check(getattr(self.L, name)(*args(optptr)))
        else:
            with device_call([problems, skip] + list(outs) + [kf[k] for k in KF_KEYS] + [pts[k] for k in PT_KEYS], outputs=tuple(outs)) as (addr, stream):
                check(getattr(self.L, name + "_device")(*args(addr), stream))

    def search_batch(self, problems, kf, pts, cam, bounds, scale_factors, log_scale_factor, skip=None, matched=None, n_matches=None, n_passes=None, n_pt_out=None, n_kp_out=None,
                     device=False):
        """SearchByProjection of every problem.  problems: PROBLEM_DTYPE array (pack_problems); kf: dict of the per-keypoint arrays (KF_KEYS; state =
        vpMatched[idx] != NULL); pts: dict of the per-point arrays (PT_KEYS); cam = (fx, fy, cx, cy); bounds = (mnMinX, mnMinY, mnMaxX, mnMaxY); skip None or
        uint8 [n_pt_out].  Returns dict(matched [n_kp_out] int32, n_matches [n_problems] int32, n_passes [n_problems] int32); arrays given by the caller are
        written in place (rows the call does not write keep what they held).  device=True goes through the _device entry point on a side stream, over torch
        tensors."""
        problems, kf, pts = np.ascontiguousarray(problems, PROBLEM_DTYPE), pack_kf_rows(kf), pack_pt_rows(pts)
        n = len(problems)
        if n_pt_out is None:
            n_pt_out = len(skip) if skip is not None else _rows_of(problems, "n_pts", "pt_out_off")
        if n_kp_out is None:
            n_kp_out = len(matched) if matched is not None else _rows_of(problems, "n_kp", "kp_out_off")
        matched = np.full(n_kp_out, -1, np.int32) if matched is None else matched
        n_matches = np.zeros(n, np.int32) if n_matches is None else n_matches
        n_passes = np.zeros(n, np.int32) if n_passes is None else n_passes
        self._call(False, problems, kf, pts, cam, bounds, scale_factors, log_scale_factor, skip, n_pt_out, n_kp_out, [matched, n_matches, n_passes], device)
        return dict(matched=matched, n_matches=n_matches, n_passes=n_passes)

    def fuse_batch(self, problems, kf, pts, cam, bounds, scale_factors, log_scale_factor, skip=None, fused_kp=None, replace=None, n_fused=None, n_pt_out=None, device=False):
        """Fuse of every problem (kf["state"]: 0 = no map point at the keypoint, 1 = a good one, 2 = a bad one).  Returns dict(fused_kp [n_pt_out] int32,
        replace [n_pt_out] int32: -1, FUSE_ADDED, FUSE_OCCUPANT or a list index, n_fused [n_problems] int32); otherwise as search_batch."""
        problems, kf, pts = np.ascontiguousarray(problems, PROBLEM_DTYPE), pack_kf_rows(kf), pack_pt_rows(pts)
        n = len(problems)
        if n_pt_out is None:
            n_pt_out = len(fused_kp) if fused_kp is not None else len(skip) if skip is not None else _rows_of(problems, "n_pts", "pt_out_off")
        fused_kp = np.full(n_pt_out, -1, np.int32) if fused_kp is None else fused_kp
        replace = np.full(n_pt_out, -1, np.int32) if replace is None else replace
        n_fused = np.zeros(n, np.int32) if n_fused is None else n_fused
        self._call(True, problems, kf, pts, cam, bounds, scale_factors, log_scale_factor, skip, n_pt_out, 0, [fused_kp, replace, n_fused], device)
        return dict(fused_kp=fused_kp, replace=replace, n_fused=n_fused)
