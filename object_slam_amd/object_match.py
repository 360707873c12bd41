"""ctypes view of the object association (include/oslam_hip.h, "Object association"): what Tracking::TrackObject (src/Tracking.cc:1058-1076) runs per frame,
Frame::ExtractHSVHistogramsFromMask (src/Frame.cc:388-414), ObjectMatcher::MatchTwoFrame (src/ObjectMatcher.cc:47-440) and ObjectMatcher::MatchMapToFrame
(:442-801), for batches of independent frames.

`ObjectMatcher.hsv_histograms`, `.match_two_frame` and `.match_map_to_frame` are launches of the gfx950 kernels (no CPU fallback: creating an ObjectMatcher
fails without a device).  Detections, objects, observations and keypoints are rows of flat arrays; the `pack_*` helpers build the records that name them.
Operators: the driver does not call them and still takes the caller's track_id per detection.
"""
import ctypes as C

import numpy as np

from ._lib import Handle, check, device_call, lib, optptr, ptr
from ._proj_common import _consecutive

BINS = 94
MAX_DETECTIONS = 32
DONE, REFUSED_RECORD, REFUSED_NO_OBSERVATION, REFUSED_NO_KEYPOINT = 0, -1, -2, -3
MIN_SIMILARITY, MIN_IOU, MAX_MEAN_DIST, MAX_MIN_DIST = 0.8, 0.5, 0.3, 0.1   # src/ObjectMatcher.cc:430, :783, :789


class Params(C.Structure):       # oslam_objmatch_params_t
    _fields_ = [("min_similarity", C.c_double), ("min_iou", C.c_double), ("max_mean_dist", C.c_double), ("max_min_dist", C.c_double)]


class DetRows(C.Structure):      # oslam_objmatch_det_rows_t
    _fields_ = [("n_rows", C.c_int32), ("label", C.c_void_p), ("hist", C.c_void_p), ("box", C.c_void_p), ("obj3d", C.c_void_p), ("kp_off", C.c_void_p), ("kp_n", C.c_void_p),
                ("n_kps", C.c_int32), ("kps", C.c_void_p)]


class ObjRows(C.Structure):      # oslam_objmatch_obj_rows_t
    _fields_ = [("n_rows", C.c_int32), ("obj3d_id", C.c_void_p), ("label", C.c_void_p), ("obs_off", C.c_void_p), ("obs_n", C.c_void_p), ("n_obs", C.c_int32),
                ("obs_center", C.c_void_p), ("obs_hist", C.c_void_p)]


FRAME_DTYPE = np.dtype([("n_masks", "<i4"), ("mask_off", "<i4")])
PAIR_DTYPE = np.dtype([("n_pre", "<i4"), ("off_pre", "<i4"), ("n_cur", "<i4"), ("off_cur", "<i4"), ("off_score", "<i4"), ("reserved", "<i4", (3,))])
MAP_DTYPE = np.dtype([("n_cur", "<i4"), ("off_cur", "<i4"), ("n_obj", "<i4"), ("off_obj", "<i4"), ("off_score", "<i4"), ("reserved", "<i4"), ("Rwc", "<f4", (9,)), ("Ow", "<f4", (3,)),
                      ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4")])
_DET_TYPES = dict(label=(np.int32, ()), hist=(np.float32, (BINS,)), box=(np.float32, (4,)), obj3d=(np.int32, ()), kp_off=(np.int32, ()), kp_n=(np.int32, ()))
_OBJ_TYPES = dict(obj3d_id=(np.int32, ()), label=(np.int32, ()), obs_off=(np.int32, ()), obs_n=(np.int32, ()))


def _bind(L):
    if getattr(L, "_oslam_objmatch_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int
    L.oslam_objmatch_create.argtypes = [C.POINTER(vp)] + [i32] * 7
    L.oslam_objmatch_destroy.argtypes = [vp]
    L.oslam_objmatch_destroy.restype = None
    L.oslam_objmatch_hsv_histograms.argtypes = [vp] + [i32] * 5 + [vp, vp, i32, vp, vp, vp]
    L.oslam_objmatch_hsv_histograms_device.argtypes = [vp] + [i32] * 5 + [vp, vp, i32, vp, vp, vp, vp]
    L.oslam_objmatch_match_two_frame.argtypes = [vp, i32, vp, vp, vp, vp, i32] + [vp] * 4
    L.oslam_objmatch_match_two_frame_device.argtypes = [vp, i32, vp, vp, vp, vp, i32] + [vp] * 5
    L.oslam_objmatch_match_map_to_frame.argtypes = [vp, i32, vp, vp, vp, vp, i32] + [vp] * 6
    L.oslam_objmatch_match_map_to_frame_device.argtypes = [vp, i32, vp, vp, vp, vp, i32] + [vp] * 7
    L.oslam_objmatch_set_timing.argtypes = [vp, i32]
    L.oslam_objmatch_last_kernel_ms.argtypes = [vp, vp]
    L._oslam_objmatch_bound = True
    return L


def make_params(min_similarity=MIN_SIMILARITY, min_iou=MIN_IOU, max_mean_dist=MAX_MEAN_DIST, max_min_dist=MAX_MIN_DIST):
    return Params(min_similarity, min_iou, max_mean_dist, max_min_dist)


def pack_frames(n_masks, mask_off=None):
    """FRAME_DTYPE records.  mask_off defaults to consecutive masks in the order given."""
    n = np.asarray(n_masks, np.int32).reshape(-1)
    fr = np.zeros(len(n), FRAME_DTYPE)
    fr["n_masks"], fr["mask_off"] = n, _consecutive(n) if mask_off is None else np.asarray(mask_off, np.int32)
    return fr


def pack_pair_problems(n_pre, n_cur, off_pre=None, off_cur=None, off_score=None):
    """PAIR_DTYPE records.  The offsets default to consecutive rows and score blocks."""
    n_pre, n_cur = np.asarray(n_pre, np.int32).reshape(-1), np.asarray(n_cur, np.int32).reshape(-1)
    pr = np.zeros(len(n_pre), PAIR_DTYPE)
    pr["n_pre"], pr["n_cur"] = n_pre, n_cur
    pr["off_pre"] = _consecutive(n_pre) if off_pre is None else np.asarray(off_pre, np.int32)
    pr["off_cur"] = _consecutive(n_cur) if off_cur is None else np.asarray(off_cur, np.int32)
    pr["off_score"] = _consecutive(n_pre * n_cur) if off_score is None else np.asarray(off_score, np.int32)
    return pr


def pack_map_problems(n_cur, n_obj, Rwc, Ow, K, off_cur=None, off_obj=None, off_score=None):
    """MAP_DTYPE records.  Rwc [n, 9] or [n, 3, 3], Ow [n, 3], K = (fx, fy, cx, cy) for all or [n, 4]."""
    n_cur, n_obj = np.asarray(n_cur, np.int32).reshape(-1), np.asarray(n_obj, np.int32).reshape(-1)
    n = len(n_cur)
    pr = np.zeros(n, MAP_DTYPE)
    pr["n_cur"], pr["n_obj"] = n_cur, n_obj
    pr["off_cur"] = _consecutive(n_cur) if off_cur is None else np.asarray(off_cur, np.int32)
    pr["off_obj"] = _consecutive(n_obj) if off_obj is None else np.asarray(off_obj, np.int32)
    pr["off_score"] = _consecutive(n_cur * n_obj) if off_score is None else np.asarray(off_score, np.int32)
    pr["Rwc"], pr["Ow"] = np.asarray(Rwc, np.float32).reshape(n, 9), np.asarray(Ow, np.float32).reshape(n, 3)
    K = np.broadcast_to(np.asarray(K, np.float32), (n, 4))
    pr["fx"], pr["fy"], pr["cx"], pr["cy"] = K[:, 0], K[:, 1], K[:, 2], K[:, 3]
    return pr


def _rows(rows, types, what):
    """the arrays of `rows` that `types` names, contiguous and of the ABI's types; all present ones have the same number of rows"""
    out, n = {}, None
    for k, (dt, shape) in types.items():
        if rows.get(k) is None:
            continue
        a = rows[k] if isinstance(rows[k], np.ndarray) and rows[k].dtype == dt and rows[k].flags.c_contiguous else np.ascontiguousarray(rows[k], dt)
        a = a.reshape((-1,) + shape)
        assert n is None or len(a) == n, "%s rows: %s has %d entries, not %d" % (what, k, len(a), n)
        out[k], n = a, len(a)
    return out, n or 0


def pack_det_rows(rows):
    """A dict of detection rows as contiguous arrays: label, hist [n, 94], obj3d, and box [n, 4] (MatchTwoFrame) or kp_off, kp_n and kps [., 3] (MatchMapToFrame)."""
    out, n = _rows(rows, _DET_TYPES, "detection")
    if rows.get("kps") is not None:
        out["kps"] = np.ascontiguousarray(rows["kps"], np.float32).reshape(-1, 3)
    return out, n


def pack_obj_rows(rows):
    """A dict of object rows as contiguous arrays: obj3d_id, label, obs_off, obs_n, obs_center [., 3], obs_hist [., 94]."""
    out, n = _rows(rows, _OBJ_TYPES, "object")
    out["obs_center"] = np.ascontiguousarray(rows["obs_center"], np.float32).reshape(-1, 3)
    out["obs_hist"] = np.ascontiguousarray(rows["obs_hist"], np.float32).reshape(-1, BINS)
    assert len(out["obs_center"]) == len(out["obs_hist"])
    return out, n


class ObjectMatcher(Handle):
    """A handle for calls of up to max_frames frames (or problems) of up to max_width x max_height pixels and max_detections <= 32 detections each, maps of up to
    max_objects objects per problem, and flat observation and keypoint arrays of the given sizes."""

    def __init__(self, max_frames=64, max_width=640, max_height=480, max_detections=8, max_objects=64, max_observations_total=1 << 16, max_keypoints_total=1 << 18):
        super().__init__(_bind(lib()), "oslam_objmatch", max_frames, max_width, max_height, max_detections, max_objects, max_observations_total, max_keypoints_total)

    def set_timing(self, on=True):
        check(self.L.oslam_objmatch_set_timing(self.h, int(bool(on))))

    def last_kernel_ms(self):
        """milliseconds of the last call's kernels: (counting, combine) of a histogram call, (the kernel, 0) of a matcher call; needs set_timing()"""
        ms = np.zeros(2, np.float32)
        check(self.L.oslam_objmatch_last_kernel_ms(self.h, ptr(ms)))
        return float(ms[0]), float(ms[1])

    def hsv_histograms(self, images, masks, frames=None, width=None, counts=None, hist=None, device=False):
        """images: uint8 [n_frames, H, stride] (stride >= 3 * width bytes; width defaults to stride // 3), read as B, G, R; masks: uint8 [n_masks_total, H, mask_stride];
        frames: FRAME_DTYPE records (pack_frames), default: one frame per image with all masks split evenly.  Returns dict(counts int32 [n_masks_total, 94],
        hist float32 [n_masks_total, 94]); arrays given by the caller are written in place."""
        assert images.dtype == np.uint8 and images.ndim == 3 and images.flags.c_contiguous and masks.dtype == np.uint8 and masks.ndim == 3 and masks.flags.c_contiguous
        nf, H, stride = images.shape
        nm, mstride = masks.shape[0], masks.shape[2]
        assert masks.shape[1] == H or nm == 0
        W = stride // 3 if width is None else int(width)
        frames = pack_frames([nm // nf] * nf) if frames is None else np.ascontiguousarray(frames, FRAME_DTYPE)
        assert len(frames) == nf
        counts = np.zeros((nm, BINS), np.int32) if counts is None else counts
        hist = np.zeros((nm, BINS), np.float32) if hist is None else hist
        assert counts.dtype == np.int32 and counts.size == nm * BINS and counts.flags.c_contiguous and hist.dtype == np.float32 and hist.size == nm * BINS and hist.flags.c_contiguous
        head = (self.h, nf, W, H, stride, mstride)
        if not device:
            check(self.L.oslam_objmatch_hsv_histograms(*head, ptr(images), ptr(frames), nm, optptr(masks if nm else None), optptr(counts if nm else None), optptr(hist if nm else None)))
        else:
            with device_call([images, frames, masks, counts, hist], outputs=(counts, hist)) as (addr, stream):
                check(self.L.oslam_objmatch_hsv_histograms_device(*head, addr(images), addr(frames), nm, addr(masks), addr(counts), addr(hist), stream))
        return dict(counts=counts, hist=hist)

    def match_two_frame(self, problems, pre, cur, params=None, similarity=None, iou=None, n_assigned=None, status=None, n_scores=None, device=False):
        """MatchTwoFrame of every problem.  problems: PAIR_DTYPE (pack_pair_problems); pre / cur: dicts of detection rows with label, hist, box, obj3d (pre: the
        Object3D ids and labels of the previous frame's objects).  cur["obj3d"] is written in place when it is a contiguous int32 array, and returned.  Returns
        dict(cur_obj3d, similarity, iou [n_scores] float32, n_assigned, status [n_problems] int32)."""
        problems = np.ascontiguousarray(problems, PAIR_DTYPE)
        params = make_params() if params is None else params
        (pre, n_pre), (cur, n_cur) = pack_det_rows(pre), pack_det_rows(cur)
        n = len(problems)
        if n_scores is None:
            n_scores = int(max([0] + [int(p["off_score"]) + int(p["n_pre"]) * int(p["n_cur"]) for p in problems])) if similarity is None else similarity.size
        similarity = np.full(n_scores, np.nan, np.float32) if similarity is None else similarity
        iou = np.full(n_scores, np.nan, np.float32) if iou is None else iou
        n_assigned = np.zeros(n, np.int32) if n_assigned is None else n_assigned
        status = np.zeros(n, np.int32) if status is None else status
        outs = [cur.get("obj3d"), similarity, iou, n_assigned, status]
        keys = ("label", "hist", "box", "obj3d")
        arrays = [problems] + [pre.get(k) for k in keys] + [cur.get(k) for k in keys[:3]] + outs

        def args(a):
            rp = DetRows(n_pre, a(pre.get("label")), a(pre.get("hist")), a(pre.get("box")), a(pre.get("obj3d")), None, None, 0, None)
            rc = DetRows(n_cur, a(cur.get("label")), a(cur.get("hist")), a(cur.get("box")), a(cur.get("obj3d")), None, None, 0, None)
            return (self.h, n, a(problems), C.byref(rp), C.byref(rc), C.byref(params), n_scores) + tuple(a(o) for o in outs[1:])
        if not device:
            check(self.L.oslam_objmatch_match_two_frame(*args(optptr)))
        else:
            with device_call(arrays, outputs=tuple(outs)) as (addr, stream):
                check(self.L.oslam_objmatch_match_two_frame_device(*args(addr), stream))
        return dict(cur_obj3d=cur.get("obj3d"), similarity=similarity, iou=iou, n_assigned=n_assigned, status=status)

    def match_map_to_frame(self, problems, cur, objects, params=None, similarity=None, mean_dist=None, min_dist=None, n_by_similarity=None, n_by_distance=None, status=None,
                           n_scores=None, device=False):
        """MatchMapToFrame of every problem.  problems: MAP_DTYPE (pack_map_problems); cur: detection rows with label, hist, obj3d, kp_off, kp_n and kps; objects:
        object rows (pack_obj_rows' keys).  Returns dict(cur_obj3d, similarity, mean_dist, min_dist [n_scores], n_by_similarity, n_by_distance, status [n_problems])."""
        problems = np.ascontiguousarray(problems, MAP_DTYPE)
        params = make_params() if params is None else params
        (cur, n_cur), (obj, n_obj) = pack_det_rows(cur), pack_obj_rows(objects)
        n, n_kps, n_obs = len(problems), len(cur["kps"]) if cur.get("kps") is not None else 0, len(obj["obs_center"])
        if n_scores is None:
            n_scores = int(max([0] + [int(p["off_score"]) + int(p["n_obj"]) * int(p["n_cur"]) for p in problems])) if similarity is None else similarity.size
        scores = [np.full(n_scores, np.nan, np.float32) if s is None else s for s in (similarity, mean_dist, min_dist)]
        ints = [np.zeros(n, np.int32) if s is None else s for s in (n_by_similarity, n_by_distance, status)]
        outs = [cur.get("obj3d")] + scores + ints
        ck, ok = ("label", "hist", "kp_off", "kp_n", "kps"), ("obj3d_id", "label", "obs_off", "obs_n", "obs_center", "obs_hist")
        arrays = [problems] + [cur.get(k) for k in ck] + [obj.get(k) for k in ok] + outs

        def args(a):
            rc = DetRows(n_cur, a(cur.get("label")), a(cur.get("hist")), None, a(cur.get("obj3d")), a(cur.get("kp_off")), a(cur.get("kp_n")), n_kps, a(cur.get("kps")))
            ro = ObjRows(n_obj, a(obj.get("obj3d_id")), a(obj.get("label")), a(obj.get("obs_off")), a(obj.get("obs_n")), n_obs, a(obj.get("obs_center")), a(obj.get("obs_hist")))
            return (self.h, n, a(problems), C.byref(rc), C.byref(ro), C.byref(params), n_scores) + tuple(a(o) for o in outs[1:])
        if not device:
            check(self.L.oslam_objmatch_match_map_to_frame(*args(optptr)))
        else:
            with device_call(arrays, outputs=tuple(outs)) as (addr, stream):
                check(self.L.oslam_objmatch_match_map_to_frame_device(*args(addr), stream))
        return dict(cur_obj3d=cur.get("obj3d"), similarity=scores[0], mean_dist=scores[1], min_dist=scores[2], n_by_similarity=ints[0], n_by_distance=ints[1], status=ints[2])
