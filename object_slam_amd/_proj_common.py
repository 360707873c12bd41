"""What the ctypes views of the windowed projection searches (sim3_match.py, sim3_project.py, reloc_project.py) share: row packing, the leading ints of a
problem record, and the camera arguments."""
import numpy as np

from .matcher import Camera


def _consecutive(n):
    return np.concatenate([[0], np.cumsum(np.maximum(n, 0))[:-1]]) if len(n) else np.zeros(0, np.int64)


def _pack(rows, keys, types, what):
    out = {}
    for k in keys:
        dt, shape = types[k]
        out[k] = np.ascontiguousarray(rows[k], dt).reshape((-1,) + shape)
    n = len(out[keys[0]])
    assert all(len(v) == n for v in out.values()), "the per-%s arrays differ in length" % what
    return out


def _rows_of(pr, n_field, off_field):
    return int((pr[off_field].astype(np.int64) + np.maximum(pr[n_field], 0)).max()) if len(pr) else 0


def _problem_head(dtype, n_kp, kp_off, n_pts, pt_off, kp_out_off, pt_out_off):
    """Records of `dtype` with the six leading ints of both projection operators filled in; kp_out_off / pt_out_off default to consecutive output rows."""
    n_kp, n_pts = np.asarray(n_kp, np.int32).reshape(-1), np.asarray(n_pts, np.int32).reshape(-1)
    pr = np.zeros(len(n_kp), dtype)
    pr["n_kp"], pr["kp_off"], pr["n_pts"], pr["pt_off"] = n_kp, np.asarray(kp_off, np.int32), n_pts, np.asarray(pt_off, np.int32)
    pr["kp_out_off"] = _consecutive(n_kp) if kp_out_off is None else np.asarray(kp_out_off, np.int32)
    pr["pt_out_off"] = _consecutive(n_pts) if pt_out_off is None else np.asarray(pt_out_off, np.int32)
    return pr


def _camera_args(cam, bounds, scale_factors):
    """(oslam_camera_t, bounds [4] float32, scaleFactors float32) of cam = (fx, fy, cx, cy, ...); the caller keeps them alive until the call has returned"""
    c = np.asarray(cam, np.float32).reshape(-1)
    return Camera(c[0], c[1], c[2], c[3], 0.0, 0.0), np.ascontiguousarray(bounds, np.float32).reshape(4), np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
