"""ctypes view of the map corrections of LoopClosing (include/oslam_hip.h, "LoopClosing: map corrections"): mg2oScw = gScm * gSmw
(src/LoopClosing.cc:334-336), CorrectLoop's Sim3 propagation with its point correction and corrected poses (:436-517), and the map update after global
BA (:677-738), for batches of independent sequences.

Every method of `LoopCorrector` runs the gfx950 kernels (no CPU fallback: creating the handle fails without a device).  The driver does not close
loops and calls none of this.
"""
import ctypes as C

import numpy as np

from ._lib import Handle, check, device_call, lib, optptr


class Problem(C.Structure):      # oslam_loop_correct_problem_t
    _fields_ = [("n_kf", C.c_int32), ("kf_offset", C.c_int32), ("cur", C.c_int32), ("n_points", C.c_int32), ("point_offset", C.c_int32), ("n_entries", C.c_int32),
                ("entry_offset", C.c_int32), ("reserved", C.c_int32)]


class GbaProblem(C.Structure):   # oslam_loop_gba_problem_t
    _fields_ = [("n_kf", C.c_int32), ("kf_offset", C.c_int32), ("n_points", C.c_int32), ("point_offset", C.c_int32), ("refuse", C.c_int32), ("reserved", C.c_int32 * 3)]


PROBLEM_DTYPE = np.dtype([("n_kf", "<i4"), ("kf_offset", "<i4"), ("cur", "<i4"), ("n_points", "<i4"), ("point_offset", "<i4"), ("n_entries", "<i4"), ("entry_offset", "<i4"),
                          ("reserved", "<i4")])
GBA_PROBLEM_DTYPE = np.dtype([("n_kf", "<i4"), ("kf_offset", "<i4"), ("n_points", "<i4"), ("point_offset", "<i4"), ("refuse", "<i4"), ("reserved", "<i4", (3,))])


def _bind(L):
    if getattr(L, "_oslam_loop_correct_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int
    L.oslam_loop_correct_create.argtypes = [C.POINTER(vp), i32, i32, i32, i32, i32]
    L.oslam_loop_correct_destroy.argtypes = [vp]
    L.oslam_loop_correct_destroy.restype = None
    L.oslam_loop_compose_scw.argtypes = [vp, i32, vp, vp, vp, vp]
    L.oslam_loop_compose_scw_device.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.oslam_loop_propagate.argtypes = [vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.oslam_loop_propagate_device.argtypes = L.oslam_loop_propagate.argtypes + [vp]
    L.oslam_loop_update_after_gba.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.oslam_loop_update_after_gba_device.argtypes = L.oslam_loop_update_after_gba.argtypes + [vp]
    L._oslam_loop_correct_bound = True
    return L


def _out(a, shape, dtype):
    """the caller's output array (checked) or a new one of zeros"""
    if a is None:
        return np.zeros(shape, dtype)
    assert a.dtype == dtype and a.size == int(np.prod(shape)) and a.flags.c_contiguous
    return a


class LoopCorrector(Handle):
    """A handle for up to max_problems problems with max_keyframes keyframes, max_entries (keyframe, keypoint) entries and max_points points in all."""

    def __init__(self, max_problems=64, max_keyframes=1 << 12, max_entries=1 << 20, max_points=1 << 20, device=0):
        super().__init__(_bind(lib()), "oslam_loop_correct", max_problems, max_keyframes, max_entries, max_points, device)

    def compose_scw(self, Scm, Tmw, device=False):
        """mg2oScw = gScm * gSmw (:334-336).  Scm [n, 13] float64 = R row-major, t, s; Tmw [n, 4, 4] float32.  Returns (Scw [n, 13] float64 = R, t, s; mScw
        [n, 4, 4] float32 = Converter::toCvMat(Scw))."""
        Scm = np.ascontiguousarray(Scm, np.float64).reshape(-1, 13)
        Tmw = np.ascontiguousarray(Tmw, np.float32).reshape(-1, 16)
        n = len(Scm)
        assert len(Tmw) == n
        Scw, mScw = np.zeros((n, 13), np.float64), np.zeros((n, 4, 4), np.float32)
        if not device:
            check(self.L.oslam_loop_compose_scw(self.h, n, optptr(Scm), optptr(Tmw), optptr(Scw), optptr(mScw)))
        else:
            with device_call((Scm, Tmw, Scw, mScw), outputs=(Scw, mScw)) as (a, stream):
                check(self.L.oslam_loop_compose_scw_device(self.h, n, a(Scm), a(Tmw), a(Scw), a(mScw), stream))
        return Scw, mScw

    def propagate(self, problems, Tiw, Scw, kf_entries, entries, P, bad, Scorr_out=None, Snc_out=None, Tiw_out=None, P_out=None, corrected_ref=None, status=None, device=False):
        """CorrectLoop's propagation (:436-517).  problems: PROBLEM_DTYPE array; Tiw [N, 4, 4] float32; Scw [n, 13] float64; kf_entries [N, 2] int32 = first,
        count; entries [E] int32; P [M, 3] float32; bad [M] uint8.  Returns dict(Scorr, Snc [N, 13] float64 = R, t, s; Tiw [N, 4, 4] float32; P [M, 3] float32;
        corrected_ref [M] int32; status [n, 4] int32).  Output arrays given by the caller are written in place: what the call does not write keeps what it
        held."""
        problems = np.ascontiguousarray(problems, PROBLEM_DTYPE)
        Tiw = np.ascontiguousarray(Tiw, np.float32).reshape(-1, 16)
        Scw = np.ascontiguousarray(Scw, np.float64).reshape(-1, 13)
        kf_entries = np.ascontiguousarray(kf_entries, np.int32).reshape(-1, 2)
        entries = np.ascontiguousarray(entries, np.int32).reshape(-1)
        P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
        bad = np.ascontiguousarray(bad, np.uint8).reshape(-1)
        n, N, E, M = len(problems), len(Tiw), len(entries), len(P)
        assert len(Scw) == n and len(kf_entries) == N and len(bad) == M
        Scorr_out, Snc_out = _out(Scorr_out, (N, 13), np.float64), _out(Snc_out, (N, 13), np.float64)
        Tiw_out, P_out = _out(Tiw_out, (N, 4, 4), np.float32), _out(P_out, (M, 3), np.float32)
        corrected_ref, status = _out(corrected_ref, (M,), np.int32), _out(status, (n, 4), np.int32)
        if not device:
            check(self.L.oslam_loop_propagate(self.h, n, optptr(problems), N, optptr(Tiw), optptr(Scw), optptr(kf_entries), E, optptr(entries), M, optptr(P), optptr(bad),
                                              optptr(Scorr_out), optptr(Snc_out), optptr(Tiw_out), optptr(P_out), optptr(corrected_ref), optptr(status)))
        else:
            outs = (Scorr_out, Snc_out, Tiw_out, P_out, corrected_ref, status)
            with device_call((problems, Tiw, Scw, kf_entries, entries, P, bad) + outs, outputs=outs) as (a, stream):
                check(self.L.oslam_loop_propagate_device(self.h, n, a(problems), N, a(Tiw), a(Scw), a(kf_entries), E, a(entries), M, a(P), a(bad), a(Scorr_out), a(Snc_out),
                                                         a(Tiw_out), a(P_out), a(corrected_ref), a(status), stream))
        return dict(Scorr=Scorr_out.reshape(N, 13), Snc=Snc_out.reshape(N, 13), Tiw=Tiw_out.reshape(N, 4, 4), P=P_out.reshape(M, 3), corrected_ref=corrected_ref.reshape(M),
                    status=status.reshape(n, 4))

    def update_after_gba(self, problems, parent, kf_in_ba, Tcw, TcwGBA, P, PosGBA, pt_in_ba, bad, ref, Tcw_out=None, reached=None, P_out=None, status=None, device=False):
        """The map update after global BA (:677-738).  problems: GBA_PROBLEM_DTYPE array; parent [N] int32; kf_in_ba [N] uint8; Tcw, TcwGBA [N, 4, 4] float32; P,
        PosGBA [M, 3] float32; pt_in_ba, bad [M] uint8; ref [M] int32.  Returns dict(Tcw [N, 4, 4] float32, reached [N] uint8, P [M, 3] float32, status
        [n, 4] int32).  device=False validates `parent` on the host first (a cycle: status -1); hand no cyclic `parent` to device=True."""
        problems = np.ascontiguousarray(problems, GBA_PROBLEM_DTYPE)
        parent = np.ascontiguousarray(parent, np.int32).reshape(-1)
        kf_in_ba = np.ascontiguousarray(kf_in_ba, np.uint8).reshape(-1)
        Tcw, TcwGBA = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 16), np.ascontiguousarray(TcwGBA, np.float32).reshape(-1, 16)
        P, PosGBA = np.ascontiguousarray(P, np.float32).reshape(-1, 3), np.ascontiguousarray(PosGBA, np.float32).reshape(-1, 3)
        pt_in_ba, bad = np.ascontiguousarray(pt_in_ba, np.uint8).reshape(-1), np.ascontiguousarray(bad, np.uint8).reshape(-1)
        ref = np.ascontiguousarray(ref, np.int32).reshape(-1)
        n, N, M = len(problems), len(parent), len(P)
        assert len(kf_in_ba) == N and len(Tcw) == N and len(TcwGBA) == N and len(PosGBA) == M and len(pt_in_ba) == M and len(bad) == M and len(ref) == M
        Tcw_out, reached = _out(Tcw_out, (N, 4, 4), np.float32), _out(reached, (N,), np.uint8)
        P_out, status = _out(P_out, (M, 3), np.float32), _out(status, (n, 4), np.int32)
        if not device:
            check(self.L.oslam_loop_update_after_gba(self.h, n, optptr(problems), N, optptr(parent), optptr(kf_in_ba), optptr(Tcw), optptr(TcwGBA), M, optptr(P), optptr(PosGBA),
                                                     optptr(pt_in_ba), optptr(bad), optptr(ref), optptr(Tcw_out), optptr(reached), optptr(P_out), optptr(status)))
        else:
            outs = (Tcw_out, reached, P_out, status)
            with device_call((problems, parent, kf_in_ba, Tcw, TcwGBA, P, PosGBA, pt_in_ba, bad, ref) + outs, outputs=outs) as (a, stream):
                check(self.L.oslam_loop_update_after_gba_device(self.h, n, a(problems), N, a(parent), a(kf_in_ba), a(Tcw), a(TcwGBA), M, a(P), a(PosGBA), a(pt_in_ba), a(bad),
                                                                a(ref), a(Tcw_out), a(reached), a(P_out), a(status), stream))
        return dict(Tcw=Tcw_out.reshape(N, 4, 4), reached=reached.reshape(N), P=P_out.reshape(M, 3), status=status.reshape(n, 4))
