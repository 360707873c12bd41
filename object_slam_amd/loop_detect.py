"""ctypes view of the loop detector (include/oslam_hip.h, "LoopClosing::DetectLoop"): LoopClosing::DetectLoop (src/LoopClosing.cc:104-230) for many
independent sequences, over a KeyFrameDatabase that it borrows.  The connected-keyframe bitsets of the keyframes and mvConsistentGroups live on the device.

`LoopDetector.detect` is the kfdb's loop query with its bound derived on the device, followed by the consistency update over that query's candidates:
two launches on one stream (no CPU fallback).  The gate `mnId < mLastLoopKFid + 10` and `mpKeyFrameDB->add` stay with the caller.
"""
import ctypes as C

import numpy as np

from ._lib import Handle, check, device_call, lib, optptr
from .keyframe_db import QUERY_DTYPE, _bind as _bind_kfdb

MAX_GROUPS = 64   # OSLAM_LOOPDET_MAX_GROUPS

CONN_DTYPE = np.dtype([("database", "<i4"), ("keyframe", "<i4"), ("off", "<i4"), ("n", "<i4")])   # oslam_loopdet_conn_t
UPDATE_DTYPE = np.dtype([("database", "<i4"), ("cand_off", "<i4"), ("n_cand", "<i4")])            # oslam_loopdet_update_t


class Conn(C.Structure):      # oslam_loopdet_conn_t
    _fields_ = [("database", C.c_int32), ("keyframe", C.c_int32), ("off", C.c_int32), ("n", C.c_int32)]


class Update(C.Structure):    # oslam_loopdet_update_t
    _fields_ = [("database", C.c_int32), ("cand_off", C.c_int32), ("n_cand", C.c_int32)]


def _bind(L):
    if getattr(L, "_oslam_loopdet_bound", False):
        return L
    _bind_kfdb(L)
    vp, i32 = C.c_void_p, C.c_int
    L.oslam_loopdet_create.argtypes = [C.POINTER(vp), vp, i32, i32]
    L.oslam_loopdet_destroy.argtypes = [vp]
    L.oslam_loopdet_destroy.restype = None
    L.oslam_loopdet_set_connected.argtypes = [vp, i32, vp, i32, vp]
    L.oslam_loopdet_reset.argtypes = [vp, i32, vp]
    L.oslam_loopdet_get_groups.argtypes = [vp, i32, vp, vp, vp]
    L.oslam_loopdet_update_consistency.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp]
    L.oslam_loopdet_update_consistency_device.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp]
    L.oslam_loopdet_detect.argtypes = [vp, vp, i32, vp, i32, vp, vp, i32, vp] + [vp] * 9
    L.oslam_loopdet_detect_device.argtypes = [vp, vp, i32, vp, i32, vp, vp, i32, vp] + [vp] * 10
    L._oslam_loopdet_bound = True
    return L


def _flat(lists):
    cnt = np.array([len(l) for l in lists], np.int32)
    off = (np.concatenate([[0], np.cumsum(cnt)[:-1]]) if len(cnt) else np.zeros(0)).astype(np.int32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(l, np.int32).reshape(-1) for l in lists] + [np.zeros(0, np.int32)]))
    return off, cnt, flat


def pack_connected(databases, keyframes, lists):
    """(CONN_DTYPE records, ids): lists[i] = the ids of GetConnectedKeyFrames() of keyframes[i] of databases[i]."""
    rec = np.zeros(len(lists), CONN_DTYPE)
    rec["database"], rec["keyframe"] = np.asarray(databases, np.int32), np.asarray(keyframes, np.int32)
    rec["off"], rec["n"], ids = _flat(lists)
    return rec, ids


def pack_updates(databases, candidates):
    """(UPDATE_DTYPE records, cand): candidates[i] = vpCandidateKFs of databases[i], ids in the query's order."""
    rec = np.zeros(len(candidates), UPDATE_DTYPE)
    rec["database"] = np.asarray(databases, np.int32)
    rec["cand_off"], rec["n_cand"], cand = _flat(candidates)
    return rec, cand


def bits_to_ids(bits):
    """the ids of one bitset row (uint32 words, bit i of word i // 32 = id i), ascending"""
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(bits, "<u4").view(np.uint8), bitorder="little")).tolist()


class LoopDetector(Handle):
    """A detector over `kfdb` (a KeyFrameDatabase, which must outlive it): its databases, max_keyframes, device and stream.  max_groups <= 64 groups per
    database; consistency_th is mnCovisibilityConsistencyTh."""

    def __init__(self, kfdb, max_groups=MAX_GROUPS, consistency_th=3):
        super().__init__(_bind(lib()), "oslam_loopdet", kfdb.h, max_groups, consistency_th)
        self.kfdb, self.max_groups, self.consistency_th = kfdb, max_groups, consistency_th
        self.n_databases, self.max_keyframes = kfdb.n_databases, kfdb.max_keyframes
        self.words = (kfdb.max_keyframes + 31) // 32

    def set_connected(self, rec, ids):
        """KeyFrame::GetConnectedKeyFrames of every record (pack_connected): whole rows, in record order."""
        rec, ids = np.ascontiguousarray(rec, CONN_DTYPE), np.ascontiguousarray(ids, np.int32)
        check(self.L.oslam_loopdet_set_connected(self.h, len(rec), optptr(rec), len(ids), optptr(ids)))

    def reset(self, databases):
        d = np.ascontiguousarray(np.atleast_1d(databases), np.int32)
        check(self.L.oslam_loopdet_reset(self.h, len(d), optptr(d)))

    def get_groups(self, database):
        """mvConsistentGroups of one database in list order: [(sorted ids of the group, consistency counter)]."""
        n = np.zeros(1, np.int32)
        cnt, bits = np.zeros(self.max_groups, np.int32), np.zeros((self.max_groups, self.words), np.uint32)
        check(self.L.oslam_loopdet_get_groups(self.h, int(database), optptr(n), optptr(cnt), optptr(bits)))
        return [(bits_to_ids(bits[g]), int(cnt[g])) for g in range(int(n[0]))]

    def _outputs(self, n):
        # fills no result has: what a query does not write stays visible
        return np.full((n, self.max_keyframes), -1, np.int32), np.full(n, -9, np.int32), np.full(n, -9, np.int32)

    def update_consistency(self, rec, cand, device=False):
        """:144-226 given the candidates (pack_updates).  Returns dict(enough [n, max_keyframes] int32: row q holds n_enough[q] ids in candidate order,
        n_enough [n] (-2 / -3: refused, the groups are unchanged), n_groups [n])."""
        rec, cand = np.ascontiguousarray(rec, UPDATE_DTYPE), np.ascontiguousarray(cand, np.int32)
        n = len(rec)
        enough, n_enough, n_groups = self._outputs(n)
        args = lambda a: (self.h, n, a(rec), len(cand), a(cand), a(enough), a(n_enough), a(n_groups))   # noqa: E731
        if not device:
            check(self.L.oslam_loopdet_update_consistency(*args(optptr)))
        else:
            with device_call([rec, cand, enough, n_enough, n_groups], outputs=(enough, n_enough, n_groups)) as (addr, stream):
                check(self.L.oslam_loopdet_update_consistency_device(*args(addr), stream))
        return dict(enough=enough, n_enough=n_enough, n_groups=n_groups)

    def detect(self, rec, ids, vals, conn, device=False, voc=None):
        """:122-226 for the current keyframe of every query (keyframe_db.pack_queries with connected; min_scores are ignored).  Returns what
        KeyFrameDatabase.detect_loop_candidates returns plus min_score [n] (the derived bound), enough, n_enough and n_groups."""
        rec, ids, vals = np.ascontiguousarray(rec, QUERY_DTYPE), np.ascontiguousarray(ids, np.uint32), np.ascontiguousarray(vals, np.float64)
        conn = np.ascontiguousarray(conn if conn is not None else np.zeros(0), np.int32)
        n, K = len(rec), self.max_keyframes
        assert len(ids) == len(vals)
        cand, acc = np.full((n, K), -1, np.int32), np.full((n, K), np.nan, np.float32)
        n_cand, diag = np.full(n, -9, np.int32), np.full((n, 5), -9, np.int32)
        cs, ms = np.full(len(conn), np.nan, np.float32), np.full(n, np.nan, np.float32)
        enough, n_enough, n_groups = self._outputs(n)
        vh = (voc or self.kfdb.voc).h
        args = lambda a: (self.h, vh, n, a(rec), len(ids), a(ids), a(vals), len(conn), a(conn), a(cand), a(acc), a(n_cand), a(diag), a(cs), a(ms), a(enough),   # noqa: E731
                          a(n_enough), a(n_groups))
        if not device:
            check(self.L.oslam_loopdet_detect(*args(optptr)))
        else:
            outs = (cand, acc, n_cand, diag, cs, ms, enough, n_enough, n_groups)
            with device_call([rec, ids, vals, conn] + list(outs), outputs=outs) as (addr, stream):
                check(self.L.oslam_loopdet_detect_device(*args(addr), stream))
        return dict(cand=cand, cand_acc=acc, n_cand=n_cand, diag=diag, conn_score=cs, min_score=ms, enough=enough, n_enough=n_enough, n_groups=n_groups)
