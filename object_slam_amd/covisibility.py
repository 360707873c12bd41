"""ctypes view of the covisibility graph (include/oslam_hip.h, "Covisibility graph"): the point-side observation lists and KeyFrame's covisibility
bookkeeping (src/KeyFrame.cc:123-208, :289-398, :553-567; src/MapPoint.cc:201-271) for many independent sequences, one graph per sequence, resident on
the device, with KeyFrame::UpdateConnections, the covisibility queries and Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1496-1604) as kernels over
it (no CPU fallback).  What keyframe_db.set_covisibility, loop_detect.set_connected and essential_graph_edges take comes from here: INTEGRATION.md.
"""
import ctypes as C

import numpy as np

from ._lib import Handle, check, device_call, lib, optptr

MAX_KEYFRAMES, MAX_OBS = 2048, 64                     # OSLAM_COVIS_MAX_KEYFRAMES, OSLAM_COVIS_MAX_OBS
PT_BAD, PT_OVERFLOW = 1, 2                            # OSLAM_COVIS_PT_*
KF_ORDERED_ALL, KF_CONNECTED, KF_IS_BAD = 1, 2, 4     # OSLAM_COVIS_KF_*
OBS_ADD, OBS_ERASE, POINT_BAD, CONN_ADD, CONN_ERASE, KF_BAD, PARENT_SET = range(7)   # OSLAM_COVIS_EV_*
REFUSED_RECORD, REFUSED_OVERFLOW, EMPTY_VOTE = -2, -3, -1

EVENT_DTYPE = np.dtype([("graph", "<i4"), ("type", "<i4"), ("a", "<i4"), ("b", "<i4"), ("c", "<i4")])                                        # oslam_covis_event_t
UPDATE_DTYPE = np.dtype([("graph", "<i4"), ("keyframe", "<i4"), ("pts_off", "<i4"), ("n_pts", "<i4"), ("excl_off", "<i4"), ("n_excl", "<i4")])   # oslam_covis_update_t
QUERY_DTYPE = np.dtype([("graph", "<i4"), ("keyframe", "<i4"), ("max_n", "<i4"), ("min_w", "<i4")])                                          # oslam_covis_query_t
KEY_DTYPE = np.dtype([("graph", "<i4"), ("keyframe", "<i4")])                                                                                # oslam_covis_key_t
LOCAL_DTYPE = np.dtype([("graph", "<i4"), ("pts_off", "<i4"), ("n_pts", "<i4")])                                                             # oslam_covis_local_t


def _struct(dtype):
    return type("S", (C.Structure,), {"_fields_": [(n, C.c_int32) for n in dtype.names]})


Event, Update, Query, Key, Local = (_struct(d) for d in (EVENT_DTYPE, UPDATE_DTYPE, QUERY_DTYPE, KEY_DTYPE, LOCAL_DTYPE))


def _bind(L):
    if getattr(L, "_oslam_covis_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int
    L.oslam_covis_create.argtypes = [C.POINTER(vp), i32, i32, i32, i32, i32]
    L.oslam_covis_destroy.argtypes = [vp]
    L.oslam_covis_destroy.restype = None
    L.oslam_covis_reset.argtypes = [vp, i32, vp]
    L.oslam_covis_apply.argtypes = [vp, i32, vp, vp]
    L.oslam_covis_apply_device.argtypes = [vp, i32, vp, vp, vp]
    L.oslam_covis_update_connections.argtypes = [vp, i32, vp, i32, vp, i32, vp] + [vp] * 7
    L.oslam_covis_update_connections_device.argtypes = [vp, i32, vp, i32, vp, i32, vp] + [vp] * 8
    L.oslam_covis_covisibles.argtypes = [vp, i32, vp, vp, vp, vp]
    L.oslam_covis_covisibles_device.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.oslam_covis_connected_rows.argtypes = [vp, i32, vp, vp]
    L.oslam_covis_connected_rows_device.argtypes = [vp, i32, vp, vp, vp]
    L.oslam_covis_local_keyframes.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp]
    L.oslam_covis_local_keyframes_device.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    L.oslam_covis_get_state.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp]
    L._oslam_covis_bound = True
    return L


def _flat(lists):
    cnt = np.array([len(l) for l in lists], np.int32)
    off = (np.concatenate([[0], np.cumsum(cnt)[:-1]]) if len(cnt) else np.zeros(0)).astype(np.int32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(l, np.int32).reshape(-1) for l in lists] + [np.zeros(0, np.int32)]))
    return off, cnt, flat


def pack_events(events):
    """EVENT_DTYPE records of [(graph, type, a[, b[, c]])], in the order given."""
    rec = np.zeros(len(events), EVENT_DTYPE)
    for i, e in enumerate(events):
        rec[i] = tuple(e) + (0,) * (5 - len(e))
    return rec


def pack_updates(graphs, keyframes, points, exclude=None):
    """(UPDATE_DTYPE records, points, exclude): points[i] = mvpMapPoints of keyframes[i] of graphs[i] as point ids (-1: empty slot), exclude[i] = the
    keyframe ids left out of its new_links."""
    rec = np.zeros(len(points), UPDATE_DTYPE)
    rec["graph"], rec["keyframe"] = np.asarray(graphs, np.int32), np.asarray(keyframes, np.int32)
    rec["pts_off"], rec["n_pts"], pts = _flat(points)
    rec["excl_off"], rec["n_excl"], excl = _flat(exclude if exclude is not None else [[]] * len(points))
    return rec, pts, excl


def pack_queries(graphs, keyframes, max_n, min_w=0):
    """QUERY_DTYPE records; max_n and min_w are broadcast."""
    rec = np.zeros(len(graphs), QUERY_DTYPE)
    rec["graph"], rec["keyframe"], rec["max_n"], rec["min_w"] = np.asarray(graphs, np.int32), np.asarray(keyframes, np.int32), max_n, min_w
    return rec


def pack_keys(graphs, keyframes):
    rec = np.zeros(len(graphs), KEY_DTYPE)
    rec["graph"], rec["keyframe"] = np.asarray(graphs, np.int32), np.asarray(keyframes, np.int32)
    return rec


def pack_local(graphs, points):
    """(LOCAL_DTYPE records, points): points[i] = mCurrentFrame.mvpMapPoints of the frame of graphs[i] as point ids (-1: NULL)."""
    rec = np.zeros(len(points), LOCAL_DTYPE)
    rec["graph"] = np.asarray(graphs, np.int32)
    rec["pts_off"], rec["n_pts"], pts = _flat(points)
    return rec, pts


class CovisibilityGraph(Handle):
    """n_graphs graphs of up to max_keyframes (<= 2048) keyframes and max_points point slots with observation lists of up to obs_cap (<= 64) entries."""

    def __init__(self, n_graphs, max_keyframes, max_points, obs_cap=16, device=0):
        super().__init__(_bind(lib()), "oslam_covis", n_graphs, max_keyframes, max_points, obs_cap, device)
        self.n_graphs, self.max_keyframes, self.max_points, self.obs_cap = n_graphs, max_keyframes, max_points, obs_cap
        self.words = (max_keyframes + 31) // 32

    @staticmethod
    def bytes_per_graph(max_keyframes, max_points, obs_cap):
        return 8 * max_points * obs_cap + 4 * max_points + 4 * max_keyframes * max_keyframes + 8 * max_keyframes

    def reset(self, graphs):
        g = np.ascontiguousarray(np.atleast_1d(graphs), np.int32)
        check(self.L.oslam_covis_reset(self.h, len(g), optptr(g)))

    def apply(self, events, device=False):
        """The events (pack_events) of each graph in record order.  Returns n_overflow [n_graphs]."""
        ev = np.ascontiguousarray(events, EVENT_DTYPE)
        nov = np.full(self.n_graphs, -9, np.int32)
        if not device:
            check(self.L.oslam_covis_apply(self.h, len(ev), optptr(ev), optptr(nov)))
        else:
            with device_call([ev, nov], outputs=(nov,)) as (addr, stream):
                check(self.L.oslam_covis_apply_device(self.h, len(ev), addr(ev), addr(nov), stream))
        return nov

    def update_connections(self, rec, points, exclude=None, device=False):
        """KeyFrame::UpdateConnections of every record (pack_updates), the records of one graph in record order.  Returns dict(status [n], ordered_ids and
        ordered_w [n, max_keyframes] with n_ordered [n], parent [n], new_links [n, max_keyframes] with n_new_links [n])."""
        rec, points = np.ascontiguousarray(rec, UPDATE_DTYPE), np.ascontiguousarray(points, np.int32)
        excl = np.ascontiguousarray(exclude if exclude is not None else np.zeros(0), np.int32)
        n, K = len(rec), self.max_keyframes
        # fills no result has: what a record does not write stays visible
        st, no, pa, nl = (np.full(n, -9, np.int32) for _ in range(4))
        oi, ow, li = (np.full((n, K), -1, np.int32) for _ in range(3))
        args = lambda a: (self.h, n, a(rec), len(points), a(points), len(excl), a(excl), a(st), a(oi), a(ow), a(no), a(pa), a(li), a(nl))   # noqa: E731
        if not device:
            check(self.L.oslam_covis_update_connections(*args(optptr)))
        else:
            outs = (st, oi, ow, no, pa, li, nl)
            with device_call([rec, points, excl] + list(outs), outputs=outs) as (addr, stream):
                check(self.L.oslam_covis_update_connections_device(*args(addr), stream))
        return dict(status=st, ordered_ids=oi, ordered_w=ow, n_ordered=no, parent=pa, new_links=li, n_new_links=nl)

    def covisibles(self, rec, device=False):
        """The ordered list of every record (pack_queries).  Returns dict(ids, weights [n, max_keyframes], n [n])."""
        rec = np.ascontiguousarray(rec, QUERY_DTYPE)
        n, K = len(rec), self.max_keyframes
        ids, w, cnt = np.full((n, K), -1, np.int32), np.full((n, K), -1, np.int32), np.full(n, -9, np.int32)
        if not device:
            check(self.L.oslam_covis_covisibles(self.h, n, optptr(rec), optptr(ids), optptr(w), optptr(cnt)))
        else:
            with device_call([rec, ids, w, cnt], outputs=(ids, w, cnt)) as (addr, stream):
                check(self.L.oslam_covis_covisibles_device(self.h, n, addr(rec), addr(ids), addr(w), addr(cnt), stream))
        return dict(ids=ids, weights=w, n=cnt)

    def connected_rows(self, rec, device=False):
        """GetConnectedKeyFrames() of every record (pack_keys) as bitset rows [n, words] (loop_detect.bits_to_ids reads one)."""
        rec = np.ascontiguousarray(rec, KEY_DTYPE)
        bits = np.zeros((len(rec), self.words), np.uint32)
        if not device:
            check(self.L.oslam_covis_connected_rows(self.h, len(rec), optptr(rec), optptr(bits)))
        else:
            with device_call([rec, bits], outputs=(bits,)) as (addr, stream):
                check(self.L.oslam_covis_connected_rows_device(self.h, len(rec), addr(rec), addr(bits), stream))
        return bits

    def local_keyframes(self, rec, points, device=False):
        """Tracking::UpdateLocalKeyFrames of every record (pack_local).  Returns dict(list [n, max_keyframes], n_list [n] (-1: empty vote, -3: overflow),
        ref_kf [n], null [len(points)] uint8)."""
        rec, points = np.ascontiguousarray(rec, LOCAL_DTYPE), np.ascontiguousarray(points, np.int32)
        n, K = len(rec), self.max_keyframes
        lst, nl, ref, null = np.full((n, K), -1, np.int32), np.full(n, -9, np.int32), np.full(n, -9, np.int32), np.full(len(points), 9, np.uint8)
        args = lambda a: (self.h, n, a(rec), len(points), a(points), a(lst), a(nl), a(ref), a(null))   # noqa: E731
        if not device:
            check(self.L.oslam_covis_local_keyframes(*args(optptr)))
        else:
            outs = (lst, nl, ref, null)
            with device_call([rec, points] + list(outs), outputs=outs) as (addr, stream):
                check(self.L.oslam_covis_local_keyframes_device(*args(addr), stream))
        return dict(list=lst, n_list=nl, ref_kf=ref, null=null)

    def get_state(self, graph, points=(), weights=True):
        """A readback of one graph: dict(weights [K, K] (None if not asked for), parents [K], kf_flags [K], observations {point: [(keyframe, index)]},
        point_flags {point: PT_*})."""
        K, Cc = self.max_keyframes, self.obs_cap
        pts = np.ascontiguousarray(points, np.int32)
        w = np.zeros((K, K), np.int32) if weights else None
        pa, kf = np.zeros(K, np.int32), np.zeros(K, np.uint32)
        obs, cnt, fl = np.zeros((len(pts), Cc, 2), np.int32), np.zeros(len(pts), np.int32), np.zeros(len(pts), np.uint32)
        check(self.L.oslam_covis_get_state(self.h, int(graph), optptr(w), optptr(pa), optptr(kf), len(pts), optptr(pts), optptr(obs), optptr(cnt), optptr(fl)))
        return dict(weights=w, parents=pa, kf_flags=kf, observations={int(p): [tuple(e) for e in obs[i, :cnt[i]].tolist()] for i, p in enumerate(pts)},
                    point_flags={int(p): int(fl[i]) for i, p in enumerate(pts)})
