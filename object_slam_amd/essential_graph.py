"""ctypes view of OptimizeEssentialGraph (include/oslam_hip.h, "OptimizeEssentialGraph"): Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:781-1044),
the pose graph LoopClosing::CorrectLoop optimises over every keyframe of the map (src/LoopClosing.cc:568), for batches of independent graphs, its point
correction, and the reference's edge selection over flat views (host arithmetic, no GPU part).

`EssentialGraphOptimizer.optimize_batch` is one launch of the gfx950 kernel over all graphs (no CPU fallback: creating the handle fails without a
device).  The driver does not close loops and calls none of this.
"""
import ctypes as C

import numpy as np

from ._lib import Handle, check, device_call, lib, optptr

TRACE_ROWS = 200       # OSLAM_ESSENTIAL_GRAPH_TRACE_ROWS
MIN_FEAT = 100         # const int minFeat = 100 (src/Optimizer.cc:806)
KIND_LOOP, KIND_NORMAL = 0, 1


class Problem(C.Structure):      # oslam_essential_graph_problem_t
    _fields_ = [("n_kf", C.c_int32), ("kf_offset", C.c_int32), ("n_edges", C.c_int32), ("edge_offset", C.c_int32), ("fix_scale", C.c_int32), ("env_offset", C.c_int32),
                ("env_blocks", C.c_int32), ("reserved", C.c_int32)]


PROBLEM_DTYPE = np.dtype([("n_kf", "<i4"), ("kf_offset", "<i4"), ("n_edges", "<i4"), ("edge_offset", "<i4"), ("fix_scale", "<i4"), ("env_offset", "<i4"), ("env_blocks", "<i4"),
                          ("reserved", "<i4")])


def _bind(L):
    if getattr(L, "_oslam_essential_graph_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int
    L.oslam_essential_graph_create.argtypes = [C.POINTER(vp), i32, i32, i32, C.c_longlong, i32]
    L.oslam_essential_graph_destroy.argtypes = [vp]
    L.oslam_essential_graph_destroy.restype = None
    L.oslam_optimize_essential_graph_batch.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.oslam_optimize_essential_graph_batch_device.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.oslam_essential_graph_correct_points.argtypes = [vp, i32, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp]
    L.oslam_essential_graph_correct_points_device.argtypes = [vp, i32, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L._oslam_essential_graph_bound = True
    return L


def pack_problems(n_kf, n_edges, fix_scale, kf_offsets=None, edge_offsets=None):
    """PROBLEM_DTYPE records of problems with n_kf keyframes and n_edges edges each; the offsets default to consecutive rows.  env_offset / env_blocks stay 0:
    `envelope` fills them in for the device entry point, the host entry point computes them itself."""
    n_kf, n_edges = np.asarray(n_kf, np.int32).reshape(-1), np.asarray(n_edges, np.int32).reshape(-1)
    n = len(n_kf)
    pr = np.zeros(n, PROBLEM_DTYPE)
    consecutive = lambda c: np.concatenate([[0], np.cumsum(np.maximum(c, 0))[:-1]]) if n else 0
    pr["n_kf"], pr["n_edges"] = n_kf, n_edges
    pr["kf_offset"] = consecutive(n_kf) if kf_offsets is None else np.asarray(kf_offsets, np.int32)
    pr["edge_offset"] = consecutive(n_edges) if edge_offsets is None else np.asarray(edge_offsets, np.int32)
    pr["fix_scale"] = np.asarray(fix_scale, np.int32)
    return pr


def envelope(problems, fixed, edges):
    """The block envelope of every problem: (row_first [n_kf_total] int32, env_blocks [n] int64).  row_first[k] is the smallest index m <= k (inside the
    problem) of a keyframe an edge joins to k, k itself without one; the block row of a free keyframe runs from the first free keyframe at or after
    row_first[k] to its diagonal, and env_blocks counts those 7 x 7 blocks.  Problems that do not lie inside the arrays, and edges with an index
    outside their problem, are passed over (the operator reports them)."""
    problems = np.asarray(problems, PROBLEM_DTYPE)
    fixed = np.asarray(fixed, np.uint8).reshape(-1)
    edges = np.asarray(edges, np.int32).reshape(-1, 3)
    row_first = np.zeros(len(fixed), np.int32)
    blocks = np.zeros(len(problems), np.int64)
    for b, p in enumerate(problems):
        n, o, ne, eo = int(p["n_kf"]), int(p["kf_offset"]), int(p["n_edges"]), int(p["edge_offset"])
        if n < 0 or o < 0 or o + n > len(fixed) or ne < 0 or eo < 0 or eo + ne > len(edges):
            continue
        rf = np.arange(n, dtype=np.int64)
        e = edges[eo:eo + ne, :2].astype(np.int64)
        e = e[((e >= 0) & (e < n)).all(1)]
        if len(e):
            np.minimum.at(rf, e.max(1), e.min(1))
        free = fixed[o:o + n] == 0
        fidx = np.cumsum(free) - free   # free keyframes before k
        blocks[b] = int((fidx[free] - fidx[rf[free]] + 1).sum())
        row_first[o:o + n] = rf
    return row_first, blocks


def with_envelope(problems, fixed, edges):
    """problems with env_offset / env_blocks filled in consecutively, and row_first: what the device entry point takes"""
    pr = np.array(problems, PROBLEM_DTYPE)
    row_first, blocks = envelope(pr, fixed, edges)
    pr["env_blocks"] = blocks
    pr["env_offset"] = np.concatenate([[0], np.cumsum(blocks)[:-1]]) if len(pr) else 0
    return pr, row_first


def essential_graph_edges(parent, children, loop_edges, covisibles, loop_connections, cur, loop, weight=None):
    """The edge list of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:847-983) as [(i, j, kind)] int32 in the reference's order: i is setVertex(0), j
    setVertex(1), kind 0 a new loop connection, 1 a spanning-tree, old-loop or covisibility edge.  Keyframes are the indices 0 .. n - 1 of the good
    keyframes in ascending mnId.
      parent[k]            index of GetParent(), -1 without one
      children[k]          the indices hasChild() answers true for
      loop_edges[k]        GetLoopEdges()
      covisibles[k]        GetCovisiblesByWeight(100), in the order it returns them (bad keyframes already left out)
      loop_connections     {k: connections}, the LoopConnections map
      weight(k, m)         GetWeight (only asked for loop connections); None = every weight is below 100
      cur, loop            pCurKF, pLoopKF
    Normalisation: the reference walks std::map<KeyFrame*, ...> and std::set<KeyFrame*> in pointer order; here both run in ascending keyframe index."""
    out = []
    inserted = set()
    for i in sorted(loop_connections):
        for j in sorted(set(loop_connections[i])):
            if (i != cur or j != loop) and (0 if weight is None else weight(i, j)) < MIN_FEAT:   # :863
                continue
            out.append((i, j, KIND_LOOP))
            inserted.add((min(i, j), max(i, j)))
    for i in range(len(parent)):
        p = int(parent[i])
        if p >= 0:
            out.append((i, p, KIND_NORMAL))
        le = set(int(v) for v in loop_edges[i])
        for l in sorted(le):
            if l < i:
                out.append((i, l, KIND_NORMAL))
        ch = set(int(v) for v in children[i])
        for n in covisibles[i]:
            n = int(n)
            if n != p and n not in ch and n not in le and n < i:
                if (min(i, n), max(i, n)) in inserted:
                    continue
                out.append((i, n, KIND_NORMAL))
    return np.array(out, np.int32).reshape(-1, 3)


class EssentialGraphOptimizer(Handle):
    """A handle for up to max_problems graphs with max_keyframes keyframes, max_edges edges and max_envelope_blocks 7 x 7 blocks of envelope in all."""

    def __init__(self, max_problems=256, max_keyframes=1 << 14, max_edges=1 << 17, max_envelope_blocks=1 << 18, device=0):
        super().__init__(_bind(lib()), "oslam_essential_graph", max_problems, max_keyframes, max_edges, max_envelope_blocks, device)

    def optimize_batch(self, problems, Scw, Snc, has_noncorrected, fixed, edges, Scw_out=None, Tcw_out=None, status=None, trace=False, device=False, row_first=None):
        """OptimizeEssentialGraph of every problem.  problems: PROBLEM_DTYPE array (pack_problems); Scw, Snc [N, 13] float32 = s, R row-major, t;
        has_noncorrected, fixed [N] uint8; edges [E, 3] int32 = i, j, kind.  Returns dict(Scw [N, 13] float64 = R row-major, t, s; Tcw [N, 4, 4] float32;
        status [n, 4] int32 = 0 / -1 / -2, n_free, n_edges, 256 * LM iterations + LM trials[, trace [n, 200, 6] float64, trace_n [n] int32]).  Output arrays
        given by the caller are written in place: what the call does not write keeps what it held.  device=True goes through
        oslam_optimize_essential_graph_batch_device on a side stream, over torch tensors, with the envelope of `with_envelope` (or the problems and row_first
        as given, when row_first is not None)."""
        problems = np.ascontiguousarray(problems, PROBLEM_DTYPE)
        Scw, Snc = np.ascontiguousarray(Scw, np.float32).reshape(-1, 13), np.ascontiguousarray(Snc, np.float32).reshape(-1, 13)
        has_noncorrected, fixed = np.ascontiguousarray(has_noncorrected, np.uint8).reshape(-1), np.ascontiguousarray(fixed, np.uint8).reshape(-1)
        edges = np.ascontiguousarray(edges, np.int32).reshape(-1, 3)
        n, N, E = len(problems), len(Scw), len(edges)
        assert len(Snc) == N and len(has_noncorrected) == N and len(fixed) == N
        Scw_out = np.zeros((N, 13), np.float64) if Scw_out is None else Scw_out
        Tcw_out = np.zeros((N, 4, 4), np.float32) if Tcw_out is None else Tcw_out
        status = np.zeros((n, 4), np.int32) if status is None else status
        assert Scw_out.dtype == np.float64 and Scw_out.size == 13 * N and Scw_out.flags.c_contiguous and Tcw_out.dtype == np.float32 and Tcw_out.size == 16 * N and Tcw_out.flags.c_contiguous
        assert status.dtype == np.int32 and status.size == 4 * n and status.flags.c_contiguous
        tr = np.zeros((n, TRACE_ROWS, 6), np.float64) if trace else None
        tn = np.zeros(n, np.int32) if trace else None
        if not device:
            check(self.L.oslam_optimize_essential_graph_batch(self.h, n, optptr(problems), N, optptr(Scw), optptr(Snc), optptr(has_noncorrected), optptr(fixed), E, optptr(edges),
                                                              optptr(Scw_out), optptr(Tcw_out), optptr(status), optptr(tr), optptr(tn)))
        else:
            if row_first is None:
                problems, row_first = with_envelope(problems, fixed, edges)
            row_first = np.ascontiguousarray(row_first, np.int32)
            with device_call((problems, Scw, Snc, has_noncorrected, fixed, row_first, edges, Scw_out, Tcw_out, status, tr, tn), outputs=(Scw_out, Tcw_out, status, tr, tn)) as (a, stream):
                check(self.L.oslam_optimize_essential_graph_batch_device(self.h, n, a(problems), N, a(Scw), a(Snc), a(has_noncorrected), a(fixed), a(row_first), E, a(edges),
                                                                         a(Scw_out), a(Tcw_out), a(status), a(tr), a(tn), stream))
        out = dict(Scw=Scw_out.reshape(N, 13), Tcw=Tcw_out.reshape(N, 4, 4), status=status.reshape(n, 4))
        if trace:
            out["trace"], out["trace_n"] = tr, tn
        return out

    def correct_points(self, problems, Scw, Scw_out, status, point_problem, ref, P, P_out=None, device=False):
        """P' = Scw_out[r].inverse().map(Scw[r].map(P)) per point (src/Optimizer.cc:1013-1043); point_problem, ref [M] int32, P [M, 3] float32.  A point with
        ref < 0, or of a problem whose status[0] is not 0, keeps the bytes of P_out.  Returns P_out [M, 3] float32."""
        problems = np.ascontiguousarray(problems, PROBLEM_DTYPE)
        Scw = np.ascontiguousarray(Scw, np.float32).reshape(-1, 13)
        Scw_out = np.ascontiguousarray(Scw_out, np.float64).reshape(-1, 13)
        status = np.ascontiguousarray(status, np.int32).reshape(-1, 4)
        point_problem, ref = np.ascontiguousarray(point_problem, np.int32).reshape(-1), np.ascontiguousarray(ref, np.int32).reshape(-1)
        P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
        n, N, M = len(problems), len(Scw), len(P)
        assert len(Scw_out) == N and len(status) == n and len(point_problem) == M and len(ref) == M
        P_out = np.zeros((M, 3), np.float32) if P_out is None else P_out
        assert P_out.dtype == np.float32 and P_out.size == 3 * M and P_out.flags.c_contiguous
        if not device:
            check(self.L.oslam_essential_graph_correct_points(self.h, n, optptr(problems), N, optptr(Scw), optptr(Scw_out), optptr(status), M, optptr(point_problem), optptr(ref),
                                                              optptr(P), optptr(P_out)))
        else:
            with device_call((problems, Scw, Scw_out, status, point_problem, ref, P, P_out), outputs=(P_out,)) as (a, stream):
                check(self.L.oslam_essential_graph_correct_points_device(self.h, n, a(problems), N, a(Scw), a(Scw_out), a(status), M, a(point_problem), a(ref), a(P), a(P_out), stream))
        return P_out.reshape(M, 3)


def optimize_batch(problems, Scw, Snc, has_noncorrected, fixed, edges, **kw):
    pr, _ = with_envelope(np.asarray(problems, PROBLEM_DTYPE), fixed, edges)
    h = EssentialGraphOptimizer(max(1, len(pr)), max(1, len(np.asarray(fixed).reshape(-1))), max(1, len(np.asarray(edges).reshape(-1, 3))), max(1, int(pr["env_blocks"].sum())))
    try:
        return h.optimize_batch(problems, Scw, Snc, has_noncorrected, fixed, edges, **kw)
    finally:
        h.close()
