"""ctypes view of the KeyFrameDatabase operator (include/oslam_hip.h, "KeyFrameDatabase"): ORB_SLAM2::KeyFrameDatabase (src/KeyFrameDatabase.cc) for many
independent databases, one per sequence, resident on the device.  The query Tracking::Relocalization (src/Tracking.cc:1616) and LoopClosing::DetectLoop
(src/LoopClosing.cc:143) begin with.

`KeyFrameDatabase.detect_loop_candidates` / `detect_relocalization_candidates` are one launch of the gfx950 kernel over all queries of a call (no CPU
fallback: creating a KeyFrameDatabase fails without a device).  BowVectors are (ids uint32 ascending, vals float64) pairs as Vocabulary.vectors returns
them; the `pack_*` helpers build the records and the flat arrays.
"""
import ctypes as C

import numpy as np

from ._lib import Handle, check, device_call, lib, optptr

COVIS = 10             # OSLAM_KFDB_COVIS
CHUNK = 128            # OSLAM_KFDB_CHUNK
MAX_KEYFRAMES = 2048   # OSLAM_KFDB_MAX_KEYFRAMES
MAX_WORDS = 2400       # OSLAM_KFDB_MAX_WORDS

ADD_DTYPE = np.dtype([("database", "<i4"), ("keyframe", "<i4"), ("word_off", "<i4"), ("n_words", "<i4")])                    # oslam_kfdb_add_t
KEY_DTYPE = np.dtype([("database", "<i4"), ("keyframe", "<i4")])                                                             # oslam_kfdb_key_t
COVIS_DTYPE = np.dtype([("database", "<i4"), ("keyframe", "<i4"), ("n", "<i4"), ("ids", "<i4", (COVIS,))])                   # oslam_kfdb_covis_t
QUERY_DTYPE = np.dtype([("database", "<i4"), ("query_id", "<i4"), ("word_off", "<i4"), ("n_words", "<i4"), ("conn_off", "<i4"), ("n_conn", "<i4"),
                        ("min_score", "<f4"), ("reserved", "<i4")])                                                          # oslam_kfdb_query_t
DIAG = ("n_sharing", "maxCommonWords", "minCommonWords", "nscores", "n_kept")


def _bind(L):
    if getattr(L, "_oslam_kfdb_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int
    L.oslam_kfdb_create.argtypes = [C.POINTER(vp), i32, i32, i32, C.c_longlong, i32]
    L.oslam_kfdb_destroy.argtypes = [vp]
    L.oslam_kfdb_destroy.restype = None
    L.oslam_kfdb_info.argtypes = [vp, vp]
    L.oslam_kfdb_add.argtypes = [vp, i32, vp, i32, vp, vp]
    L.oslam_kfdb_erase.argtypes = [vp, i32, vp]
    L.oslam_kfdb_clear.argtypes = [vp, i32, vp]
    L.oslam_kfdb_set_covisibility.argtypes = [vp, i32, vp]
    L.oslam_kfdb_detect_loop_candidates.argtypes = [vp, vp, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.oslam_kfdb_detect_relocalization_candidates.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    L.oslam_kfdb_detect_loop_candidates_device.argtypes = [vp, vp, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.oslam_kfdb_detect_relocalization_candidates_device.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L._oslam_kfdb_bound = True
    return L


def _csr(vectors):
    """[(ids, vals), ...] -> (off [n], cnt [n], ids flat uint32, vals flat float64)"""
    cnt = np.array([len(v[0]) for v in vectors], np.int32)
    off = (np.concatenate([[0], np.cumsum(cnt)[:-1]]) if len(cnt) else np.zeros(0)).astype(np.int32)
    ids = np.concatenate([np.asarray(v[0], np.uint32).reshape(-1) for v in vectors] + [np.zeros(0, np.uint32)])
    vals = np.concatenate([np.asarray(v[1], np.float64).reshape(-1) for v in vectors] + [np.zeros(0, np.float64)])
    assert len(ids) == len(vals)
    return off, cnt, np.ascontiguousarray(ids), np.ascontiguousarray(vals)


def pack_add(databases, keyframes, vectors):
    """(ADD_DTYPE records, ids, vals) of keyframes[i] of databases[i] with BowVector vectors[i] = (ids, vals)."""
    rec = np.zeros(len(vectors), ADD_DTYPE)
    rec["database"], rec["keyframe"] = np.asarray(databases, np.int32), np.asarray(keyframes, np.int32)
    rec["word_off"], rec["n_words"], ids, vals = _csr(vectors)
    return rec, ids, vals


def pack_keys(databases, keyframes):
    rec = np.zeros(len(np.atleast_1d(databases)), KEY_DTYPE)
    rec["database"], rec["keyframe"] = np.asarray(databases, np.int32), np.asarray(keyframes, np.int32)
    return rec


def pack_covisibility(databases, keyframes, lists):
    """COVIS_DTYPE records: lists[i] = the at most 10 ids GetBestCovisibilityKeyFrames(10) returns for keyframes[i], in its order."""
    rec = np.zeros(len(lists), COVIS_DTYPE)
    rec["database"], rec["keyframe"] = np.asarray(databases, np.int32), np.asarray(keyframes, np.int32)
    rec["ids"] = -1
    for i, l in enumerate(lists):
        assert len(l) <= COVIS, "at most %d covisible keyframes" % COVIS
        rec["n"][i] = len(l)
        rec["ids"][i, :len(l)] = np.asarray(l, np.int32)
    return rec


def pack_queries(databases, vectors, query_ids=None, min_scores=None, connected=None):
    """(QUERY_DTYPE records, ids, vals, conn) of one query per entry: vectors[i] = the query's BowVector; for loop queries min_scores[i] and
    connected[i] = the ids of pKF->GetConnectedKeyFrames()."""
    n = len(vectors)
    rec = np.zeros(n, QUERY_DTYPE)
    rec["database"] = np.asarray(databases, np.int32)
    rec["query_id"] = np.arange(n) if query_ids is None else np.asarray(query_ids, np.int32)
    rec["word_off"], rec["n_words"], ids, vals = _csr(vectors)
    conn = np.zeros(0, np.int32)
    if connected is not None:
        cnt = np.array([len(c) for c in connected], np.int32)
        rec["n_conn"] = cnt
        rec["conn_off"] = np.concatenate([[0], np.cumsum(cnt)[:-1]]) if n else 0
        conn = np.ascontiguousarray(np.concatenate([np.asarray(c, np.int32).reshape(-1) for c in connected] + [np.zeros(0, np.int32)]))
    if min_scores is not None:
        rec["min_score"] = np.asarray(min_scores, np.float32)
    return rec, ids, vals, conn


class KeyFrameDatabase(Handle):
    """n_databases databases of up to max_keyframes (<= 2048) keyframes with up to max_words (<= 2400) words each; pool_words words of storage shared by all
    of them, in chunks of 128.  `voc` (a Vocabulary) must be L1_NORM: the queries refuse any other."""

    def __init__(self, voc, n_databases, max_keyframes, max_words=MAX_WORDS, pool_words=None, device=0):
        if pool_words is None:
            pool_words = n_databases * max_keyframes * ((max_words + CHUNK - 1) // CHUNK) * CHUNK
        super().__init__(_bind(lib()), "oslam_kfdb", n_databases, max_keyframes, max_words, int(pool_words), device)
        self.voc, self.n_databases, self.max_keyframes, self.max_words = voc, n_databases, max_keyframes, max_words

    @property
    def info(self):
        out = np.zeros(3, np.int64)
        check(self.L.oslam_kfdb_info(self.h, optptr(out)))
        return dict(free_chunks=int(out[0]), chunks=int(out[1]), present=int(out[2]))

    def add(self, rec, ids, vals):
        """KeyFrameDatabase::add of every record (pack_add)."""
        rec, ids, vals = np.ascontiguousarray(rec, ADD_DTYPE), np.ascontiguousarray(ids, np.uint32), np.ascontiguousarray(vals, np.float64)
        assert len(ids) == len(vals)
        check(self.L.oslam_kfdb_add(self.h, len(rec), optptr(rec), len(ids), optptr(ids), optptr(vals)))

    def erase(self, rec):
        rec = np.ascontiguousarray(rec, KEY_DTYPE)
        check(self.L.oslam_kfdb_erase(self.h, len(rec), optptr(rec)))

    def clear(self, databases):
        d = np.ascontiguousarray(np.atleast_1d(databases), np.int32)
        check(self.L.oslam_kfdb_clear(self.h, len(d), optptr(d)))

    def set_covisibility(self, rec):
        rec = np.ascontiguousarray(rec, COVIS_DTYPE)
        check(self.L.oslam_kfdb_set_covisibility(self.h, len(rec), optptr(rec)))

    def _query(self, loop, rec, ids, vals, conn, device, voc):
        rec, ids, vals = np.ascontiguousarray(rec, QUERY_DTYPE), np.ascontiguousarray(ids, np.uint32), np.ascontiguousarray(vals, np.float64)
        conn = np.ascontiguousarray(conn if conn is not None else np.zeros(0), np.int32)
        n, K = len(rec), self.max_keyframes
        assert len(ids) == len(vals)
        # fills no result has: what a query does not write stays visible
        cand, acc = np.full((n, K), -1, np.int32), np.full((n, K), np.nan, np.float32)
        n_cand, diag = np.full(n, -9, np.int32), np.full((n, 5), -9, np.int32)
        cs = np.full(len(conn), np.nan, np.float32)
        vh = (voc or self.voc).h
        if loop:
            name = "oslam_kfdb_detect_loop_candidates"
            args = lambda a: (self.h, vh, n, a(rec), len(ids), a(ids), a(vals), len(conn), a(conn), a(cand), a(acc), a(n_cand), a(diag), a(cs))   # noqa: E731
        else:
            name = "oslam_kfdb_detect_relocalization_candidates"
            args = lambda a: (self.h, vh, n, a(rec), len(ids), a(ids), a(vals), a(cand), a(acc), a(n_cand), a(diag))   # noqa: E731
        if not device:
            check(getattr(self.L, name)(*args(optptr)))
        else:
            with device_call([rec, ids, vals, conn, cand, acc, n_cand, diag, cs], outputs=(cand, acc, n_cand, diag, cs)) as (addr, stream):
                check(getattr(self.L, name + "_device")(*args(addr), stream))
        out = dict(cand=cand, cand_acc=acc, n_cand=n_cand, diag=diag)
        if loop:
            out["conn_score"] = cs
        return out

    def detect_loop_candidates(self, rec, ids, vals, conn, device=False, voc=None):
        """DetectLoopCandidates of every query (pack_queries with min_scores and connected).  Returns dict(cand [n, max_keyframes] int32: row q holds
        n_cand[q] candidate ids in the reference's order, cand_acc their accumulated scores, n_cand [n], diag [n, 5] (DIAG), conn_score [len(conn)]).
        device=True goes through the _device entry point on a side stream, over torch tensors."""
        return self._query(True, rec, ids, vals, conn, device, voc)

    def detect_relocalization_candidates(self, rec, ids, vals, device=False, voc=None):
        """DetectRelocalizationCandidates of every query; rewrites the reloc_score of every keyframe it scores."""
        return self._query(False, rec, ids, vals, None, device, voc)
