#!/usr/bin/env python3
"""Measures the KeyFrameDatabase queries' device entry points (oslam_kfdb_detect_*_candidates_device, object_slam_amd/csrc/keyframe_db.hip).

    python tools/keyframe_db_bench.py [--databases 64,1024] [--keyframes 200] [--words 1000] [--warmup 3] [--reps 20]

For every number of databases: each database holds `keyframes` keyframes of about `words` words (+- 10 %), drawn from four scenes of 3 * words words each out of
a 1 000 000-word vocabulary, so that a query (a vector of one of the scenes) shares many words with a quarter of the keyframes and a few with the rest; every
keyframe has a covisibility list of 10.  16 distinct databases are generated and repeated up to the number asked for.  One call = one query per database =
one launch, query arrays and outputs resident on the device, timed with device events after the warm-up calls; the median over the timed calls.

Bytes moved, by the tool's own model of what one query has to read and write: the word ids of every present keyframe once (count pass, 4 B a word) with its
slot fields and chunk table row; ids and values of every scored keyframe and every connected one (score pass, 12 B a word); the query vector (12 B a word);
the covisibility rows of the kept keyframes (40 B); the outputs.  Prints one JSON line per size and query kind; no host loop is timed, so no ratio to a
CPU is claimed.  Fails without a GPU."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

VOCAB = 1000000


def make_database(rng, n_kf, words):
    scenes = [rng.choice(VOCAB, 3 * words, replace=False) for _ in range(4)]
    vecs = []
    for k in range(n_kf):
        n = int(words * rng.uniform(0.9, 1.1))
        ids = np.sort(np.concatenate([rng.choice(scenes[k % 4], n - n // 10, replace=False), rng.integers(0, VOCAB, n // 10)]))
        ids = np.unique(ids).astype(np.uint32)
        v = rng.random(len(ids)) + 0.05
        vecs.append((ids, v / v.sum()))
    covis = [rng.choice(n_kf, min(10, n_kf), replace=False).tolist() for _ in range(n_kf)]
    n = words
    q = np.unique(np.concatenate([rng.choice(scenes[1], n - n // 10, replace=False), rng.integers(0, VOCAB, n // 10)])).astype(np.uint32)
    qv = rng.random(len(q)) + 0.05
    return vecs, covis, (q, qv / qv.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--databases", default="64,1024")
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("keyframe_db_bench: no GPU (there is no CPU fallback to time)")
    import voc_common as V
    from object_slam_amd import keyframe_db as kd
    from object_slam_amd._lib import check, upload as up
    from object_slam_amd.vocabulary import Vocabulary
    voc = Vocabulary.from_arrays(*V.make_tree(5, 4, 2).arrays())
    stream = torch.cuda.current_stream()
    K, W = args.keyframes, args.words
    max_words = min(kd.MAX_WORDS, int(W * 1.1) + 1)
    rng = np.random.default_rng(12)
    base = [make_database(rng, K, W) for _ in range(16)]
    for B in [int(x) for x in args.databases.split(",")]:
        db = kd.KeyFrameDatabase(voc, B, K, max_words)
        for d0 in range(0, B, 16):   # 16 databases a call: the staging block stays small
            ds = range(d0, min(B, d0 + 16))
            db.add(*kd.pack_add([d for d in ds for _ in range(K)], [k for _ in ds for k in range(K)], [v for d in ds for v in base[d % 16][0]]))
            db.set_covisibility(kd.pack_covisibility([d for d in ds for _ in range(K)], [k for _ in ds for k in range(K)], [l for d in ds for l in base[d % 16][1]]))
        conn = [list(range(5)) for _ in range(B)]
        rec, ids, vals, cn = kd.pack_queries(np.arange(B), [base[d % 16][2] for d in range(B)], min_scores=[0.05] * B, connected=conn)
        d_rec, d_ids, d_vals, d_cn = up(rec), up(ids), up(vals), up(cn)
        d_cand, d_acc = up(np.full((B, K), -1, np.int32)), up(np.zeros((B, K), np.float32))
        d_n, d_diag, d_cs = up(np.zeros(B, np.int32)), up(np.zeros((B, 5), np.int32)), up(np.zeros(len(cn), np.float32))
        st = C.c_void_p(stream.cuda_stream)
        kf_words = np.array([sum(len(v[0]) for v in base[d % 16][0]) for d in range(B)], np.int64)
        mc = (max_words + kd.CHUNK - 1) // kd.CHUNK

        def loop():
            check(db.L.oslam_kfdb_detect_loop_candidates_device(db.h, voc.h, B, d_rec.data_ptr(), len(ids), d_ids.data_ptr(), d_vals.data_ptr(), len(cn), d_cn.data_ptr(),
                                                                d_cand.data_ptr(), d_acc.data_ptr(), d_n.data_ptr(), d_diag.data_ptr(), d_cs.data_ptr(), st))

        def reloc():
            check(db.L.oslam_kfdb_detect_relocalization_candidates_device(db.h, voc.h, B, d_rec.data_ptr(), len(ids), d_ids.data_ptr(), d_vals.data_ptr(), d_cand.data_ptr(),
                                                                          d_acc.data_ptr(), d_n.data_ptr(), d_diag.data_ptr(), st))

        for kind, launch, n_conn in (("reloc", reloc, 0), ("loop", loop, 5)):
            ms = []
            for rep in range(args.warmup + args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch()
                e1.record(stream)
                e1.synchronize()
                if rep >= args.warmup:
                    ms.append(e0.elapsed_time(e1))
            diag = d_diag.cpu().numpy().view(np.int32).reshape(B, 5)
            n_cand = d_n.cpu().numpy().view(np.int32)[:B]
            mean_words = kf_words / K
            model = (4 * kf_words + K * (8 + 4 * mc) + 12 * mean_words * (diag[:, 3] + n_conn) + 12 * rec["n_words"] + 40 * diag[:, 4] + 8 * np.maximum(n_cand, 0) + 24 + 4 * n_conn).sum()
            med = float(np.median(ms))
            print(json.dumps(dict(tool="keyframe_db_bench", query=kind, databases=B, keyframes=K, words=W, warmup=args.warmup, reps=args.reps, us_median=round(med * 1e3, 2),
                                  us_min=round(min(ms) * 1e3, 2), us_max=round(max(ms) * 1e3, 2), queries_per_s=round(B / med * 1e3, 1), us_per_query=round(med * 1e3 / B, 3),
                                  model_bytes=int(model), model_GB_per_s=round(float(model) / med / 1e6, 2), mean_n_sharing=round(float(diag[:, 0].mean()), 1),
                                  mean_nscores=round(float(diag[:, 3].mean()), 2), mean_candidates=round(float(n_cand.mean()), 2), refused=int((n_cand < 0).sum()))), flush=True)
        db.close()


if __name__ == "__main__":
    main()
