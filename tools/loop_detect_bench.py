#!/usr/bin/env python3
"""Measures the loop detector's device entry point (oslam_loopdet_detect_device, object_slam_amd/csrc/loop_detect.hip) against the same work through the
KeyFrameDatabase interface alone.

    python tools/loop_detect_bench.py [--databases 64,1024] [--reps 3]

For every number of databases B: every database replays the keyframe stream of tests/loop_detect_common.py (revisit_script: 50 keyframes over three scenes,
two of them seen again; 16 distinct seeds repeated up to B) in lockstep, as the caller of LoopClosing::DetectLoop does it: connected rows and covisibility
lists, the +10 gate, the detection, the add.  Each of the 40 keyframes that pass the gate is one timed call with B queries; the query arrays and the outputs
are resident on the device.  Two ways, host wall clock from the first launch to the end of a stream synchronisation:

  detect   one oslam_loopdet_detect_device call: the loop query with its bound derived in the kernel, then the consistency update (two launches, no host
           round trip).
  two_pass what a caller had before: oslam_kfdb_detect_loop_candidates_device for conn_score, a download, the minimum per query on the host, an upload of
           min_score into the records, the query again.  It does NOT update any consistency groups: it is the lower bound of the old path.

Prints one JSON line per size: the median over the 40 calls (and over --reps replays) of each, in microseconds.  Fails without a GPU."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--databases", default="64,1024")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("loop_detect_bench: no GPU (there is no CPU fallback to time)")
    import loop_detect_common as lc
    import voc_common as V
    from object_slam_amd import keyframe_db as kd, loop_detect as ld
    from object_slam_amd._lib import check, upload as up
    from object_slam_amd.vocabulary import Vocabulary
    voc = Vocabulary.from_arrays(*V.make_tree(5, 4, 2).arrays())
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    K = 64
    base = [lc.revisit_script(s) for s in range(16)]
    for B in [int(x) for x in args.databases.split(",")]:
        db = kd.KeyFrameDatabase(voc, B, K, 128)
        det = ld.LoopDetector(db)
        D = list(range(B))
        t_detect, t_two, n_cand, n_enough = [], [], 0, 0
        for rep in range(args.reps):
            db.clear(D)
            det.reset(D)
            for k in range(lc.N_STREAM):
                S = [base[d % 16][k] for d in D]
                rows = [(d, x, l) for d in D for x, l in S[d]["rows"]]
                det.set_connected(*ld.pack_connected([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]))
                cv = [(d, x, l) for d in D for x, l in S[d]["covis"]]
                if cv:
                    db.set_covisibility(kd.pack_covisibility([r[0] for r in cv], [r[1] for r in cv], [r[2] for r in cv]))
                if k >= 10:
                    rec, ids, vals, conn = kd.pack_queries(D, [(s["ids"], s["vals"]) for s in S], connected=[s["conn"] for s in S])
                    d_rec, d_ids, d_vals, d_conn = up(rec), up(ids), up(vals), up(conn)
                    d_cand, d_acc = up(np.full((B, K), -1, np.int32)), up(np.zeros((B, K), np.float32))
                    d_n, d_diag, d_cs, d_ms = up(np.zeros(B, np.int32)), up(np.zeros((B, 5), np.int32)), up(np.zeros(len(conn), np.float32)), up(np.zeros(B, np.float32))
                    d_en, d_ne, d_ng = up(np.full((B, K), -1, np.int32)), up(np.zeros(B, np.int32)), up(np.zeros(B, np.int32))

                    def query():
                        check(db.L.oslam_kfdb_detect_loop_candidates_device(db.h, voc.h, B, d_rec.data_ptr(), len(ids), d_ids.data_ptr(), d_vals.data_ptr(), len(conn),
                                                                            d_conn.data_ptr(), d_cand.data_ptr(), d_acc.data_ptr(), d_n.data_ptr(), d_diag.data_ptr(),
                                                                            d_cs.data_ptr(), st))

                    # the old path first: it leaves the groups alone
                    off, cnt = rec["conn_off"], rec["n_conn"]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    query()
                    cs = d_cs.cpu().numpy().view(np.float32)[:len(conn)]
                    ms = np.ones(B, np.float32)
                    has = cnt > 0
                    if has.any():   # (the queries' ranges are contiguous and in order: reduceat over the non-empty ones)
                        ms[has] = np.minimum(np.float32(1), np.minimum.reduceat(np.where(cs >= 0, cs, np.float32(1)), off[has]))
                    rec["min_score"] = ms
                    d_rec.copy_(torch.from_numpy(rec.view(np.uint8).reshape(-1)), non_blocking=False)
                    query()
                    stream.synchronize()
                    t_two.append(time.perf_counter() - t0)
                    two_n = d_n.cpu().numpy().view(np.int32)[:B].copy()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    check(det.L.oslam_loopdet_detect_device(det.h, voc.h, B, d_rec.data_ptr(), len(ids), d_ids.data_ptr(), d_vals.data_ptr(), len(conn), d_conn.data_ptr(),
                                                            d_cand.data_ptr(), d_acc.data_ptr(), d_n.data_ptr(), d_diag.data_ptr(), d_cs.data_ptr(), d_ms.data_ptr(),
                                                            d_en.data_ptr(), d_ne.data_ptr(), d_ng.data_ptr(), st))
                    stream.synchronize()
                    t_detect.append(time.perf_counter() - t0)
                    nc, ne = d_n.cpu().numpy().view(np.int32)[:B], d_ne.cpu().numpy().view(np.int32)[:B]
                    assert (nc >= 0).all() and (ne >= 0).all() and np.array_equal(nc, two_n)   # both ways found the same number of candidates
                    n_cand += int(nc.sum()); n_enough += int(ne.sum())
                db.add(*kd.pack_add(D, [k] * B, [(s["ids"], s["vals"]) for s in S]))
                db.set_covisibility(kd.pack_covisibility(D, [k] * B, [s["covis_after"][1] for s in S]))
        calls = len(t_detect)
        md, mt = float(np.median(t_detect)) * 1e6, float(np.median(t_two)) * 1e6
        print(json.dumps(dict(tool="loop_detect_bench", databases=B, keyframes_per_stream=lc.N_STREAM, max_keyframes=K, calls=calls, reps=args.reps,
                              detect_us_median=round(md, 1), detect_us_min=round(min(t_detect) * 1e6, 1), detect_us_per_query=round(md / B, 3),
                              two_pass_us_median=round(mt, 1), two_pass_us_min=round(min(t_two) * 1e6, 1), two_pass_us_per_query=round(mt / B, 3),
                              candidates_per_call=round(n_cand / calls, 1), enough_per_call=round(n_enough / calls, 1))), flush=True)
        det.close()
        db.close()


if __name__ == "__main__":
    main()
