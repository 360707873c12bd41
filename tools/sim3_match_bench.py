#!/usr/bin/env python3
"""Measures SearchBySim3's batch entry point (oslam_match_search_by_sim3_batch_device, object_slam_amd/csrc/sim3_match.hip).

    python tools/sim3_match_bench.py [--pairs 64,8192] [--keypoints 1000] [--warmup 3] [--reps 20]

For every batch size: pairs of keyframes of about `keypoints` keypoints each from tests/sim3_match_common.py's generator (about 60 % of the keypoints
carry map points, fixed-scale and scaled Sim3s, th = 7.5), everything resident on the device, one call = one launch timed with device events after
the warm-up calls; the median over the timed calls.  64 distinct pairs are generated and repeated (with rows of their own) up to the batch size.
Prints one JSON line per batch size; fails without a GPU."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="64,8192")
    ap.add_argument("--keypoints", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sim3_match_bench: no GPU (there is no CPU fallback to time)")
    import sim3_match_common as smc
    from object_slam_amd import sim3_match
    from object_slam_amd._lib import check, ptr, upload as up
    from object_slam_amd.matcher import Camera
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    K = args.keypoints
    base = [smc.make_pair(900 + i, K - 40 + (i * 7) % 80, K - 40 + (i * 13) % 80, (None, 1.1, 0.9, 1.05)[i % 4]) for i in range(64)]
    rows, off1, off2, out_off, m_in = smc.concat_batch(base)
    n_base_rows, n_base_out = len(rows["has_mp"]), len(m_in)
    cam = Camera(*smc.CAM, 0.0, 0.0)
    bnd, sf = np.asarray(smc.BOUNDS, np.float32), np.ascontiguousarray(smc.SF)
    for B in [int(x) for x in args.pairs.split(",")]:
        reps = (B + 63) // 64
        pr = sim3_match.pack_pairs(*[np.tile(v, reps)[:B] for v in ([len(p["kf1"]["has_mp"]) for p in base], off1, [len(p["kf2"]["has_mp"]) for p in base], off2, [p["s12"] for p in base])],
                                   *[np.tile(np.stack([p[k] for p in base]), (reps, 1, 1))[:B] if k != "t12" else np.tile(np.stack([p[k] for p in base]), (reps, 1))[:B]
                                     for k in ("R12", "t12", "T1w", "T2w")], smc.TH, np.tile(out_off, reps)[:B])
        blk = np.arange(B) // 64   # every repetition of the 64 pairs reads rows, and writes output rows, of its own
        pr["off1"] += blk * n_base_rows; pr["off2"] += blk * n_base_rows; pr["out_off"] += blk * n_base_out
        d_rows = {k: up(np.tile(rows[k], (reps,) + (1,) * (rows[k].ndim - 1))) for k in sim3_match.ROW_KEYS}
        d_pr, d_in = up(pr), up(np.tile(m_in, reps))
        d_m = torch.full((reps * n_base_out,), -1, dtype=torch.int32, device=dev)
        d_nf = torch.zeros(B, dtype=torch.int32, device=dev)
        r = sim3_match.Rows(reps * n_base_rows, *[d_rows[k].data_ptr() for k in sim3_match.ROW_KEYS])
        matcher = sim3_match.Sim3Matcher(B, sim3_match.MAX_KEYPOINTS)

        def launch():
            check(matcher.L.oslam_match_search_by_sim3_batch_device(matcher.h, B, d_pr.data_ptr(), C.addressof(r), reps * n_base_out, d_in.data_ptr(), C.addressof(cam), ptr(bnd), ptr(sf),
                                                                    len(sf), float(smc.LOG_SF), d_m.data_ptr(), d_nf.data_ptr(), C.c_void_p(stream.cuda_stream)))

        ms = []
        for rep in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            e1.synchronize()
            if rep >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        nf = d_nf.cpu().numpy()
        med = float(np.median(ms))
        print(json.dumps(dict(tool="sim3_match_bench", pairs=B, keypoints=K, map_point_share=round(float(rows["has_mp"].mean()), 3), warmup=args.warmup, reps=args.reps,
                              us_median=round(med * 1e3, 2), us_min=round(min(ms) * 1e3, 2), us_max=round(max(ms) * 1e3, 2), pairs_per_s=round(B / med * 1e3, 1),
                              us_per_pair=round(med * 1e3 / B, 3), mean_n_found=round(float(nf.mean()), 2), refused=int((nf < 0).sum()))), flush=True)
        matcher.close()


if __name__ == "__main__":
    main()
