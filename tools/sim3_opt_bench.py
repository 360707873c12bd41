#!/usr/bin/env python3
"""Measures OptimizeSim3's batch entry point (oslam_optimize_sim3_batch_device, object_slam_amd/csrc/sim3_opt.hip).

    python tools/sim3_opt_bench.py [--problems 4096] [--correspondences 100,300] [--warmup 3] [--reps 20]

For every correspondence count: `problems` problems from tests/sim3_opt_common.py's generator (10 % gross outliers, alternately a fixed and a free scale,
the start a few degrees / percent off the truth, th2 = 10), everything resident on the device, one call = one launch timed with device events after the
warm-up calls; the median over the timed calls.  64 distinct problems are generated and repeated (with rows of their own) up to the batch size.
Prints one JSON line per count; fails without a GPU."""
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
    ap.add_argument("--problems", type=int, default=4096)
    ap.add_argument("--correspondences", default="100,300")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sim3_opt_bench: no GPU (there is no CPU fallback to time)")
    import sim3_opt_common as soc
    from object_slam_amd import sim3_opt
    from object_slam_amd._lib import check, upload as up
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    B = args.problems
    reps = (B + 63) // 64
    for N in [int(x) for x in args.correspondences.split(",")]:
        base = [soc.make_problem(700 + i, N, i % 2) for i in range(64)]
        arrays, counts = soc.concat_batch(base)
        tile = lambda v: np.tile(v, (reps,) + (1,) * (np.ndim(v) - 1))[:B]
        pr = sim3_opt.pack_problems(tile(counts), soc.K, soc.K, tile(np.array([p["s12"] for p in base])), tile(np.stack([p["R12"] for p in base])),
                                    tile(np.stack([p["t12"] for p in base])), tile(np.array([p["fix_scale"] for p in base])))
        M = int(pr["count"].sum())
        keys = ("X3Dc1", "X3Dc2", "obs1", "obs2", "invSigma2_1", "invSigma2_2")
        d = {k: up(np.tile(arrays[k], (reps,) + (1,) * (arrays[k].ndim - 1))[:M]) for k in keys}   # every repetition reads, and writes, rows of its own
        d_pr = up(pr)
        d_S = torch.zeros(B * 13, dtype=torch.float64, device=dev)
        d_in = torch.zeros(M, dtype=torch.uint8, device=dev)
        d_st = torch.zeros(B * 4, dtype=torch.int32, device=dev)
        opt = sim3_opt.Sim3Optimizer(B, M)

        def launch():
            check(opt.L.oslam_optimize_sim3_batch_device(opt.h, B, d_pr.data_ptr(), M, *[d[k].data_ptr() for k in keys], d_S.data_ptr(), d_in.data_ptr(), d_st.data_ptr(), None, None,
                                                         C.c_void_p(stream.cuda_stream)))

        ms = []
        for rep in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            e1.synchronize()
            if rep >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        st = d_st.cpu().numpy().reshape(B, 4)
        med = float(np.median(ms))
        print(json.dumps(dict(tool="sim3_opt_bench", problems=B, correspondences=N, warmup=args.warmup, reps=args.reps, us_median=round(med * 1e3, 2), us_min=round(min(ms) * 1e3, 2),
                              us_max=round(max(ms) * 1e3, 2), us_per_problem=round(med * 1e3 / B, 3), problems_per_s=round(B / med * 1e3, 1),
                              mean_inliers=round(float(st[:, 0].mean()), 2), mean_lm_iterations=round(float((st[:, 3] >> 8).mean()), 2),
                              mean_lm_trials=round(float((st[:, 3] & 255).mean()), 2), refused=int((st[:, 0] < 0).sum()))), flush=True)
        opt.close()


if __name__ == "__main__":
    main()
