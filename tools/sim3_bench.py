#!/usr/bin/env python3
"""Measures the Sim3 solver's batch entry point (oslam_sim3_iterate_batch_device, object_slam_amd/csrc/sim3.hip).

    python tools/sim3_bench.py [--problems 64,1024,8192] [--n 60,257] [--outliers 0.2] [--warmup 3] [--reps 20]

For every batch (problems x correspondences per problem; tests/sim3_common.py's generator, a fifth of the pairs outliers, LoopClosing's parameters
(0.99, 20, 300), everything resident on the device) two calls are timed with device events around both launches, after the warm-up calls: one
iterate(5) round of fresh solvers, as LoopClosing::ComputeSim3 issues it, and one find (300 iterations) of fresh solvers.  The state records are
reset on the stream before every call (outside the timed span).  `hypotheses` is the number of (problem, iteration) pairs the hypotheses kernel
evaluates in the call.  Prints one JSON line; fails without a GPU."""
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
    ap.add_argument("--problems", default="64,1024,8192")
    ap.add_argument("--n", default="60,257")
    ap.add_argument("--outliers", type=float, default=0.2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sim3_bench: no GPU (there is no CPU fallback to time)")
    import sim3_common as sc3
    from object_slam_amd import sim3
    from object_slam_amd._lib import check, upload as up
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    prm = sim3.make_params()
    results = []
    for N in [int(x) for x in args.n.split(",")]:
        base = [sc3.make_scene(500 + i, N, outlier_frac=args.outliers, scale=None if i % 2 else 1.3) for i in range(64)]   # 64 distinct scenes, repeated with other seeds
        its = sim3.ransac_params(N)["iterations"]
        for B in [int(x) for x in args.problems.split(",")]:
            scenes = [base[i % len(base)] for i in range(B)]
            pr = sim3.pack_problems([N] * B, [s["K1"] for s in scenes], [s["K2"] for s in scenes], np.arange(B) + 1, [s["fix_scale"] for s in scenes])
            cat = lambda k: np.concatenate([s[k] for s in scenes])
            solver = sim3.Sim3Solver(B, B * N, prm.max_iterations)
            d_pr, d_x1, d_x2, d_s1, d_s2 = up(pr), up(cat("X1")), up(cat("X2")), up(cat("sigma2_1")), up(cat("sigma2_2"))
            d_fresh, d_state = up(sim3.fresh_states(B)), up(sim3.fresh_states(B))
            d_T = torch.zeros(B * 16, dtype=torch.float32, device=dev)
            d_in = torch.zeros(B * N, dtype=torch.uint8, device=dev)
            d_st = torch.zeros(B * 4, dtype=torch.int32, device=dev)

            def launch(n_iterations):
                check(solver.L.oslam_sim3_iterate_batch_device(solver.h, B, d_pr.data_ptr(), d_state.data_ptr(), B * N, d_x1.data_ptr(), d_x2.data_ptr(), d_s1.data_ptr(),
                                                               d_s2.data_ptr(), C.addressof(prm), n_iterations, None, d_T.data_ptr(), d_in.data_ptr(), d_st.data_ptr(), None, None,
                                                               C.c_void_p(stream.cuda_stream)))

            row = dict(problems=B, n=N, iterations=its)
            for name, n_it in (("iterate5", 5), ("find", 300)):
                ms = []
                for rep in range(args.warmup + args.reps):
                    d_state.copy_(d_fresh)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    launch(n_it)
                    e1.record(stream)
                    e1.synchronize()
                    if rep >= args.warmup:
                        ms.append(e0.elapsed_time(e1))
                st = d_st.cpu().numpy().reshape(B, 4)
                hyp = B * min(n_it, its)
                med = float(np.median(ms))
                row[name] = dict(hypotheses=hyp, us_median=round(med * 1e3, 2), us_min=round(min(ms) * 1e3, 2), us_max=round(max(ms) * 1e3, 2),
                                 hypotheses_per_s=round(hyp / med * 1e3, 1), returned=int((st[:, 0] == 1).sum()), mean_iterations_run=round(float(st[:, 2].mean()), 2))
                if name == "find":
                    truth = np.stack([s["truth"] for s in scenes])
                    flags = d_in.cpu().numpy().reshape(B, N).astype(bool)
                    row[name]["inlier_sets_equal_truth"] = int(((flags == truth).all(1) & (st[:, 0] == 1)).sum())
            results.append(row)
            solver.close()
    print(json.dumps(dict(tool="sim3_bench", outliers=args.outliers, warmup=args.warmup, reps=args.reps, params=dict(sim3.REFERENCE_PARAMS), batches=results)))


if __name__ == "__main__":
    main()
