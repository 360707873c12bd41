#!/usr/bin/env python3
"""Measures the PnP solver's batch entry point (oslam_pnp_ransac_batch_device, object_slam_amd/csrc/pnp.hip).

    python tools/pnp_bench.py [--problems 1024] [--n 100] [--outliers 0.2] [--warmup 3] [--reps 20]

`--problems` generated scenes (tests/pnp_common.py's generator: N correspondences each, a fifth of them outliers) with the reference's parameters
(0.99, 10, 300, 4, 0.5, 5.991), resident on the device; device events around each call (both launches) after the warm-up calls; median, minimum and
maximum over the repetitions.  Prints one JSON line; fails without a GPU."""
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
    ap.add_argument("--problems", type=int, default=1024)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--outliers", type=float, default=0.2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pnp_bench: no GPU (there is no CPU fallback to time)")
    import pnp_common as pc
    from object_slam_amd import pnp
    from object_slam_amd._lib import check, upload as up
    B, N = args.problems, args.n
    base = [pc.make_scene(500 + i, N, outlier_frac=args.outliers) for i in range(min(B, 64))]   # 64 distinct scenes, repeated with other seeds
    scenes = [base[i % len(base)] for i in range(B)]
    pr = pnp.pack_problems([N] * B, [s["K"] for s in scenes], np.arange(B) + 1)
    p3 = np.concatenate([s["P3Dw"] for s in scenes]); p2 = np.concatenate([s["P2D"] for s in scenes]); sg = np.concatenate([s["sigma2"] for s in scenes])
    prm = pnp.make_params()
    solver = pnp.PnPsolver(B, B * N, prm.max_iterations)
    dev = torch.device("cuda", 0)
    d_pr, d_p3, d_p2, d_sg = up(pr), up(p3), up(p2), up(sg)
    d_T = torch.zeros(B * 16, dtype=torch.float32, device=dev)
    d_in = torch.zeros(B * N, dtype=torch.uint8, device=dev)
    d_st = torch.zeros(B * 4, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream()

    def launch():
        check(solver.L.oslam_pnp_ransac_batch_device(solver.h, B, d_pr.data_ptr(), B * N, d_p3.data_ptr(), d_p2.data_ptr(), d_sg.data_ptr(), C.addressof(prm), None,
                                                     d_T.data_ptr(), d_in.data_ptr(), d_st.data_ptr(), None, C.c_void_p(stream.cuda_stream)))

    for _ in range(args.warmup):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    st = d_st.cpu().numpy().reshape(B, 4)
    truth = np.stack([s["truth"] for s in scenes])
    flags = d_in.cpu().numpy().reshape(B, N).astype(bool)
    rp = pnp.ransac_params(N)
    hyp = B * rp["iterations"]
    med = float(np.median(ms))
    print(json.dumps(dict(tool="pnp_bench", problems=B, n=N, outliers=args.outliers, iterations=rp["iterations"], hypotheses=hyp, warmup=args.warmup, reps=args.reps,
                          ms_median=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), problems_per_s=round(B / med * 1e3, 1),
                          hypotheses_per_s=round(hyp / med * 1e3, 1), refined=int((st[:, 0] == 1).sum()), best_unrefined=int((st[:, 0] == 2).sum()),
                          none=int((st[:, 0] == 0).sum()), inlier_sets_equal_truth=int((flags == truth).all(1).sum()),
                          mean_iterations_run=round(float(st[:, 2].mean()), 2))))
    solver.close()


if __name__ == "__main__":
    main()
