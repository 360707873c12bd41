#!/usr/bin/env python3
"""Measures OptimizeEssentialGraph's batch entry point (oslam_optimize_essential_graph_batch_device, object_slam_amd/csrc/essential_graph.hip) and its
point correction.

    python tools/essential_graph_bench.py [--keyframes 64,256,1024] [--batches 1,256] [--points 100000] [--warmup 2] [--reps 7]

For every keyframe count, batch size and fix_scale value: drifted rings of tests/essential_graph_common.py (spanning tree, a covisibility edge three
keyframes back, one loop edge whose endpoint is corrected; eight distinct rings repeated up to the batch size, each with rows of its own), everything
resident on the device, one call = one launch timed with device events after the warm-up calls; the median over the timed calls.  Then the point
correction of `points` points over the last batch.  Prints one JSON line per measurement, with the envelope's size; fails without a GPU."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402


def timed(fn, stream, warmup, reps):
    import torch
    ms = []
    for rep in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        if rep >= warmup:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="64,256,1024")
    ap.add_argument("--batches", default="1,256")
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("essential_graph_bench: no GPU (there is no CPU fallback to time)")
    import essential_graph_common as egc
    from object_slam_amd import essential_graph as eg
    from object_slam_amd._lib import check, upload as up
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    for N in [int(x) for x in args.keyframes.split(",")]:
        for fix in (1, 0):
            base = [egc.make_ring(N, 900 + i, bool(fix), scale_drift=not fix) for i in range(8)]
            for B in [int(x) for x in args.batches.split(",")]:
                problems = [base[i % 8] for i in range(B)]
                arrays, n_kf, n_ed = egc.concat_batch(problems)
                pr, row_first = eg.with_envelope(eg.pack_problems(n_kf, n_ed, [fix] * B), arrays["fixed"], arrays["edges"])
                K, E, blocks = int(n_kf.sum()), int(n_ed.sum()), int(pr["env_blocks"].sum())
                d = {k: up(v) for k, v in arrays.items()}
                d_pr, d_rf = up(pr), up(row_first)
                d_S = torch.zeros(K * 13, dtype=torch.float64, device=dev)
                d_T = torch.zeros(K * 16, dtype=torch.float32, device=dev)
                d_st = torch.zeros(B * 4, dtype=torch.int32, device=dev)
                opt = eg.EssentialGraphOptimizer(B, K, E, blocks)

                def launch():
                    check(opt.L.oslam_optimize_essential_graph_batch_device(opt.h, B, d_pr.data_ptr(), K, d["Scw"].data_ptr(), d["Snc"].data_ptr(), d["has_nc"].data_ptr(),
                                                                            d["fixed"].data_ptr(), d_rf.data_ptr(), E, d["edges"].data_ptr(), d_S.data_ptr(), d_T.data_ptr(),
                                                                            d_st.data_ptr(), None, None, sp))

                med, lo, hi = timed(launch, stream, args.warmup, args.reps)
                st = d_st.cpu().numpy().reshape(B, 4)
                print(json.dumps(dict(tool="essential_graph_bench", keyframes=N, batch=B, fix_scale=fix, edges_per_graph=int(n_ed[0]), envelope_blocks_per_graph=int(pr["env_blocks"][0]),
                                      envelope_MiB_per_graph=round(int(pr["env_blocks"][0]) * 800 / 2 ** 20, 3), warmup=args.warmup, reps=args.reps, ms_median=round(med, 3),
                                      ms_min=round(lo, 3), ms_max=round(hi, 3), ms_per_graph=round(med / B, 4), mean_lm_iterations=round(float((st[:, 3] >> 8).mean()), 2),
                                      mean_lm_trials=round(float((st[:, 3] & 255).mean()), 2), refused=int((st[:, 0] != 0).sum()))), flush=True)
                if N == int(args.keyframes.split(",")[-1]) and B == int(args.batches.split(",")[-1]) and fix:
                    M = args.points
                    rng = np.random.default_rng(1)
                    pp = rng.integers(0, B, M).astype(np.int32)
                    ref = rng.integers(0, N, M).astype(np.int32)
                    d_pp, d_ref, d_P = up(pp), up(ref), up(rng.uniform(-5, 5, (M, 3)).astype(np.float32))
                    d_Po = torch.zeros(M * 3, dtype=torch.float32, device=dev)

                    def correct():
                        check(opt.L.oslam_essential_graph_correct_points_device(opt.h, B, d_pr.data_ptr(), K, d["Scw"].data_ptr(), d_S.data_ptr(), d_st.data_ptr(), M, d_pp.data_ptr(),
                                                                                d_ref.data_ptr(), d_P.data_ptr(), d_Po.data_ptr(), sp))

                    med, lo, hi = timed(correct, stream, 3, 20)
                    print(json.dumps(dict(tool="essential_graph_bench", what="correct_points", points=M, us_median=round(med * 1e3, 2), us_min=round(lo * 1e3, 2),
                                          us_max=round(hi * 1e3, 2))), flush=True)
                opt.close()


if __name__ == "__main__":
    main()
