#!/usr/bin/env python3
"""Measures the Initializer's batch entry point (oslam_init_initialize_batch_device, object_slam_amd/csrc/initializer.hip).

    python tools/initializer_bench.py [--problems 64,1024,8192] [--matches 300] [--keys 1000] [--iterations 200] [--warmup 3] [--reps 10] [--cpu-problems 4]

For every batch (problems x matches per problem among about `keys` keys per frame; tests/initializer_common.py's generator: general and planar scenes in
turn, 0.5 px noise, a fifth of the matches outliers; the reference's 200 iterations; everything resident on the device) the call is timed with device
events around both launches, after the warm-up calls, and the library's own events between the two launches (oslam_init_set_timing) give the split
between the hypothesis kernel and the reconstruction kernel.  The only comparison is the numpy restatement of tests/initializer_common.py on one CPU
core over the first --cpu-problems problems of the same batch.  Prints one JSON line; fails without a GPU."""
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
    ap.add_argument("--problems", default="64,1024,8192")
    ap.add_argument("--matches", type=int, default=300)
    ap.add_argument("--keys", type=int, default=1000)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-problems", type=int, default=4)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("initializer_bench: no GPU (there is no CPU fallback to time)")
    import initializer_common as ic
    from object_slam_amd import initializer as ini
    from object_slam_amd._lib import check, upload as up
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    N, extra = args.matches, max(0, args.keys - args.matches)
    prm = ini.make_params(max_iterations=args.iterations)
    base = [ic.make_scene(700 + i, N, "planar" if i % 2 else "general", extra1=extra, extra2=extra) for i in range(32)]   # 32 distinct scenes, repeated with other seeds
    t0 = time.perf_counter()
    for i in range(args.cpu_problems):
        s = base[i % len(base)]
        ic.initialize(s["keys1"], s["keys2"], s["matches12"], s["K"], s["sigma"], i + 1, dict(ic.REF, max_iterations=args.iterations))
    cpu_s = (time.perf_counter() - t0) / max(1, args.cpu_problems)
    results = []
    for B in [int(x) for x in args.problems.split(",")]:
        scenes = [base[i % len(base)] for i in range(B)]
        pr = ini.pack_problems([len(s["keys1"]) for s in scenes], [len(s["keys2"]) for s in scenes], [s["K"] for s in scenes], 1.0, np.arange(B) + 1)
        k1 = np.concatenate([s["keys1"] for s in scenes])
        k2 = np.concatenate([s["keys2"] for s in scenes])
        m12 = np.concatenate([s["matches12"] for s in scenes])
        M1, M2 = len(k1), len(k2)
        h = ini.Initializer(B, max(M1, M2), args.iterations)
        h.set_timing(True)
        d_pr, d_k1, d_k2, d_m = up(pr), up(k1), up(k2), up(m12)
        d_R = torch.zeros(B * 9, dtype=torch.float32, device=dev)
        d_t = torch.zeros(B * 3, dtype=torch.float32, device=dev)
        d_P = torch.zeros(M1 * 3, dtype=torch.float32, device=dev)
        d_tri = torch.zeros(M1, dtype=torch.uint8, device=dev)
        d_st = torch.zeros(B * 8, dtype=torch.int32, device=dev)
        d_sc = torch.zeros(B * 4, dtype=torch.float32, device=dev)
        ms, split = [], []
        for rep in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            check(h.L.oslam_init_initialize_batch_device(h.h, B, d_pr.data_ptr(), M1, d_k1.data_ptr(), d_m.data_ptr(), M2, d_k2.data_ptr(), C.addressof(prm), None, d_R.data_ptr(),
                                                         d_t.data_ptr(), d_P.data_ptr(), d_tri.data_ptr(), d_st.data_ptr(), d_sc.data_ptr(), None, None, None, None,
                                                         C.c_void_p(stream.cuda_stream)))
            e1.record(stream)
            e1.synchronize()
            if rep >= args.warmup:
                ms.append(e0.elapsed_time(e1))
                split.append(h.last_kernel_ms())
        st = d_st.cpu().numpy().reshape(B, 8)
        med = float(np.median(ms))
        results.append(dict(problems=B, matches=N, keys1=M1 // B, keys2=M2 // B, iterations=args.iterations, us_median=round(med * 1e3, 1), us_min=round(min(ms) * 1e3, 1),
                            us_max=round(max(ms) * 1e3, 1), problems_per_s=round(B / med * 1e3, 1), hypotheses_per_s=round(2 * B * args.iterations / med * 1e3, 1),
                            us_hypotheses_kernel=round(float(np.median([a for a, _ in split])) * 1e3, 1), us_reconstruct_kernel=round(float(np.median([b for _, b in split])) * 1e3, 1),
                            returned=int((st[:, 0] == 1).sum()), model_H=int((st[:, 1] == 1).sum()), model_F=int((st[:, 1] == 2).sum())))
        h.close()
    print(json.dumps(dict(tool="initializer_bench", warmup=args.warmup, reps=args.reps, params=dict(ini.REFERENCE_PARAMS, max_iterations=args.iterations),
                          restatement_one_core=dict(problems=args.cpu_problems, s_per_problem=round(cpu_s, 4), problems_per_s=round(1 / cpu_s, 2)), batches=results)))


if __name__ == "__main__":
    main()
