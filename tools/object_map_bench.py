#!/usr/bin/env python3
"""Measures the object map maintenance's device entry points (object_slam_amd/csrc/object_map.hip).

    python tools/object_map_bench.py [--problems 512] [--points 300 3000] [--stream-points 6000] [--objects 64] [--warmup 3] [--reps 15] [--out FILE]

reject_outliers, mode UPDATE, every label good: per point count a batch of blobs (jittered grids of spacing 0.07, one cluster each) and a batch of single lines of
spacing 0.09 in shuffled order (the worst case for the component search); then the TEST5 path at --stream-points points, and center_and_size at every size.
Kernel milliseconds come from the handle's timing (oslam_objmap_last_kernel_ms), medians over the calls after the warm-up.  The clustering shapes report the
rounds the search took and pair tests per second (rounds * n * n per problem); the streaming kernels report the ratio to a device-to-device copy of their input
bytes, timed with events the same way.  merge_sets: --problems maps of --objects objects.  One JSON line per configuration (appended to --out).  Fails without a GPU."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=512)
    ap.add_argument("--points", type=int, nargs="+", default=[300, 3000])
    ap.add_argument("--stream-points", type=int, default=6000)
    ap.add_argument("--objects", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("object_map_bench: no GPU (there is no CPU fallback to time)")
    from object_slam_amd import object_map as om
    from object_slam_amd._lib import check, upload as up
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    rng = np.random.default_rng(0)
    B = args.problems
    m = om.ObjectMap(B, om.MIN_CLUSTER_POINTS, om.MAX_OBJECTS)
    m.set_timing(True)

    def kernel_ms(fn):
        ms = []
        for rep in range(args.warmup + args.reps):
            fn()
            stream.synchronize()
            if rep >= args.warmup:
                ms.append(m.last_kernel_ms())
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    def copy_ms(nbytes):
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        ms = []
        for rep in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            dst.copy_(src)
            e1.record(stream)
            e1.synchronize()
            if rep >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    def emit(out):
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def blob(n):
        side = int(np.ceil(n ** (1 / 3)))
        g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(side ** 3)[:n]]
        return g * 0.07 + rng.uniform(-0.01, 0.01, (n, 3))

    def line(n):
        p = np.zeros((n, 3))
        p[:, 0] = 0.09 * rng.permutation(n)
        return p

    def run(op, shape, n, make):
        pos = np.concatenate([make(n) for _ in range(B)]).astype(np.float32)
        R = B * n
        t = dict(pr=up(om.pack_problems([n] * B)), pos=up(pos), cnt=up(np.full(R, 3, np.int32)), total=up(np.full(R, 4, np.int32)), keep=up(np.zeros(R, np.uint8)),
                 cluster=up(np.zeros(R, np.int32)), res=up(om.new_results(B)))
        a = lambda k: t[k].data_ptr()
        if op == "reject_outliers":
            call = lambda: check(m.L.oslam_objmap_reject_outliers_device(m.h, B, a("pr"), R, a("pos"), a("cnt"), a("total"), a("keep"), a("cluster"), a("res"), sp))
            in_bytes = R * 20
        else:
            call = lambda: check(m.L.oslam_objmap_center_and_size_device(m.h, B, a("pr"), R, a("pos"), a("res"), sp))
            in_bytes = R * 12
        med, lo, hi = kernel_ms(call)
        res = t["res"].cpu().numpy()[:B * om.RESULT_DTYPE.itemsize].view(om.RESULT_DTYPE)
        out = dict(tool="object_map_bench", op=op, shape=shape, problems=B, points=n, warmup=args.warmup, reps=args.reps, kernel_ms=round(med, 4), kernel_ms_min=round(lo, 4),
                   kernel_ms_max=round(hi, 4), us_per_problem=round(med * 1e3 / B, 3), refused=int((res["status"] != 0).sum()), mean_kept=round(float(res["n_kept"].mean()), 1))
        if op == "reject_outliers" and n <= om.TEST5_ABOVE:
            rounds = res["rounds"].astype(np.int64)
            out.update(path="TEST7", rounds_max=int(rounds.max()), rounds_mean=round(float(rounds.mean()), 2), clusters_mean=round(float(res["n_clusters"].mean()), 2),
                       pair_tests_per_s=round(float(rounds.sum()) * n * n / (med * 1e-3), 0))
        else:
            c = copy_ms(in_bytes)
            out.update(path="TEST5" if op == "reject_outliers" else "extent", input_bytes=in_bytes, copy_ms=round(c, 4), times_the_copy=round(med / c, 1))
        emit(out)
        return med

    for n in args.points:
        tb = run("reject_outliers", "blobs", n, blob)
        tl = run("reject_outliers", "line", n, line)
        emit(dict(tool="object_map_bench", op="reject_outliers", points=n, line_over_blob=round(tl / tb, 2)))
    run("reject_outliers", "blobs", args.stream_points, blob)
    for n in list(args.points) + [args.stream_points]:
        run("center_and_size", "blobs", n, blob)

    # ---- merge sets ----
    n = args.objects
    lo = rng.uniform(-2, 2, (B * n, 3))
    bbox = np.concatenate([lo + rng.uniform(0.3, 1.2, (B * n, 3)), lo], axis=1).astype(np.float32)
    t = dict(pr=up(om.pack_merge_problems([n] * B)), label=up(rng.integers(0, 3, B * n).astype(np.int32)), track=up(np.tile(np.arange(n, dtype=np.int32), B)), bbox=up(bbox),
             ratio=up(np.zeros(B * n * n, np.float32)), member=up(np.zeros(B * n * n, np.uint8)), target=up(np.zeros(B * n, np.int32)), ns=up(np.zeros(B, np.int32)), st=up(np.zeros(B, np.int32)))
    a = lambda k: t[k].data_ptr()
    med, lo_, hi = kernel_ms(lambda: check(m.L.oslam_objmap_merge_sets_device(m.h, B, a("pr"), B * n, a("label"), a("track"), a("bbox"), 6, B * n * n, a("ratio"), a("member"), a("target"),
                                                                                a("ns"), a("st"), sp)))
    ns = t["ns"].cpu().numpy()[:4 * B].view(np.int32)
    emit(dict(tool="object_map_bench", op="merge_sets", problems=B, objects=n, kernel_ms=round(med, 4), kernel_ms_min=round(lo_, 4), kernel_ms_max=round(hi, 4),
              us_per_problem=round(med * 1e3 / B, 3), sets_mean=round(float(ns.mean()), 2), sets_max=int(ns.max())))
    m.close()


if __name__ == "__main__":
    main()
