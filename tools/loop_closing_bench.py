#!/usr/bin/env python3
"""Measures the operators of LoopClosing's own arithmetic: SearchByBoW(pKF1, pKF2) (mode 2 of object_slam_amd/csrc/bow_matcher.hip, through
oslam_match_bow_batch, whose kernel time the handle reports), and oslam_loop_propagate_device / oslam_loop_update_after_gba_device of
object_slam_amd/csrc/loop_correct.hip.

    python tools/loop_closing_bench.py [--batches 1,16,64] [--warmup 2] [--reps 7]

BoW: pairs of 2000 x 2000 keypoints over 400 nodes (the clustered generator of tests/loop_closing_common.py, so that claims chain), B pairs per call; the
kernel's device time per call and the number of matches.  Propagation: B problems of 40 keyframes, 300 entries each, 4000 points (the size of
CorrectLoop's neighbourhood), and one problem of 200 keyframes, 1000 entries each, 100 000 points; everything resident on the device, one call = three
launches timed with device events.  Map update after global BA: B maps of 300 keyframes (a chain whose last 12 are outside the BA) and 20 000 points, and
one map of 2000 keyframes and 500 000 points.  The median over the timed calls; one JSON line per measurement; fails without a GPU."""
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
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("loop_closing_bench: no GPU (there is no CPU fallback to time)")
    import loop_closing_common as lcc
    from object_slam_amd import BowMatcher, LoopCorrector, feature_vector
    from object_slam_amd._lib import KP_DTYPE, check, lib, upload as up
    from object_slam_amd.matcher import BowJob
    batches = [int(x) for x in args.batches.split(",")]
    L = lib()
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)

    # ---- SearchByBoW(pKF1, pKF2)
    rng = np.random.default_rng(1)
    pairs = [lcc.bow_kf_pair(rng, 2000, 2000, 400, clusters=600) for _ in range(4)]
    bm = BowMatcher(2400)
    L.oslam_bow_kernel_time.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    for B in batches:
        keep, jobs = [], []
        a = lambda x, dt: keep.append(np.ascontiguousarray(x, dt)) or keep[-1]
        for b in range(B):
            p = pairs[b % 4]
            job = BowJob()
            qi, qn, _, _, _ = feature_vector(p["node1"])
            _, _, nodes, start, items = feature_vector(p["node2"])
            s1, s2 = job.s1, job.s2
            s1.N, s1.keys, s1.desc, s1.flag = 2000, a(p["keys1"], KP_DTYPE).ctypes.data, a(p["desc1"], np.uint8).ctypes.data, a(p["valid1"], np.uint8).ctypes.data
            s1.nq, s1.q_idx, s1.q_node = len(qi), a(qi, np.int32).ctypes.data, a(qn, np.uint32).ctypes.data
            s2.N, s2.keys, s2.desc, s2.has_mp = 2000, a(p["keys2"], KP_DTYPE).ctypes.data, a(p["desc2"], np.uint8).ctypes.data, a(p["valid2"], np.uint8).ctypes.data
            s2.nNodes, s2.nodes, s2.start, s2.items = len(nodes), a(nodes, np.uint32).ctypes.data, a(start, np.int32).ctypes.data, a(items, np.int32).ctypes.data
            job.triangulation, job.nnratio, job.checkOri = 2, 0.75, 1
            job.match = a(np.full(2000, -1, np.int32), np.int32).ctypes.data
            jobs.append(job)
        arr = (BowJob * B)(*jobs)
        ms = []
        for rep in range(args.warmup + args.reps):
            check(L.oslam_bow_kernel_time(bm.h, 1, None, None))
            check(L.oslam_match_bow_batch(bm.h, B, arr, None, None, 0))
            t, n = C.c_double(0), C.c_longlong(0)
            check(L.oslam_bow_kernel_time(bm.h, 0, C.byref(t), C.byref(n)))
            if rep >= args.warmup:
                ms.append(t.value)
        print(json.dumps(dict(op="search_by_bow_kf", pairs=B, keypoints=2000, kernel_ms=float(np.median(ms)), min_ms=min(ms), max_ms=max(ms),
                              us_per_pair=1e3 * float(np.median(ms)) / B, matches=[int(arr[b].nmatches) for b in range(min(B, 4))])), flush=True)
    bm.close()

    # ---- propagation
    def run_prop(problems, tag):
        recs, arr = lcc.pack_prop(problems)
        N, E, M = len(arr["Tiw"]), len(arr["entries"]), len(arr["P"])
        h = LoopCorrector(len(recs), max(N, 1), max(E, 1), max(M, 1))
        outs = [np.zeros((N, 13)), np.zeros((N, 13)), np.zeros((N, 16), np.float32), np.zeros((M, 3), np.float32), np.zeros(M, np.int32), np.zeros((len(recs), 4), np.int32)]
        d = [up(x) for x in (recs, arr["Tiw"], arr["Scw"], arr["kf_entries"], arr["entries"], arr["P"], arr["bad"])] + [up(x) for x in outs]
        torch.cuda.synchronize()
        q = [t.data_ptr() for t in d]
        fn = lambda: check(L.oslam_loop_propagate_device(h.h, len(recs), q[0], N, q[1], q[2], q[3], E, q[4], M, q[5], q[6], q[7], q[8], q[9], q[10], q[11], q[12], sp))
        med, lo, hi = timed(fn, stream, args.warmup, args.reps)
        st = d[12].cpu().numpy().view(np.int32).reshape(-1, 4)[:len(recs)]
        assert (st[:, 0] == 0).all(), st
        print(json.dumps(dict(op="propagate", shape=tag, problems=len(recs), keyframes=N, entries=E, points=M, ms=med, min_ms=lo, max_ms=hi, us_per_problem=1e3 * med / len(recs),
                              points_corrected=int(st[:, 2].sum()))), flush=True)
        h.close()

    base = [lcc.make_prop_problem(300 + i, 40, 300, 4000) for i in range(4)]
    for B in batches:
        run_prop([base[b % 4] for b in range(B)], "40 kf x 300 entries, 4000 points")
    run_prop([lcc.make_prop_problem(310, 200, 1000, 100000, share=8)], "200 kf x 1000 entries, 100000 points")

    # ---- the map update after global BA
    def run_gba(problems, tag):
        recs, arr = lcc.pack_gba(problems)
        N, M = len(arr["parent"]), len(arr["P"])
        h = LoopCorrector(len(recs), max(N, 1), 1, max(M, 1))
        outs = [np.zeros((N, 16), np.float32), np.zeros(N, np.uint8), np.zeros((M, 3), np.float32), np.zeros((len(recs), 4), np.int32)]
        d = [up(x) for x in (recs, arr["parent"], arr["kf_in_ba"], arr["Tcw"], arr["TcwGBA"], arr["P"], arr["PosGBA"], arr["pt_in_ba"], arr["bad"], arr["ref"])] + [up(x) for x in outs]
        torch.cuda.synchronize()
        q = [t.data_ptr() for t in d]
        fn = lambda: check(L.oslam_loop_update_after_gba_device(h.h, len(recs), q[0], N, q[1], q[2], q[3], q[4], M, q[5], q[6], q[7], q[8], q[9], q[10], q[11], q[12], q[13], sp))
        med, lo, hi = timed(fn, stream, args.warmup, args.reps)
        st = d[13].cpu().numpy().view(np.int32).reshape(-1, 4)[:len(recs)]
        assert (st[:, 0] == 0).all(), st
        print(json.dumps(dict(op="update_after_gba", shape=tag, maps=len(recs), keyframes=N, points=M, ms=med, min_ms=lo, max_ms=hi, us_per_map=1e3 * med / len(recs),
                              rounds=int(st[0, 3]), points_written=int(st[:, 2].sum()))), flush=True)
        h.close()

    chain = lambda n, out: ([-1] + list(range(n - 1)), [1] * (n - out) + [0] * out)
    gbase = [lcc.make_gba_problem(400 + i, *chain(300, 12), 20000) for i in range(4)]
    for B in batches:
        run_gba([gbase[b % 4] for b in range(B)], "300 kf (12 outside the BA), 20000 points")
    run_gba([lcc.make_gba_problem(410, *chain(2000, 40), 500000)], "2000 kf (40 outside the BA), 500000 points")


if __name__ == "__main__":
    main()
