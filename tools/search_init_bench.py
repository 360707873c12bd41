#!/usr/bin/env python3
"""Measures the initialisation search's batch entry point (oslam_match_search_for_initialization_batch_device, object_slam_amd/csrc/search_init.hip).

    python tools/search_init_bench.py [--problems 1 64 1024 8192] [--keys 2000] [--warmup 3] [--reps 15] [--out profiles/search_init_bench.jsonl]

Per problem count one batch from tests/search_init_common.py's generator: every problem two frames of `keys` keys (2000: the monocular extractor's 2 * nFeatures),
windowSize 100, nnratio 0.9, the orientation check on, the carried points at the keys' own positions (the first call after the reference frame was taken).  Eight
distinct problems are generated and repeated over the batch; every problem has frames-1 rows, carried points and output rows of its own (the ABI asks for that) and
reads the frames-2 rows of its base problem.  Everything is resident on the device; one call = one launch timed with device events on the call's stream after the
warm-up calls, the carried points put back before every call; the median over the timed calls.  Prints one JSON line per batch (and appends it to --out):
microseconds per call, problems per second, the share of workgroup 0's shader-clock ticks spent in the sequential replay (phase B), and the share of the searching
keys whose candidate list overflowed the kernel's per-key cache.  Fails without a GPU."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

N_BASE = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, nargs="+", default=[1, 64, 1024, 8192])
    ap.add_argument("--keys", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("search_init_bench: no GPU (there is no CPU fallback to time)")
    import search_init_common as sic
    from object_slam_amd import search_init
    from object_slam_amd._lib import check, ptr, upload as up
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    n = args.keys
    extra = max(20, n // 13)
    base = [sic.make_problem(960 + i, n - extra, extra, extra, frac0=0.35, n_plant=12, n_chain=4, n_twin=4, n_crowd=2) for i in range(N_BASE)]
    f1, f2, prev, _, off2 = sic.concat_batch(base)
    searching = np.array([int((p["f1"]["keysUn"]["octave"] == 0).sum()) for p in base])
    d_f2 = {k: up(f2[k]) for k in search_init.ROW_KEYS}
    r2 = search_init.F2Rows(len(f2["desc"]), *[d_f2[k].data_ptr() for k in search_init.ROW_KEYS])
    d_base1 = {k: up(f1[k]) for k in search_init.ROW_KEYS}
    d_base_prev = up(prev)
    bnd = np.asarray(sic.BOUNDS, np.float32)
    for B in args.problems:
        rounds = (B + N_BASE - 1) // N_BASE
        M1 = B * n
        # frames-1 rows of problem j = those of base problem j % 8, at rows j * keys: the eight base problems, repeated on the device
        d_f1 = {k: d_base1[k].repeat(rounds)[:M1 * (28 if k == "keysUn" else 32)].contiguous() for k in search_init.ROW_KEYS}
        d_prev0 = d_base_prev.repeat(rounds)[:M1 * 8].contiguous()
        d_prev = d_prev0.clone()
        which = np.arange(B) % N_BASE
        pr = search_init.pack_problems([n] * B, [n] * B, sic.WINDOW, np.arange(B, dtype=np.int64) * n, off2[which])
        d_pr = up(pr)
        r1 = search_init.F1Rows(M1, *[d_f1[k].data_ptr() for k in search_init.ROW_KEYS])
        d_m12 = torch.full((M1,), -1, dtype=torch.int32, device=dev)
        d_count, d_removed, d_disp, d_over = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4)]
        m = search_init.InitMatcher(B, search_init.MAX_KEYPOINTS, M1)

        def launch():
            check(m.L.oslam_match_search_for_initialization_batch_device(m.h, B, d_pr.data_ptr(), C.addressof(r1), C.addressof(r2), ptr(bnd), float(sic.NNRATIO), 1, d_prev.data_ptr(),
                                                                         d_m12.data_ptr(), d_count.data_ptr(), d_removed.data_ptr(), d_disp.data_ptr(), d_over.data_ptr(),
                                                                         C.c_void_p(stream.cuda_stream)))

        ms = []
        for rep in range(args.warmup + args.reps):
            d_prev.copy_(d_prev0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            e1.synchronize()
            if rep >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        ticks = m.last_phase_ticks()
        cnt, over = d_count.cpu().numpy(), d_over.cpu().numpy()
        # the batch computes what the restatement computes (the first problem of the batch, on the CPU)
        want = sic.run_problem(base[0])
        ok = bool(np.array_equal(d_m12[:n].cpu().numpy(), want[0]) and int(cnt[0]) == want[2])
        med = float(np.median(ms))
        out = dict(tool="search_init_bench", problems=B, keys=n, window=sic.WINDOW, nnratio=float(sic.NNRATIO), warmup=args.warmup, reps=args.reps, us_median=round(med * 1e3, 2),
                   us_min=round(min(ms) * 1e3, 2), us_max=round(max(ms) * 1e3, 2), us_per_problem=round(med * 1e3 / B, 3), problems_per_s=round(B / med * 1e3, 1),
                   phase_ticks=dict(zip(("stage", "candidates", "replay", "outputs"), ticks)), replay_share=round(ticks[2] / max(1, sum(ticks)), 4),
                   searching_keys_mean=round(float(searching[which].mean()), 1), overflow_share=round(float(over.sum()) / float(searching[which].sum()), 6),
                   mean_matches=round(float(cnt.mean()), 2), mean_removed=round(float(d_removed.cpu().numpy().mean()), 2), mean_displaced=round(float(d_disp.cpu().numpy().mean()), 2),
                   refused=int((cnt < 0).sum()), first_problem_matches_restatement=ok)
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        m.close()
        del d_f1, d_prev0, d_prev, d_m12


if __name__ == "__main__":
    main()
