#!/usr/bin/env python3
"""Measures the object association's device entry points (object_slam_amd/csrc/object_match.hip).

    python tools/object_match_bench.py [--frames 1 64 512] [--detections 3 8] [--objects 8 64] [--observations 1 16 128] [--warmup 3] [--reps 15] [--only OPERATOR ...] [--out FILE]

Histograms: 640 x 480 frames of uniformly random pixels (and once a frame of one colour, where every pixel of a mask hits the same three counters), masks that are
rectangles of a tenth to a half of the frame.  Per (frames, detections): microseconds per frame, the two kernels' milliseconds (oslam_objmatch_last_kernel_ms),
and achieved bytes per second against the byte model image bytes + n mask bytes per pixel, next to a device-to-device copy of as many bytes timed the same way.
Matchers: random L1-normalised histograms, 20 keypoints per detection; per configuration microseconds per problem.  Everything is resident on the device; a call
is timed with device events on its stream after the warm-up calls; medians.  One JSON line per configuration (appended to --out).  Fails without a GPU."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

W, H, BINS, KPS = 640, 480, 94, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 64, 512])
    ap.add_argument("--detections", type=int, nargs="+", default=[3, 8])
    ap.add_argument("--objects", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--observations", type=int, nargs="+", default=[1, 16, 128])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", choices=["hsv_histograms", "match_two_frame", "match_map_to_frame"], nargs="+", default=None, help="measure these operators only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("object_match_bench: no GPU (there is no CPU fallback to time)")
    from object_slam_amd import object_match as om
    from object_slam_amd._lib import check, upload as up
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    rng = np.random.default_rng(0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

    def timed(fn, before=None):
        ms = []
        for rep in range(args.warmup + args.reps):
            if before is not None:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if rep >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    def emit(out):
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    prm = om.make_params()
    want = lambda op: args.only is None or op in args.only
    max_frames = max(args.frames)
    m = om.ObjectMatcher(max_frames, W, H, max(8, max(args.detections)), max(args.objects), max_frames * max(args.objects) * max(args.observations),
                         max_frames * max(args.detections) * KPS)
    m.set_timing(True)
    # ---- histograms ----
    for F in args.frames if want("hsv_histograms") else []:
        for n in args.detections:
            for content in ("noise", "flat") if (F, n) == (64, max(args.detections)) else ("noise",):
                img = torch.randint(0, 256, (F, H, 3 * W), dtype=torch.uint8, device=dev, generator=gen) if content == "noise" else torch.full((F, H, 3 * W), 90, dtype=torch.uint8, device=dev)
                base = np.zeros((8 * n, H, W), np.uint8)
                for k in range(8 * n):
                    w, h = int(rng.integers(W // 4, W * 3 // 4)), int(rng.integers(H // 3, H * 2 // 3))
                    x, y = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
                    base[k, y:y + h, x:x + w] = 255
                masks = up(base).reshape(8 * n, H, W).repeat((F + 7) // 8, 1, 1)[:F * n].contiguous()
                frames = up(om.pack_frames([n] * F))
                counts = torch.zeros((F * n, BINS), dtype=torch.int32, device=dev)
                hist = torch.zeros((F * n, BINS), dtype=torch.float32, device=dev)

                def call():
                    check(m.L.oslam_objmatch_hsv_histograms_device(m.h, F, W, H, 3 * W, W, img.data_ptr(), frames.data_ptr(), F * n, masks.data_ptr(), counts.data_ptr(), hist.data_ptr(), sp))
                med, lo, hi = timed(call)
                k_ms = m.last_kernel_ms()
                nbytes = F * W * H * (3 + n)
                src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                dst = torch.empty_like(src)
                cmed, _, _ = timed(lambda: dst.copy_(src))
                covered = float(counts[:n].sum().item()) / (3.0 * n * W * H)
                ok = bool((counts.sum(1).cpu().numpy() == 3 * masks.reshape(F * n, -1).ne(0).sum(1).cpu().numpy()).all())
                emit(dict(tool="object_match_bench", op="hsv_histograms", frames=F, detections=n, content=content, width=W, height=H, warmup=args.warmup, reps=args.reps,
                          us_median=round(med * 1e3, 2), us_min=round(lo * 1e3, 2), us_max=round(hi * 1e3, 2), us_per_frame=round(med * 1e3 / F, 3), count_kernel_ms=round(k_ms[0], 4),
                          combine_kernel_ms=round(k_ms[1], 4), model_bytes=nbytes, gbytes_per_s=round(nbytes / med / 1e6, 1), copy_us=round(cmed * 1e3, 2),
                          copy_gbytes_per_s=round(nbytes / cmed / 1e6, 1), share_of_copy=round(cmed / med, 3), mask_coverage=round(covered, 3), counts_sum_to_mask_pixels=ok))
                del img, masks, src, dst

    def rand_hist(rows):
        h = torch.rand((rows, BINS), dtype=torch.float32, device=dev, generator=gen) ** 4
        return (h / h.sum(1, keepdim=True)).contiguous()

    # ---- MatchTwoFrame ----
    for B in args.frames if want("match_two_frame") else []:
        for n in args.detections:
            R = B * n
            hp, hc = rand_hist(R), rand_hist(R)
            box = (torch.rand((R, 4), dtype=torch.float32, device=dev, generator=gen) * 100 + 20).contiguous()
            label = torch.randint(0, 3, (R,), dtype=torch.int32, device=dev, generator=gen)
            pre_id = torch.arange(R, dtype=torch.int32, device=dev)
            cur_id = torch.full((R,), -1, dtype=torch.int32, device=dev)
            pr = up(om.pack_pair_problems([n] * B, [n] * B))
            sim, iou = torch.zeros(R * n, dtype=torch.float32, device=dev), torch.zeros(R * n, dtype=torch.float32, device=dev)
            nas, st = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
            rp = om.DetRows(R, label.data_ptr(), hp.data_ptr(), box.data_ptr(), pre_id.data_ptr(), None, None, 0, None)
            rc = om.DetRows(R, label.data_ptr(), hc.data_ptr(), box.data_ptr(), cur_id.data_ptr(), None, None, 0, None)

            def call():
                check(m.L.oslam_objmatch_match_two_frame_device(m.h, B, pr.data_ptr(), C.byref(rp), C.byref(rc), C.byref(prm), R * n, sim.data_ptr(), iou.data_ptr(), nas.data_ptr(), st.data_ptr(), sp))
            med, lo, hi = timed(call, before=lambda: cur_id.fill_(-1))
            emit(dict(tool="object_match_bench", op="match_two_frame", problems=B, detections=n, us_median=round(med * 1e3, 2), us_min=round(lo * 1e3, 2), us_max=round(hi * 1e3, 2),
                      us_per_problem=round(med * 1e3 / B, 3), kernel_ms=round(m.last_kernel_ms()[0], 4), refused=int((st != 0).sum().item()), mean_assigned=round(float(nas.float().mean().item()), 2)))

    # ---- MatchMapToFrame ----
    for B in args.frames if want("match_map_to_frame") else []:
        for n in args.detections:
            for no in args.objects:
                for nobs in args.observations:
                    R, RO, NO = B * n, B * no, B * no * nobs
                    hc, oh = rand_hist(R), rand_hist(NO)
                    oc = (torch.rand((NO, 3), dtype=torch.float32, device=dev, generator=gen) * 4).contiguous()
                    kps = torch.rand((R * KPS, 3), dtype=torch.float32, device=dev, generator=gen)
                    kps = (kps * torch.tensor([W, H, 4.0], device=dev) + torch.tensor([0.0, 0.0, 0.5], device=dev)).contiguous()
                    label = torch.randint(0, 3, (R,), dtype=torch.int32, device=dev, generator=gen)
                    olabel = torch.randint(0, 3, (RO,), dtype=torch.int32, device=dev, generator=gen)
                    cur_id = torch.full((R,), -1, dtype=torch.int32, device=dev)
                    oid = torch.arange(RO, dtype=torch.int32, device=dev)
                    koff, kn = torch.arange(R, dtype=torch.int32, device=dev) * KPS, torch.full((R,), KPS, dtype=torch.int32, device=dev)
                    ooff, on = torch.arange(RO, dtype=torch.int32, device=dev) * nobs, torch.full((RO,), nobs, dtype=torch.int32, device=dev)
                    pr = up(om.pack_map_problems([n] * B, [no] * B, np.tile(np.eye(3, dtype=np.float32).reshape(9), (B, 1)), np.zeros((B, 3), np.float32), (520.0, 520.0, 320.0, 240.0)))
                    sc = [torch.zeros(RO * n, dtype=torch.float32, device=dev) for _ in range(3)]
                    ints = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3)]
                    rc = om.DetRows(R, label.data_ptr(), hc.data_ptr(), None, cur_id.data_ptr(), koff.data_ptr(), kn.data_ptr(), R * KPS, kps.data_ptr())
                    ro = om.ObjRows(RO, oid.data_ptr(), olabel.data_ptr(), ooff.data_ptr(), on.data_ptr(), NO, oc.data_ptr(), oh.data_ptr())

                    def call():
                        check(m.L.oslam_objmatch_match_map_to_frame_device(m.h, B, pr.data_ptr(), C.byref(rc), C.byref(ro), C.byref(prm), RO * n, sc[0].data_ptr(), sc[1].data_ptr(), sc[2].data_ptr(),
                                                                           ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(), sp))
                    med, lo, hi = timed(call, before=lambda: cur_id.fill_(-1))
                    emit(dict(tool="object_match_bench", op="match_map_to_frame", problems=B, detections=n, objects=no, observations=nobs, us_median=round(med * 1e3, 2), us_min=round(lo * 1e3, 2),
                              us_max=round(hi * 1e3, 2), us_per_problem=round(med * 1e3 / B, 3), kernel_ms=round(m.last_kernel_ms()[0], 4), refused=int((ints[2] != 0).sum().item()),
                              pairs_scored=int((~torch.isnan(sc[0])).sum().item())))
                    del oh, oc
    m.close()


if __name__ == "__main__":
    main()
