#!/usr/bin/env python3
"""Measures the relocalisation projection operator's batch entry point (oslam_match_search_by_projection_reloc_batch_device,
object_slam_amd/csrc/reloc_project.hip).

    python tools/reloc_project_bench.py [--problems 64 1024] [--keypoints 1000] [--slots 1000] [--warmup 3] [--reps 7] [--out profiles/reloc_project_bench.jsonl]

Per problem count, two batches from tests/reloc_project_common.py's generator: the coarse search (th = 10, ORBdist = 100) and the fine one (th = 3, ORBdist = 64) of
Tracking::Relocalization, every problem a frame of `keypoints` keypoints against the `slots` map-point slots of one keyframe.  Eight distinct problems per mode are
generated; every problem of a batch reads the input rows of one of them (inputs are only read, so the batch's working set is smaller than a real one's, whose frames
all differ) and writes output rows of its own.  Everything is resident on the device; one call = one launch timed with device events after the warm-up calls; the
median over the timed calls.  Prints one JSON line per batch (and appends it to --out): microseconds per call, slots per second, matches, matches the histogram
removed and the fixpoint passes taken.  Fails without a GPU."""
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
    ap.add_argument("--problems", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--keypoints", type=int, default=1000)
    ap.add_argument("--slots", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("reloc_project_bench: no GPU (there is no CPU fallback to time)")
    import reloc_project_common as rpc
    from object_slam_amd import reloc_project
    from object_slam_amd._lib import check, ptr, upload as up
    from object_slam_amd.matcher import Camera
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    cam = Camera(*rpc.CAM, 0.0, 0.0)
    bnd, sf = np.asarray(rpc.BOUNDS, np.float32), np.ascontiguousarray(rpc.SF)
    for mode in (rpc.COARSE, rpc.FINE):
        base = [rpc.make_problem(950 + i, args.keypoints - 40 + (i * 7) % 80, args.slots - 40 + (i * 13) % 80 + 1, mode) for i in range(8)]
        fr, pts, _, kp_off, pt_off = rpc.concat_batch(base)
        d_fr, d_pts = {k: up(fr[k]) for k in reloc_project.FRAME_KEYS}, {k: up(pts[k]) for k in reloc_project.PT_KEYS}
        rf = reloc_project.FrameRows(len(fr["has_mp"]), *[d_fr[k].data_ptr() for k in reloc_project.FRAME_KEYS])
        rp = reloc_project.PtRows(len(pts["Xw"]), *[d_pts[k].data_ptr() for k in reloc_project.PT_KEYS])
        for B in args.problems:
            which = np.arange(B) % len(base)
            n_kp, n_pts = np.array([len(p["frame"]["has_mp"]) for p in base])[which], np.array([len(p["skip"]) for p in base])[which]
            pr = reloc_project.pack_problems(n_kp, kp_off[which], n_pts, pt_off[which], np.stack([p["Tcw"] for p in base])[which], [mode[0]] * B, [mode[1]] * B)   # consecutive output rows
            n_kp_out, n_pt_out = int(n_kp.sum()), int(n_pts.sum())
            d_skip, d_pr = up(np.concatenate([base[w]["skip"] for w in which])), up(pr)
            d_matched = torch.full((n_kp_out,), -1, dtype=torch.int32, device=dev)
            d_count, d_removed, d_pass = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3)]
            proj = reloc_project.RelocProjector(B, reloc_project.MAX_KEYPOINTS, max(n_pt_out, len(pts["Xw"])))

            def launch():
                check(proj.L.oslam_match_search_by_projection_reloc_batch_device(proj.h, B, d_pr.data_ptr(), C.addressof(rf), C.addressof(rp), n_pt_out, d_skip.data_ptr(), n_kp_out,
                                                                                 C.addressof(cam), ptr(bnd), ptr(sf), len(sf), float(rpc.LOG_SF), 1, d_matched.data_ptr(), d_count.data_ptr(),
                                                                                 d_removed.data_ptr(), d_pass.data_ptr(), C.c_void_p(stream.cuda_stream)))

            ms = []
            for rep in range(args.warmup + args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch()
                e1.record(stream)
                e1.synchronize()
                if rep >= args.warmup:
                    ms.append(e0.elapsed_time(e1))
            cnt, passes = d_count.cpu().numpy(), d_pass.cpu().numpy()
            med = float(np.median(ms))
            out = dict(tool="reloc_project_bench", th=mode[0], ORBdist=mode[1], problems=B, keypoints=args.keypoints, slots=args.slots, warmup=args.warmup, reps=args.reps,
                       us_median=round(med * 1e3, 2), us_min=round(min(ms) * 1e3, 2), us_max=round(max(ms) * 1e3, 2), us_per_problem=round(med * 1e3 / B, 3),
                       slots_per_s=round(n_pt_out / med * 1e3, 1), mean_count=round(float(cnt.mean()), 2), mean_removed=round(float(d_removed.cpu().numpy().mean()), 2),
                       refused=int((cnt < 0).sum()), passes_max=int(passes.max()), passes_mean=round(float(passes.mean()), 2))
            line = json.dumps(out)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            proj.close()


if __name__ == "__main__":
    main()
