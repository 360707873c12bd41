#!/usr/bin/env python3
"""Measures the Sim3 projection operators' batch entry points (oslam_match_search_by_projection_sim3_batch_device and oslam_match_fuse_sim3_batch_device,
object_slam_amd/csrc/sim3_project.hip).

    python tools/sim3_project_bench.py [--sequences 64] [--keyframes 20] [--keypoints 1000] [--points 5000] [--warmup 3] [--reps 20]

Two batches at loop-sized inputs from tests/sim3_project_common.py's generator: `sequences` search problems (th = 10), and `sequences` x `keyframes` Fuse problems
(th = 4).  Eight distinct problems per mode are generated; every problem of a batch reads the input rows of one of them (inputs are only read, so the batch's
working set is smaller than a real one's, whose keyframes all differ) and writes output rows of its own.  Everything is resident on the device; one call = one
launch timed with device events after the warm-up calls; the median over the timed calls.  Prints one JSON line per mode: microseconds per call, points per second,
and for the search the fixpoint passes taken.  Fails without a GPU."""
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
    ap.add_argument("--sequences", type=int, default=64)
    ap.add_argument("--keyframes", type=int, default=20)
    ap.add_argument("--keypoints", type=int, default=1000)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sim3_project_bench: no GPU (there is no CPU fallback to time)")
    import sim3_project_common as spc
    from object_slam_amd import sim3_project
    from object_slam_amd._lib import check, ptr, upload as up
    from object_slam_amd.matcher import Camera
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    cam = Camera(*spc.CAM, 0.0, 0.0)
    bnd, sf = np.asarray(spc.BOUNDS, np.float32), np.ascontiguousarray(spc.SF)
    for mode, B in (("search", args.sequences), ("fuse", args.sequences * args.keyframes)):
        base = [spc.make_problem(950 + i, args.keypoints - 40 + (i * 7) % 80, args.points - 40 + (i * 13) % 80 + 1, (1.0, 1.1, 0.9, 1.05)[i % 4], mode) for i in range(8)]
        kf, pts, skip, kp_off, pt_off, _, _ = spc.concat_batch(base)
        which = np.arange(B) % len(base)
        n_kp, n_pts = np.array([len(p["kf"]["state"]) for p in base])[which], np.array([len(p["skip"]) for p in base])[which]
        pr = sim3_project.pack_problems(n_kp, kp_off[which], n_pts, pt_off[which], np.stack([p["Scw"] for p in base])[which], [base[0]["th"]] * B)   # consecutive output rows
        n_kp_out, n_pt_out = int(n_kp.sum()), int(n_pts.sum())
        d_skip = up(np.concatenate([base[w]["skip"] for w in which]))
        d_kf, d_pts, d_pr = {k: up(kf[k]) for k in sim3_project.KF_KEYS}, {k: up(pts[k]) for k in sim3_project.PT_KEYS}, up(pr)
        rk = sim3_project.KfRows(len(kf["state"]), *[d_kf[k].data_ptr() for k in sim3_project.KF_KEYS])
        rp = sim3_project.PtRows(len(pts["Xw"]), *[d_pts[k].data_ptr() for k in sim3_project.PT_KEYS])
        d_out0 = torch.full((n_kp_out if mode == "search" else n_pt_out,), -1, dtype=torch.int32, device=dev)
        d_out1 = torch.full((n_pt_out,), -1, dtype=torch.int32, device=dev) if mode == "fuse" else None
        d_count, d_pass = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        proj = sim3_project.Sim3Projector(B, sim3_project.MAX_KEYPOINTS, max(n_pt_out, len(pts["Xw"])))
        common = (C.addressof(cam), ptr(bnd), ptr(sf), len(sf), float(spc.LOG_SF))

        def launch():
            if mode == "search":
                check(proj.L.oslam_match_search_by_projection_sim3_batch_device(proj.h, B, d_pr.data_ptr(), C.addressof(rk), C.addressof(rp), n_pt_out, d_skip.data_ptr(), n_kp_out, *common,
                                                                                d_out0.data_ptr(), d_count.data_ptr(), d_pass.data_ptr(), C.c_void_p(stream.cuda_stream)))
            else:
                check(proj.L.oslam_match_fuse_sim3_batch_device(proj.h, B, d_pr.data_ptr(), C.addressof(rk), C.addressof(rp), n_pt_out, d_skip.data_ptr(), *common, d_out0.data_ptr(),
                                                                d_out1.data_ptr(), d_count.data_ptr(), C.c_void_p(stream.cuda_stream)))

        ms = []
        for rep in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            e1.synchronize()
            if rep >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        cnt = d_count.cpu().numpy()
        med = float(np.median(ms))
        out = dict(tool="sim3_project_bench", mode=mode, problems=B, keypoints=args.keypoints, points=args.points, warmup=args.warmup, reps=args.reps, us_median=round(med * 1e3, 2),
                   us_min=round(min(ms) * 1e3, 2), us_max=round(max(ms) * 1e3, 2), us_per_problem=round(med * 1e3 / B, 3), points_per_s=round(n_pt_out / med * 1e3, 1),
                   mean_count=round(float(cnt.mean()), 2), refused=int((cnt < 0).sum()))
        if mode == "search":
            passes = d_pass.cpu().numpy()
            out.update(passes_max=int(passes.max()), passes_mean=round(float(passes.mean()), 2))
        print(json.dumps(out), flush=True)
        proj.close()


if __name__ == "__main__":
    main()
