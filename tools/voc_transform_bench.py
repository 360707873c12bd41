#!/usr/bin/env python3
"""Measures the vocabulary kernel (oslam_voc_transform_device, object_slam_amd/csrc/vocabulary.hip) on the reference vocabulary's shape.

    python tools/voc_transform_bench.py [--arrays 8192] [--per-array 1000] [--reps 20] [--driver-seqs 1024] [--out profiles/voc_transform_<tag>.json]

Kernel leg: a full seeded `10 6` tree (1 111 110 nodes, 35.6 MB of centres) built in memory with oslam_voc_create — no text file —, 8 192 arrays x 1 000
random descriptors, levelsup 4; device events around each launch after warm-up launches, median over the repetitions.  Reported: descriptors/s,
microseconds per launch, achieved bytes/s against the GATHER MODEL of 60 centres x 32 B per descriptor (the 30 centres of the three top levels are served
from LDS: `global_model_bytes` counts the other 30 and their 8-byte links), and for scale the same batch through the two-level k_bow_nodes
(oslam_bow_nodes_device).  The figure to compare with is the machine's rate for uniformly random rows of an Infinity-Cache-resident 38 MB table
(8.6 TB/s chip-wide, measured with 1 152-byte rows; these rows are 320-byte runs).
Driver leg (--driver-seqs S > 0): S RGB-D sequences of bench.py's stream through the driver, once with the substitute vocabulary and once with this tree;
reports the wall time the driver spent in KeyFrame::ComputeBoW through the operator table (oslam_slam_bow_seconds) and the frame rate of both runs.
Prints one JSON line; fails without a GPU."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def full_tree(k=10, L=6, seed=1):
    n = sum(k ** d for d in range(1, L + 1))
    ids = np.arange(1, n + 1, dtype=np.int64)
    parent = ((ids - 1) // k).astype(np.int32)              # breadth-first numbering: the children of node p are p k + 1 .. p k + k
    first_leaf = n - k ** L + 1
    leaf = (ids >= first_leaf).astype(np.uint8)
    rng = np.random.default_rng(seed)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    weight = np.where(leaf > 0, rng.random(n) * 9.0 + 0.01, 0.0)
    return k, L, 0, 0, parent, leaf, desc, weight


def kernel_leg(args):
    import torch
    from object_slam_amd._lib import check, lib
    from object_slam_amd.vocabulary import Vocabulary
    if not torch.cuda.is_available():
        raise SystemExit("voc_transform_bench: no GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    voc = Vocabulary.from_arrays(*full_tree(seed=args.seed))
    build_s = time.perf_counter() - t0
    info = voc.info
    voc.upload(0)
    L = lib()
    n, m = args.arrays, args.per_array
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    desc = torch.randint(0, 256, (n, m, 32), dtype=torch.uint8, device=dev, generator=g)
    ptrs = torch.tensor([desc.data_ptr() + i * m * 32 for i in range(n)], dtype=torch.int64, device=dev)
    counts = torch.full((n,), m, dtype=torch.int32, device=dev)
    word = torch.zeros((n, m), dtype=torch.int32, device=dev)
    node = torch.zeros((n, m), dtype=torch.int32, device=dev)
    weight = torch.zeros((n, m), dtype=torch.float64, device=dev)
    top = torch.randint(0, 2 ** 62, (40,), dtype=torch.int64, device=dev, generator=g)
    sub = torch.randint(0, 2 ** 62, (400,), dtype=torch.int64, device=dev, generator=g)
    out2 = torch.zeros((n, m), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def voc_launch():
        check(L.oslam_voc_transform_device(voc.h, ptrs.data_ptr(), counts.data_ptr(), n, m, 4, word.data_ptr(), node.data_ptr(), weight.data_ptr(), None))

    def sub_launch():
        check(L.oslam_bow_nodes_device(C.c_void_p(ptrs.data_ptr()), C.c_void_p(counts.data_ptr()), n, m, C.c_void_p(top.data_ptr()), C.c_void_p(sub.data_ptr()),
                                       C.c_void_p(out2.data_ptr()), None))

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    # the two kernels alternate, so that a drift of the clock or of the host shows in both
    v1 = timed(voc_launch)
    s1 = timed(sub_launch)
    v2 = timed(voc_launch)
    s2 = timed(sub_launch)
    # what was timed computes the right thing: a sample against the host descent
    pick = np.random.default_rng(0).integers(0, n * m, 4000)
    hw, hn, hwt = voc.transform_host(desc.view(-1, 32)[torch.from_numpy(pick).to(dev)].cpu().numpy(), levelsup=4)
    assert np.array_equal(word.view(-1).cpu().numpy().view(np.uint32)[pick], hw) and np.array_equal(node.view(-1).cpu().numpy().view(np.uint32)[pick], hn)
    assert np.array_equal(weight.view(-1).cpu().numpy()[pick], hwt)
    N = n * m
    med = min(v1[0], v2[0])
    sub_med = min(s1[0], s2[0])
    model = 60 * 32 * N
    glob = (30 * (32 + 8) + 32 + 16 + 16) * N       # levels 4-6 centres + links, the descriptor itself, ids / weight of the leaf and the three outputs
    return {"tree": info, "tree_build_s": round(build_s, 2), "arrays": n, "per_array": m, "descriptors": N, "levelsup": 4, "warmup": args.warmup, "reps": args.reps,
            "voc_transform_ms_median_min_max": [[round(x, 4) for x in v1], [round(x, 4) for x in v2]],
            "bow_nodes_two_level_ms_median_min_max": [[round(x, 4) for x in s1], [round(x, 4) for x in s2]],
            "us_per_launch": round(med * 1e3, 1), "descriptors_per_s": round(N / (med * 1e-3), 0),
            "gather_model_bytes_per_descriptor": 1920, "gather_model_TBps": round(model / (med * 1e-3) / 1e12, 3),
            "global_model_bytes_per_descriptor": glob // N, "global_model_TBps": round(glob / (med * 1e-3) / 1e12, 3),
            "guide_figure_TBps": 8.6, "guide_figure": "uniformly random 1152-B rows of a 38 MB table (Infinity Cache), gathered into LDS, chip-wide",
            "share_of_guide_figure_gather_model": round(model / (med * 1e-3) / 8.6e12, 3),
            "two_level_descriptors_per_s": round(N / (sub_med * 1e-3), 0), "voc_over_two_level_time": round(med / sub_med, 2)}, voc


def driver_inputs(args):
    """The driver leg's input streams, rendered by worker processes BEFORE this process touches the GPU (they are forked)."""
    from object_slam_amd import seqbench
    wl = seqbench.rgbd_workload(speed=1.0, n_base=8, stagger=24)
    n_frames = args.driver_preroll + 2 + args.driver_steps
    return wl, n_frames, seqbench.base_sequences(wl, 0, args.driver_seqs, n_frames, workers=min(16, os.cpu_count() or 1))


def driver_leg(args, voc, inputs):
    import torch
    from object_slam_amd import seqbench, slam
    S, G = args.driver_seqs, 4
    wl, n_frames, seqs = inputs
    out = {}
    for tag, v in (("substitute", None), ("tree_10_6", voc)):
        summ, _, systems, _ = seqbench.run_rank(wl, lambda cfg: slam.System(cfg, vocabulary=v), 0, 1, S, G, args.driver_steps, 2, True, torch.device("cuda", 0),
                                                host_threads=4, sequences=seqs, preroll=args.driver_preroll)
        sec = kfs = nd = 0
        for sy in systems:
            a, b, c = sy.bow_seconds()
            sec += a; kfs += b; nd += c
        out[tag] = {"frames_per_s": round(summ["frames_per_s"], 1), "keyframes": summ["keyframes"], "lost_frames": summ["lost_frames"], "map_violations": summ["map_violations"],
                    "compute_bow_wall_s_sum_over_handles": round(sec, 4), "compute_bow_keyframes": kfs, "compute_bow_descriptors": nd,
                    "compute_bow_us_per_keyframe": round(sec / max(kfs, 1) * 1e6, 2), "steps_total": n_frames, "handles": G}
        for sy in systems:
            sy.close()
        del systems
    return {"sequences": S, "runs": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arrays", type=int, default=8192)
    ap.add_argument("--per-array", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--driver-seqs", type=int, default=0, help="also run the driver leg with this many sequences (0 = kernel leg only)")
    ap.add_argument("--driver-steps", type=int, default=20)
    ap.add_argument("--driver-preroll", type=int, default=40)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    inputs = driver_inputs(a) if a.driver_seqs > 0 else None
    res, voc = kernel_leg(a)
    if inputs is not None:
        res["driver"] = driver_leg(a, voc, inputs)
    try:
        res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        res["commit"] = None
    res["date"] = time.strftime("%Y-%m-%d")
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
