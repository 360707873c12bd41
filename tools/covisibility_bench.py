#!/usr/bin/env python3
"""Measures the device entry points of the covisibility graph (object_slam_amd/csrc/covisibility.hip): oslam_covis_apply_device,
oslam_covis_update_connections_device and oslam_covis_local_keyframes_device.

    python tools/covisibility_bench.py [--graphs 64,1024] [--keyframes 200] [--density 21]

For every number of graphs B: every graph replays the keyframe stream of tests/covisibility_common.py scaled to 200 keyframes (130 out, 70 back) of about
1000 keypoints (21 points per unit of length, at most 48 * 21 = 1008 per keyframe) in lockstep: per keyframe one apply call with its observations (B times
about 1000 OBS_ADD events, graph by graph), one update_connections call (B records, 2 B whenever k % 7 == 3) and one local_keyframes call (B records of
the keyframe's slots).  Records and outputs are resident on the device; each call is timed by the host's wall clock from the launch to the end of a stream
synchronisation.  The observation entries a call reads are computed from the stream on the host (the sum of the list lengths of the points it names).

Prints one JSON line per size: the median and the minimum over the calls of each kind, in microseconds.  No threshold is set on any of them.  Fails without
a GPU."""
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
    ap.add_argument("--graphs", default="64,1024")
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--density", type=int, default=21)
    ap.add_argument("--obs-cap", type=int, default=16)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("covisibility_bench: no GPU (there is no CPU fallback to time)")
    import covisibility_common as cc
    from object_slam_amd import covisibility as cv
    from object_slam_amd._lib import check, upload as up
    n_kf, n_out = args.keyframes, args.keyframes * cc.N_OUT // cc.N_KF
    ops = cc.stream(0, None, n_kf, n_out, args.density)[0]
    P = cc.stream_slots(n_out, args.density)
    expected, model = cc.run(ops, n_kf, cap=args.obs_cap, snapshots=False)
    assert not model.povf
    # the observation entries each operation reads, from a second pass of the restatement
    g = cc.Graph(args.obs_cap)
    entries = []
    for kind, arg in ops:
        if kind == "apply":
            entries.append(sum(len(g.obs[e[1]]) for e in arg if e[0] == cc.OBS_ADD))
            g.apply(arg)
        elif kind == "update":
            entries.append(sum(len(g.obs[p]) for _, pts, _ in arg for p in pts if p >= 0 and p not in g.pbad))
            for k, pts, excl in arg:
                g.update_record(k, pts, excl)
        else:
            entries.append(sum(len(g.obs[p]) for p in arg if p >= 0 and p not in g.pbad))
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    K = n_kf
    for B in [int(x) for x in args.graphs.split(",")]:
        h = cv.CovisibilityGraph(B, K, P, args.obs_cap)
        G = np.arange(B, dtype=np.int32)
        t = dict(apply=[], update=[], local=[])
        n_ev, n_read = dict(apply=[], update=[], local=[]), dict(apply=[], update=[], local=[])
        d_nov = up(np.zeros(B, np.int32))
        for (kind, arg), exp, ent in zip(ops, expected, entries):
            if kind == "apply":
                one = cv.pack_events([(0,) + tuple(e) for e in arg])
                ev = np.tile(one, B)
                ev["graph"] = np.repeat(G, len(one))
                d_ev = up(ev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                check(h.L.oslam_covis_apply_device(h.h, len(ev), d_ev.data_ptr(), d_nov.data_ptr(), st))
                stream.synchronize()
                t["apply"].append(time.perf_counter() - t0)
                assert not d_nov.cpu().numpy().view(np.int32)[:B].any()
                n_ev["apply"].append(len(ev))
            elif kind == "update":
                n = len(arg) * B
                rec, pts, excl = cv.pack_updates(np.repeat(G, len(arg)), [a[0] for a in arg] * B, [a[1] for a in arg] * B, [a[2] for a in arg] * B)
                d_rec, d_pts, d_excl = up(rec), up(pts), up(excl)
                d_st, d_no, d_pa, d_nl = (up(np.full(n, -9, np.int32)) for _ in range(4))
                d_oi, d_ow, d_li = (up(np.full((n, K), -1, np.int32)) for _ in range(3))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                check(h.L.oslam_covis_update_connections_device(h.h, n, d_rec.data_ptr(), len(pts), d_pts.data_ptr(), len(excl), d_excl.data_ptr(), d_st.data_ptr(),
                                                                d_oi.data_ptr(), d_ow.data_ptr(), d_no.data_ptr(), d_pa.data_ptr(), d_li.data_ptr(), d_nl.data_ptr(), st))
                stream.synchronize()
                t["update"].append(time.perf_counter() - t0)
                status = d_st.cpu().numpy().view(np.int32)[:n]
                assert status.tolist() == [r["status"] for r in exp["out"]] * B   # the restatement's statuses, in every graph
                n_ev["update"].append(n)
            else:
                rec, pts = cv.pack_local(G, [arg] * B)
                d_rec, d_pts = up(rec), up(pts)
                d_list, d_n, d_ref, d_null = up(np.full((B, K), -1, np.int32)), up(np.zeros(B, np.int32)), up(np.zeros(B, np.int32)), up(np.zeros(len(pts), np.uint8))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                check(h.L.oslam_covis_local_keyframes_device(h.h, B, d_rec.data_ptr(), len(pts), d_pts.data_ptr(), d_list.data_ptr(), d_n.data_ptr(), d_ref.data_ptr(),
                                                             d_null.data_ptr(), st))
                stream.synchronize()
                t["local"].append(time.perf_counter() - t0)
                assert (d_n.cpu().numpy().view(np.int32)[:B] == exp["out"]["n"]).all()
                n_ev["local"].append(B)
            n_read[kind].append(ent * B)
        out = dict(tool="covisibility_bench", graphs=B, keyframes=K, point_slots=P, obs_cap=args.obs_cap, keypoints_per_keyframe=int(np.median([len(a) for k, a in ops if k == "local"])),
                   bytes_per_graph=h.bytes_per_graph(K, P, args.obs_cap))
        for kind in ("apply", "update", "local"):
            name = dict(apply="apply", update="update_connections", local="local_keyframes")[kind]
            med = float(np.median(t[kind])) * 1e6
            out[name + "_us_median"] = round(med, 1)
            out[name + "_us_min"] = round(min(t[kind]) * 1e6, 1)
            out[name + "_calls"] = len(t[kind])
            out[name + "_records_per_call"] = int(np.median(n_ev[kind]))
            out[name + "_obs_entries_read_per_call"] = int(np.median(n_read[kind]))
        print(json.dumps(out), flush=True)
        h.close()


if __name__ == "__main__":
    main()
