"""GPU: the PnP solver (include/oslam_hip.h, "PnP solver") against the truth of generated scenes and against the numpy restatement of tests/pnp_common.py.
Single 4-point hypotheses are NOT compared with the restatement (their MtM has a four-dimensional null space whose basis is the eigen-solver's choice);
what is determined is: compute_pose for n >= 6, the refined pose, the inlier set and the control flow."""
import os
import subprocess

import numpy as np
import pytest

import pnp_common as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "object_slam_amd")
TOL = 1e-4   # the project's bar for poses: absolute on R, relative to the scene depth on t
COUNTS = (257, 60, 15, 10, 9, 4, 0)
KNOWN_ITERATIONS = {257: 35, 60: 35, 15: 14, 10: 1}


def _pack(scenes, seeds):
    from object_slam_amd import pnp
    pr = pnp.pack_problems([len(s["sigma2"]) for s in scenes], [s["K"] for s in scenes], seeds)
    cat = lambda k, w: np.concatenate([s[k].reshape(-1, w) for s in scenes]) if scenes else np.zeros((0, w), np.float32)
    return pr, cat("P3Dw", 3), cat("P2D", 2), cat("sigma2", 1).reshape(-1)


@pytest.fixture(scope="module")
def solver():
    from object_slam_amd import pnp
    s = pnp.PnPsolver(64, 4096, 300)   # the 36 sets of the EPnP test are its largest batch
    yield s
    s.close()


@pytest.fixture(scope="module")
def batch(solver):
    """One call over COUNTS (20 % outliers where N >= 15), outputs pre-filled with a pattern."""
    scenes = [pc.make_scene(40 + i, N, outlier_frac=0.2 if N >= 15 else 0.0) for i, N in enumerate(COUNTS)]
    seeds = [1000 + i for i in range(len(scenes))]
    pr, p3, p2, sg = _pack(scenes, seeds)
    Tcw = np.full((len(scenes), 4, 4), 7.0, np.float32)
    inl = np.full(len(sg), 0xAB, np.uint8)
    out = solver.ransac_batch(pr, p3, p2, sg, iter_inliers=True, Tcw=Tcw, inliers=inl)
    return dict(scenes=scenes, seeds=seeds, pr=pr, p3=p3, p2=p2, sg=sg, out={k: v.copy() for k, v in out.items()})


def _same(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("Tcw", "inliers", "status", "iter_inliers"))


def test_epnp_parity_with_the_restatement(solver):
    cases = [(n, noise, k) for n in (6, 7, 16, 64, 65, 257) for noise in (0.0, 0.5) for k in range(3)]
    scenes = [pc.make_scene(7000 + 10 * n + k + (5 if noise else 0), n, noise=noise) for n, noise, k in cases]
    R, t, err = solver.epnp([len(s["sigma2"]) for s in scenes], np.concatenate([s["P3Dw"] for s in scenes]), np.concatenate([s["P2D"] for s in scenes]), scenes[0]["K"])
    left_out, worst_R, worst_t = 0, 0.0, 0.0
    for (n, noise, k), s, Rg, tg, eg in zip(cases, scenes, R, t, err):
        e1, R1, t1 = pc.compute_pose(s["P3Dw"], s["P2D"], s["K"], "eigh")
        e2, R2, t2 = pc.compute_pose(s["P3Dw"], s["P2D"], s["K"], "svd")
        if max(np.abs(R1 - R2).max(), np.abs(t1 - t2).max()) > 1e-6:   # the restatement itself is not determined here
            left_out += 1
            continue
        dR, dt = np.abs(Rg - R1).max(), np.abs(tg - t1).max() / s["depth"]
        print("n = %3d noise %.1f #%d: |dR| %.3g  |dt| / depth %.3g  err %.6g (restatement %.6g)" % (n, noise, k, dR, dt, eg, e1))
        worst_R, worst_t = max(worst_R, dR), max(worst_t, dt)
        assert dR <= TOL and dt <= TOL, (n, noise, k, dR, dt)
        assert abs(eg - e1) <= 1e-3 + 1e-3 * e1
        if noise == 0.0:
            assert np.abs(Rg - s["R"]).max() <= TOL and np.abs(tg - s["t"]).max() <= TOL * s["depth"]
    print("worst |dR| %.3g, worst |dt| / depth %.3g, left out %d of %d" % (worst_R, worst_t, left_out, len(cases)))
    assert left_out * 10 <= len(cases)


def test_ransac_against_the_truth(batch):
    st, out = batch["out"]["status"], batch["out"]
    for b, (N, s) in enumerate(zip(COUNTS, batch["scenes"])):
        o = int(batch["pr"]["offset"][b])
        kind, n_in, its, chosen = st[b].tolist()
        flags, T = out["inliers"][o:o + N], out["Tcw"][b]
        print("N = %3d: kind %d, nInliers %d, iterations run %d, chosen %d" % (N, kind, n_in, its, chosen))
        if N >= 15:
            assert kind == 1
            assert np.array_equal(flags.astype(bool), s["truth"]) and set(flags.tolist()) <= {0, 1}
            assert n_in == int(s["truth"].sum())
            dR, dt = np.abs(T[:3, :3] - s["R"]).max(), np.abs(T[:3, 3] - s["t"]).max() / s["depth"]
            print("         |dR| %.3g, |dt| / depth %.3g" % (dR, dt))
            assert dR <= TOL and dt <= TOL
            assert np.array_equal(T[3], np.array([0, 0, 0, 1], np.float32))
            assert its == chosen + 1 and its <= KNOWN_ITERATIONS[N]
        elif N == 10:
            assert its == 1 and kind in (0, 2)   # Refine needs strictly more than 10
            if kind == 2:
                assert chosen == 0 and n_in == 10 and flags.tolist() == [1] * 10
        else:
            assert (kind, n_in, its, chosen) == (0, 0, 0, -1)
        if kind == 0:   # the outputs keep the fill pattern
            assert (T == 7.0).all() and (flags == 0xAB).all()


def _records(counts, min_inliers):
    rec, best = [], 0
    for it, c in enumerate(counts):
        if c >= min_inliers and c > best:
            rec.append(it)
            best = c
    return rec


def test_control_flow_replayed_from_the_counts(batch, solver):
    from object_slam_amd import pnp
    for b, N in enumerate(COUNTS):
        kind, n_in, its, chosen = batch["out"]["status"][b].tolist()
        rp = pnp.ransac_params(N)
        counts = batch["out"]["iter_inliers"][b]
        assert (counts[rp["iterations"]:] == -1).all() and (counts[:rp["iterations"]] >= 0).all()   # every hypothesis is counted, also past an early success
        if rp["no_more"]:
            assert kind == 0 and its == 0
            continue
        rec = _records(counts[:rp["iterations"] if kind != 1 else its].tolist(), rp["min_inliers"])
        assert (kind == 0) == (len(rec) == 0)
        if kind:
            assert chosen in rec
        if kind == 2:
            assert chosen == rec[-1] and its == rp["iterations"] and n_in == counts[chosen]
        if kind == 1:
            assert chosen == rec[-1] and its == chosen + 1   # the loop stopped there
    # the fallback: minInliers = the number of true inliers, so no Refine can succeed (it needs strictly more)
    s = pc.make_scene(77, 50, outlier_frac=0.54)
    n_true = int(s["truth"].sum())
    assert n_true == 23
    prm = pnp.make_params(min_inliers=n_true, max_iterations=40, epsilon=0.4)
    assert pnp.ransac_params(50, min_inliers=n_true, max_iterations=40, epsilon=0.4) == dict(min_inliers=n_true, epsilon=np.float32(n_true) / np.float32(50), iterations=40, no_more=False)
    rng = np.random.default_rng(3)
    good = np.nonzero(s["truth"])[0]
    samples = np.zeros((1, 40, 4), np.int32)
    for it in range(40):   # every second iteration draws among the true inliers
        samples[0, it] = rng.choice(good, 4, replace=False) if it % 2 else rng.choice(50, 4, replace=False)
    pr, p3, p2, sg = _pack([s], [5])
    out = solver.ransac_batch(pr, p3, p2, sg, prm, samples=samples, iter_inliers=True)
    kind, n_in, its, chosen = out["status"][0].tolist()
    counts = out["iter_inliers"][0].tolist()
    print("fallback: status", out["status"][0].tolist(), "counts", counts)
    assert kind == 2 and n_in == n_true and np.array_equal(out["inliers"].astype(bool), s["truth"]) and its == 40
    assert chosen == counts.index(n_true) and max(counts) == n_true


def test_independence_and_determinism(batch, solver):
    ref = batch["out"]
    pr, p3, p2, sg = batch["pr"], batch["p3"], batch["p2"], batch["sg"]
    fill = lambda: dict(Tcw=np.full((len(pr), 4, 4), 7.0, np.float32), inliers=np.full(len(sg), 0xAB, np.uint8))
    # two calls in a row
    assert _same(solver.ransac_batch(pr, p3, p2, sg, iter_inliers=True, **fill()), ref)
    # the batch reversed
    rev = solver.ransac_batch(pr[::-1].copy(), p3, p2, sg, iter_inliers=True, **fill())
    assert np.array_equal(rev["status"][::-1], ref["status"]) and np.array_equal(rev["iter_inliers"][::-1], ref["iter_inliers"])
    assert np.array_equal(rev["Tcw"][::-1].view(np.uint8), ref["Tcw"].view(np.uint8)) and np.array_equal(rev["inliers"], ref["inliers"])
    # each problem alone
    for b, N in enumerate(COUNTS):
        o = int(pr["offset"][b])
        one = pr[b:b + 1].copy()
        one["offset"] = 0
        r = solver.ransac_batch(one, p3[o:o + N], p2[o:o + N], sg[o:o + N], iter_inliers=True, Tcw=np.full((1, 4, 4), 7.0, np.float32), inliers=np.full(N, 0xAB, np.uint8))
        assert np.array_equal(r["status"][0], ref["status"][b]) and np.array_equal(r["iter_inliers"][0], ref["iter_inliers"][b])
        assert np.array_equal(r["Tcw"][0].view(np.uint8), ref["Tcw"][b].view(np.uint8)) and np.array_equal(r["inliers"], ref["inliers"][o:o + N])
    # the same draws passed explicitly
    samples = np.zeros((len(pr), 300, 4), np.int32)
    for b, N in enumerate(COUNTS):
        if N >= 4:
            for it in range(KNOWN_ITERATIONS.get(N, 1)):
                samples[b, it] = pc.draw(batch["seeds"][b], it, N)
    assert _same(solver.ransac_batch(pr, p3, p2, sg, samples=samples, iter_inliers=True, **fill()), ref)
    # the device entry point on a side stream
    assert _same(solver.ransac_batch(pr, p3, p2, sg, iter_inliers=True, device=True, **fill()), ref)
    # one problem without a correspondence: on the device path every per-correspondence array is an empty one, which gets a placeholder address
    pr0, p30, p20, sg0 = _pack([batch["scenes"][-1]], [1])
    assert len(pr0) == 1 and len(sg0) == 0
    fill0 = lambda: dict(Tcw=np.full((1, 4, 4), 7.0, np.float32), inliers=np.zeros(0, np.uint8))
    assert _same(solver.ransac_batch(pr0, p30, p20, sg0, iter_inliers=True, device=True, **fill0()), solver.ransac_batch(pr0, p30, p20, sg0, iter_inliers=True, **fill0()))


def test_bad_numbers_give_no_pose_and_leave_the_neighbours_alone(batch, solver):
    good = [batch["scenes"][1], batch["scenes"][2]]
    one_point = pc.make_scene(90, 30)
    one_point["P3Dw"][:] = one_point["P3Dw"][0]
    one_point["P2D"][:] = one_point["P2D"][0]
    with_nan = pc.make_scene(91, 30)
    with_nan["P3Dw"][3, 1] = np.nan
    scenes = [good[0], one_point, with_nan, good[1]]
    pr, p3, p2, sg = _pack(scenes, [batch["seeds"][1], 5, 6, batch["seeds"][2]])
    out = solver.ransac_batch(pr, p3, p2, sg, iter_inliers=True, Tcw=np.full((4, 4, 4), 7.0, np.float32), inliers=np.full(len(sg), 0xAB, np.uint8))   # (raises unless the call returns 0)
    print("status", out["status"].tolist())
    assert out["status"][1, 0] == 0 and out["status"][2, 0] == 0
    assert (out["Tcw"][1:3] == 7.0).all() and (out["inliers"][60:120] == 0xAB).all()
    ref = batch["out"]
    for here, there in ((0, 1), (3, 2)):
        N, o, oref = COUNTS[there], int(pr["offset"][here]), int(batch["pr"]["offset"][there])
        assert np.array_equal(out["status"][here], ref["status"][there]) and np.array_equal(out["iter_inliers"][here], ref["iter_inliers"][there])
        assert np.array_equal(out["Tcw"][here].view(np.uint8), ref["Tcw"][there].view(np.uint8))
        assert np.array_equal(out["inliers"][o:o + N], ref["inliers"][oref:oref + N])


def test_capacity_and_min_set_are_refused_before_any_launch(solver):
    from object_slam_amd import pnp
    from object_slam_amd._lib import OSLAM_E_CAPACITY, OSLAM_E_INVALID, OslamError
    s = pc.make_scene(1, 20)
    pr, p3, p2, sg = _pack([s], [1])
    with pytest.raises(OslamError) as ei:
        solver.ransac_batch(pr, p3, p2, sg, pnp.make_params(min_set=5))
    assert ei.value.code == OSLAM_E_INVALID
    with pytest.raises(OslamError) as ei:
        solver.ransac_batch(pr, p3, p2, sg, pnp.make_params(max_iterations=301))
    assert ei.value.code == OSLAM_E_CAPACITY
    small = pnp.PnPsolver(1, 19, 300)
    with pytest.raises(OslamError) as ei:
        small.ransac_batch(pr, p3, p2, sg)
    assert ei.value.code == OSLAM_E_CAPACITY
    with pytest.raises(OslamError) as ei:
        small.ransac_batch(np.concatenate([pr, pr]), p3[:10], p2[:10], sg[:10])
    assert ei.value.code == OSLAM_E_CAPACITY
    small.close()


def test_adapter_program_matches_ctypes_path(tmp_path, solver):
    from object_slam_amd import build, pnp
    from object_slam_amd._lib import KP_DTYPE
    build.build_hip()
    d = str(tmp_path)
    s = pc.make_scene(123, 80, outlier_frac=0.2)
    rng = np.random.default_rng(9)
    nK = 200                                     # keypoints of the frame; 80 of them carry a map point, 6 more a bad one
    slots = rng.permutation(nK)[:86]
    keys = np.zeros(nK, KP_DTYPE)
    keys["x"], keys["y"] = rng.uniform(0, 640, nK), rng.uniform(0, 480, nK)
    keys["octave"] = rng.integers(0, 8, nK)
    sigma2_levels = (np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)
    has, bad, Xw = np.zeros(nK, np.uint8), np.zeros(nK, np.uint8), np.zeros((nK, 3), np.float32)
    order = np.sort(slots[:80])
    keys["x"][order], keys["y"][order] = s["P2D"][:, 0], s["P2D"][:, 1]
    keys["octave"][order] = np.round(np.log(s["sigma2"]) / np.log(1.2) / 2).astype(int)
    has[slots] = 1
    bad[slots[80:]] = 1
    Xw[order] = s["P3Dw"]
    Xw[slots[80:]] = 1.0
    for name, a in (("keys", keys), ("has", has), ("bad", bad), ("Xw", Xw), ("sigma2", sigma2_levels)):
        np.ascontiguousarray(a).tofile(os.path.join(d, name + ".bin"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        for k, v in dict(fx=s["K"][0], fy=s["K"][1], cx=s["K"][2], cy=s["K"][3], seed=4242).items():
            f.write("%s %r\n" % (k, float(v)))
    prog = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adapter_pnp_program.cc"), "-o", prog,
                           "-L", LIBDIR, "-loslam_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    r = subprocess.run([prog, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    res = dict(line.split() for line in open(os.path.join(d, "out_results.txt")))
    # the ctypes path on the same correspondences
    pr = pnp.pack_problems([80], [s["K"]], [4242])
    out = solver.ransac_batch(pr, Xw[order], np.stack([keys["x"][order], keys["y"][order]], 1), sigma2_levels[keys["octave"][order]])
    kind, n_in, its, _ = out["status"][0].tolist()
    assert kind == 1 and int(res["N"]) == 80 and int(res["minInliers"]) == 40
    assert int(res["found"]) == 1 and int(res["bNoMore"]) == 0 and int(res["nInliers"]) == n_in == int(s["truth"].sum()) and int(res["iterations"]) == its
    assert int(res["found2"]) == 0 and int(res["noMore2"]) == 1
    assert np.array_equal(np.fromfile(os.path.join(d, "out_Tcw.bin"), np.float32).view(np.uint8), out["Tcw"][0].reshape(-1).view(np.uint8))
    vb = np.fromfile(os.path.join(d, "out_inliers.bin"), np.uint8)
    assert len(vb) == nK and np.array_equal(vb[order], out["inliers"]) and vb.sum() == n_in
