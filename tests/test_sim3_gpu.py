"""GPU: the Sim3 solver (include/oslam_hip.h, "Sim3 solver") against the numpy restatement of tests/sim3_common.py — every hypothesis, every count, the
control flow of iterate() with its resumable state — and against the truth of generated scenes."""
import os
import subprocess

import numpy as np
import pytest

import sim3_common as sc3

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "object_slam_amd")
TOL = 1e-4   # the project's bar for poses (TOL of test_pnp_gpu.py): absolute on R, relative to the scene depth on t, relative on s
COUNTS = sc3.PARITY_COUNTS
KEYS = ("T12", "inliers", "status", "states", "iter_inliers", "hypotheses")


def _pack(scenes, seeds):
    from object_slam_amd import sim3
    pr = sim3.pack_problems([len(s["sigma2_1"]) for s in scenes], [s["K1"] for s in scenes], [s["K2"] for s in scenes], seeds, [s["fix_scale"] for s in scenes])
    cat = lambda k, w: np.concatenate([s[k].reshape(-1, w) for s in scenes]) if scenes else np.zeros((0, w), np.float32)
    return pr, (cat("X1", 3), cat("X2", 3), cat("sigma2_1", 1).reshape(-1), cat("sigma2_2", 1).reshape(-1))


def _run(solver, pr, arrays, n_iterations, states=None, **kw):
    """One call with the outputs pre-filled with a pattern; `states` (default: fresh) is updated in place.  Returns copies."""
    from object_slam_amd import sim3
    states = sim3.fresh_states(len(pr)) if states is None else states
    out = solver.iterate_batch(pr, states, *arrays, n_iterations, iter_inliers=True, hypotheses=True, T12=np.full((len(pr), 4, 4), 7.0, np.float32),
                               inliers=np.full(len(arrays[2]), 0xAB, np.uint8), **kw)
    return {k: v.copy() for k, v in out.items()}


def _same(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in KEYS)


@pytest.fixture(scope="module")
def solver():
    from object_slam_amd import sim3
    s = sim3.Sim3Solver(16, 2048, 300)
    yield s
    s.close()


@pytest.fixture(scope="module")
def batch():
    scenes = list(sc3.parity_scenes())
    pr, arrays = _pack(scenes, sc3.PARITY_SEEDS)
    return dict(scenes=scenes, seeds=sc3.PARITY_SEEDS, pr=pr, arrays=arrays)


@pytest.fixture(scope="module")
def first(solver, batch):
    """iterate(300) of fresh solvers: one call."""
    return _run(solver, batch["pr"], batch["arrays"], 300)


@pytest.fixture(scope="module")
def budget(solver, batch, first):
    """iterate(300) again and again until every problem says no_more: the list of the calls' outputs (the first is `first`)."""
    calls, states = [first], first["states"].copy()
    while not (calls[-1]["status"][:, 3] == 1).all():
        assert len(calls) <= 301
        calls.append(_run(solver, batch["pr"], batch["arrays"], 300, states=states))
    return calls


def _returns(calls, b):
    """(returning iteration, nInliers) of problem b over the calls."""
    return [(int(c["states"]["iterations_done"][b]) - 1, int(c["status"][b, 1])) for c in calls if c["status"][b, 0] == 1]


def test_hypothesis_parity_with_the_restatement(budget):
    ref = sc3.parity_reference()
    total = left_out = 0
    worst = dict(R=0.0, t=0.0, s=0.0)
    for b, (S, _) in enumerate(ref):
        counts = np.full(300, -1, np.int64)
        hyps = np.full((300, 13), np.nan, np.float32)
        for c in budget:   # every iteration is run in exactly one call
            ran = c["iter_inliers"][b] >= 0
            assert not (ran & (counts >= 0)).any()
            counts[ran], hyps[ran] = c["iter_inliers"][b][ran], c["hypotheses"][b][ran]
        assert (counts >= 0).sum() == len(S.log) == S.iterations and (counts[:S.iterations] >= 0).all()
        for e in S.log:
            total += 1
            if e["undetermined"]:
                left_out += 1
                continue
            h = hyps[e["it"]]
            dR = np.abs(h[:9].reshape(3, 3) - e["R"]).max()
            dt = np.abs(h[9:12] - e["t"]).max() / S.sc["depth"]
            ds = abs(float(h[12]) - float(e["s"])) / max(abs(float(e["s"])), 1e-30)
            worst = dict(R=max(worst["R"], dR), t=max(worst["t"], dt), s=max(worst["s"], ds))
            assert dR <= TOL and dt <= TOL and ds <= TOL, (b, e["it"], dR, dt, ds)
            assert counts[e["it"]] == e["count"], (b, e["it"], int(counts[e["it"]]), e["count"])
    print("worst |dR| %.3g, |dt| / depth %.3g, |ds| / s %.3g; left out %d of %d iterations" % (worst["R"], worst["t"], worst["s"], left_out, total))
    assert left_out * 20 <= total


def test_first_return_against_the_truth(first, batch):
    ref = sc3.parity_reference()
    for b, (N, s) in enumerate(zip(COUNTS, batch["scenes"])):
        if N < 25:
            continue
        o = int(batch["pr"]["offset"][b])
        returned, n_in, ran, no_more = first["status"][b].tolist()
        st, T, flags = first["states"][b], first["T12"][b], first["inliers"][o:o + N]
        print("N = %3d: status %s, best iteration %d" % (N, first["status"][b].tolist(), st["best_iteration"]))
        assert returned == 1 and no_more == 0 and ran == st["iterations_done"] == st["best_iteration"] + 1 and st["best_inliers"] == n_in
        assert set(flags.tolist()) <= {0, 1} and np.array_equal(flags.astype(bool), s["truth"]) and n_in == int(s["truth"].sum())
        assert np.array_equal(T[:3, :3], (st["s"] * st["R"]).astype(np.float32)) and np.array_equal(T[:3, 3], st["t"])
        assert np.array_equal(T[3], np.array([0, 0, 0, 1], np.float32))
        if s["fix_scale"]:
            assert st["s"] == np.float32(1.0)
        it_ref, n_ref, T_ref, fl_ref = ref[b][1][0]   # the pose against the restatement: a 3-point hypothesis is unrefined
        assert it_ref == ran - 1 and n_ref == n_in and np.array_equal(fl_ref, flags.astype(bool))
        dR, dt = np.abs(T[:3, :3] - T_ref[:3, :3]).max() / max(1.0, s["s"]), np.abs(T[:3, 3] - T_ref[:3, 3]).max() / s["depth"]
        print("         |d sR| / s %.3g, |dt| / depth %.3g" % (dR, dt))
        assert dR <= TOL and dt <= TOL


def test_edge_counts(first, budget, batch):
    st = first["status"]
    for b, N in enumerate(COUNTS):
        o = int(batch["pr"]["offset"][b])
        if N == 20:     # minInliers == N: one iteration, and `>` is strict
            assert st[b].tolist() == [0, 0, 1, 1] and _returns(budget, b) == []
            assert first["states"][b]["iterations_done"] == 1
        if N == 21:     # can return only with all 21
            assert all(n == 21 for _, n in _returns(budget, b))
        if N in (19, 3, 0):
            assert st[b].tolist() == [0, 0, 0, 1]
            assert first["states"][b]["iterations_done"] == 0 and first["states"][b]["best_iteration"] == -1
        if N <= 20:     # no Sim3: the caller's bytes stay
            assert (first["T12"][b] == 7.0).all() and (first["inliers"][o:o + N] == 0xAB).all()


def test_chunks_of_5_equal_one_call_of_300(solver, batch, first):
    from object_slam_amd import sim3
    states = sim3.fresh_states(len(COUNTS))
    got = {}
    for _ in range(60):
        c = _run(solver, batch["pr"], batch["arrays"], 5, states=states)
        for b in range(len(COUNTS)):
            if b not in got and (c["status"][b, 0] == 1 or c["status"][b, 3] == 1):
                got[b] = c
        if len(got) == len(COUNTS):
            break
    assert len(got) == len(COUNTS)
    for b, N in enumerate(COUNTS):
        o, c = int(batch["pr"]["offset"][b]), got[b]
        assert c["status"][b, 0] == first["status"][b, 0] and c["status"][b, 1] == first["status"][b, 1] and c["status"][b, 3] == first["status"][b, 3]
        assert np.array_equal(c["states"][b:b + 1].view(np.uint8), first["states"][b:b + 1].view(np.uint8))     # the returning iteration and the best
        assert np.array_equal(c["T12"][b].view(np.uint8), first["T12"][b].view(np.uint8)) and np.array_equal(c["inliers"][o:o + N], first["inliers"][o:o + N])


def test_resuming_gives_the_restatements_sequence_of_returns(budget):
    ref = sc3.parity_reference()
    for b, (S, returns) in enumerate(ref):
        assert _returns(budget, b) == [(it, n) for it, n, _, _ in returns], b
        last = budget[-1]["states"][b]   # (the records are carried from call to call)
        assert (last["iterations_done"], last["best_inliers"], last["best_iteration"]) == (S.iterations_done, S.best_inliers, S.best_iteration)


def _one(sc, seed):
    pr, arrays = _pack([sc], [seed])
    return pr, arrays


def test_a_return_on_the_last_iteration_is_not_no_more(solver):
    from object_slam_amd import sim3
    sc = sc3.make_scene(31, 40, outlier_frac=0.25)
    good, bad = np.nonzero(sc["truth"])[0], np.nonzero(~sc["truth"])[0]
    prm = dict(probability=0.99, min_inliers=20, max_iterations=4)
    assert sc3.ransac_params(40, **prm) == (4, False)
    samples = np.zeros((1, 4, 3), np.int32)
    samples[0, :3] = [[bad[0], bad[1], good[0]], [bad[2], good[1], bad[3]], [bad[4], bad[5], bad[6]]]
    samples[0, 3] = [good[2], good[10], good[20]]
    S = sc3.Solver(sc, 1, prm, samples[0])
    r = S.iterate(10)
    assert r["returned"] == 1 and S.iterations_done == 4 and r["no_more"] == 0     # the construction: only the last sample returns
    pr, arrays = _one(sc, 1)
    states = sim3.fresh_states(1)
    a = _run(solver, pr, arrays, 10, states=states, params=sim3.make_params(**prm), samples=samples)
    assert a["status"][0].tolist() == [1, 30, 4, 0] and np.array_equal(a["inliers"].astype(bool), sc["truth"])
    b = _run(solver, pr, arrays, 10, states=states, params=sim3.make_params(**prm), samples=samples)
    assert b["status"][0].tolist() == [0, 0, 0, 1] and (b["T12"] == 7.0).all() and (b["inliers"] == 0xAB).all()
    assert np.array_equal(b["states"].view(np.uint8), a["states"].view(np.uint8))


def test_fallback_keeps_the_last_best_when_nothing_returns(solver):
    """minInliers = the number of true inliers: `>` never holds, and every all-inlier sample ties the best, which `>=` replaces."""
    from object_slam_amd import sim3
    sc = sc3.make_scene(77, 50, outlier_frac=0.5)
    n_true = int(sc["truth"].sum())
    assert n_true == 25
    prm = dict(probability=0.99, min_inliers=n_true, max_iterations=40)
    its = sc3.ransac_params(50, **prm)[0]
    assert its == 35
    rng = np.random.default_rng(3)
    good = np.nonzero(sc["truth"])[0]
    samples = np.zeros((1, 40, 3), np.int32)
    for it in range(40):   # every second iteration draws among the true inliers
        samples[0, it] = rng.choice(good, 3, replace=False) if it % 2 else rng.choice(50, 3, replace=False)
    pr, arrays = _one(sc, 5)
    out = _run(solver, pr, arrays, 300, params=sim3.make_params(**prm), samples=samples)
    counts = out["iter_inliers"][0]
    print("fallback: status", out["status"][0].tolist(), "counts", counts[:its].tolist())
    assert out["status"][0].tolist() == [0, 0, its, 1] and (out["T12"] == 7.0).all() and (out["inliers"] == 0xAB).all()
    assert (counts[its:] == -1).all() and counts[:its].max() == n_true
    best, best_it = 0, -1
    for it in range(its):
        if counts[it] >= best:
            best, best_it = int(counts[it]), it
    st = out["states"][0]
    assert best_it == max(it for it in range(its) if counts[it] == n_true) and best_it % 2 == 1
    assert (st["iterations_done"], st["best_inliers"], st["best_iteration"]) == (its, n_true, best_it)
    assert np.array_equal(np.concatenate([st["R"].reshape(-1), st["t"], [st["s"]]]).astype(np.float32).view(np.uint8), out["hypotheses"][0, best_it].view(np.uint8))
    S = sc3.Solver(sc, 5, prm, samples[0])
    r = S.iterate(300)
    assert r["returned"] == 0 and r["no_more"] == 1 and S.best_iteration == best_it and S.best_inliers == n_true
    assert np.abs(st["R"] - S.R).max() <= TOL and np.abs(st["t"] - S.t).max() <= TOL * sc["depth"] and abs(st["s"] - S.s) <= TOL * abs(S.s)


def test_independence_and_determinism(solver, batch, first):
    from object_slam_amd import sim3
    pr, arrays = batch["pr"], batch["arrays"]
    # two calls in a row
    assert _same(_run(solver, pr, arrays, 300), first)
    # the batch reversed
    rev = _run(solver, pr[::-1].copy(), arrays, 300)
    for k in ("T12", "status", "states", "iter_inliers", "hypotheses"):
        assert np.array_equal(np.ascontiguousarray(rev[k][::-1]).view(np.uint8), first[k].view(np.uint8)), k
    assert np.array_equal(rev["inliers"], first["inliers"])
    # each problem alone
    for b, N in enumerate(COUNTS):
        o = int(pr["offset"][b])
        one = pr[b:b + 1].copy()
        one["offset"] = 0
        r = _run(solver, one, tuple(a[o:o + N] for a in arrays), 300)
        for k in ("T12", "status", "states", "iter_inliers", "hypotheses"):
            assert np.array_equal(r[k][0:1].view(np.uint8), first[k][b:b + 1].view(np.uint8)), (b, k)
        assert np.array_equal(r["inliers"], first["inliers"][o:o + N])
    # the same draws passed explicitly
    samples = np.zeros((len(pr), 300, 3), np.int32)
    for b, N in enumerate(COUNTS):
        for it in range(sc3.ransac_params(N)[0]):
            samples[b, it] = sc3.draw(batch["seeds"][b], it, N)
    assert _same(_run(solver, pr, arrays, 300, samples=samples), first)
    # the device entry point on a side stream
    assert _same(_run(solver, pr, arrays, 300, device=True), first)
    assert _same(_run(solver, pr, arrays, 300, samples=samples, device=True), first)
    # one problem without a correspondence: on the device path every per-correspondence array is an empty one, which gets a placeholder address
    from object_slam_amd import sim3
    s0 = batch["scenes"][0]
    pr0 = sim3.pack_problems([0], [s0["K1"]], [s0["K2"]], [1], [0])
    arr0 = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32))
    assert _same(_run(solver, pr0, arr0, 300, device=True), _run(solver, pr0, arr0, 300))


def test_bad_numbers_give_no_sim3_and_leave_the_neighbours_alone(solver, batch, first):
    good = [batch["scenes"][2], batch["scenes"][4]]
    coincident = sc3.make_scene(90, 30)
    coincident["X1"][:] = coincident["X1"][0]
    coincident["X2"][:] = coincident["X2"][0]
    with_nan = sc3.make_scene(91, 30)
    with_nan["X2"][3, 1] = np.nan
    scenes = [good[0], coincident, with_nan, good[1]]
    pr, arrays = _pack(scenes, [batch["seeds"][2], 5, 6, batch["seeds"][4]])
    out = _run(solver, pr, arrays, 300)
    print("status", out["status"].tolist())
    its30 = sc3.ransac_params(30)[0]
    assert out["status"][1].tolist() == [0, 0, its30, 1] and out["states"][1]["best_iteration"] == -1 and (out["iter_inliers"][1, :its30] == 0).all()
    assert out["status"][2].tolist() == [0, 0, 0, 1] and out["states"][2]["iterations_done"] == 0 and (out["iter_inliers"][2] == -1).all()
    assert (out["T12"][1:3] == 7.0).all() and (out["inliers"][60:120] == 0xAB).all()
    for here, there in ((0, 2), (3, 4)):
        N, o, oref = COUNTS[there], int(pr["offset"][here]), int(batch["pr"]["offset"][there])
        for k in ("T12", "status", "states", "iter_inliers", "hypotheses"):
            assert np.array_equal(out[k][here:here + 1].view(np.uint8), first[k][there:there + 1].view(np.uint8)), (here, k)
        assert np.array_equal(out["inliers"][o:o + N], first["inliers"][oref:oref + N])


def test_capacity_and_invalid_arguments_are_refused_before_any_launch(solver):
    from object_slam_amd import sim3
    from object_slam_amd._lib import OSLAM_E_CAPACITY, OSLAM_E_INVALID, OslamError
    pr, arrays = _one(sc3.make_scene(1, 20), 1)
    for kw, n_it in ((dict(min_inliers=-1), 5), (dict(), -1)):
        for device in (False, True):
            with pytest.raises(OslamError) as ei:
                solver.iterate_batch(pr, sim3.fresh_states(1), *arrays, n_it, sim3.make_params(**kw), device=device)
            assert ei.value.code == OSLAM_E_INVALID
    with pytest.raises(OslamError) as ei:
        solver.iterate_batch(pr, sim3.fresh_states(1), *arrays, 5, sim3.make_params(max_iterations=301))
    assert ei.value.code == OSLAM_E_CAPACITY
    small = sim3.Sim3Solver(1, 19, 300)
    with pytest.raises(OslamError) as ei:
        small.iterate_batch(pr, sim3.fresh_states(1), *arrays, 5)
    assert ei.value.code == OSLAM_E_CAPACITY
    with pytest.raises(OslamError) as ei:
        small.iterate_batch(np.concatenate([pr, pr]), sim3.fresh_states(2), *(a[:10] for a in arrays), 5)
    assert ei.value.code == OSLAM_E_CAPACITY
    small.close()


def test_adapter_program_matches_ctypes_path(tmp_path, solver):
    from object_slam_amd import build, sim3
    from object_slam_amd._lib import KP_DTYPE
    build.build_hip()
    d = str(tmp_path)
    s = sc3.make_scene(123, 80, outlier_frac=0.2, scale=1.3)
    rng = np.random.default_rng(9)
    n1, n2 = 200, 180                            # keypoints of the two keyframes; 80 of KF1's carry a usable match, 12 more are filtered out
    slots = rng.permutation(n1)[:92]
    order = np.sort(slots[:80])
    sigma2_levels = (np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)
    keys1, keys2 = np.zeros(n1, KP_DTYPE), np.zeros(n2, KP_DTYPE)
    keys1["octave"], keys2["octave"] = rng.integers(0, 8, n1), rng.integers(0, 8, n2)
    idx1, idx2 = rng.permutation(n1)[:92], rng.permutation(n2)[:92]     # GetIndexInKeyFrame of the matched points
    matched, bad1, bad2 = np.zeros(n1, np.uint8), np.zeros(n1, np.uint8), np.zeros(n1, np.uint8)
    index1, index2 = np.full(n1, -1, np.int32), np.full(n1, -1, np.int32)
    matched[slots] = 1
    index1[slots], index2[slots] = idx1, idx2
    bad1[slots[80:83]] = 1
    bad2[slots[83:86]] = 1
    index1[slots[86:89]] = -1
    index2[slots[89:92]] = -1
    pos = {int(k): j for j, k in enumerate(slots)}
    use = np.array([pos[int(k)] for k in order])
    keys1["octave"][idx1[use]] = np.round(np.log(s["sigma2_1"]) / np.log(1.2) / 2).astype(int)
    keys2["octave"][idx2[use]] = np.round(np.log(s["sigma2_2"]) / np.log(1.2) / 2).astype(int)
    # world points: Xw = Rcw^T (Xc - tcw), float32; the solver's camera-frame points are then recomputed in float32 as the adapter does
    poses = []
    for k in range(2):
        ax = rng.normal(size=3)
        poses.append((sc3.rodrigues(0.3 * ax / np.linalg.norm(ax)).astype(np.float32), rng.uniform(-1, 1, 3).astype(np.float32)))
    Xw1, Xw2 = np.ones((n1, 3), np.float32), np.ones((n1, 3), np.float32)
    Xw1[order] = ((s["X1"].astype(np.float64) - poses[0][1]) @ poses[0][0].astype(np.float64)).astype(np.float32)
    Xw2[order] = ((s["X2"].astype(np.float64) - poses[1][1]) @ poses[1][0].astype(np.float64)).astype(np.float32)
    cam = lambda P, X: np.stack([((P[0][i, 0] * X[:, 0] + P[0][i, 1] * X[:, 1]) + P[0][i, 2] * X[:, 2]) + P[1][i] for i in range(3)], 1).astype(np.float32)
    X1c, X2c = cam(poses[0], Xw1[order]), cam(poses[1], Xw2[order])
    files = dict(keys1=keys1, keys2=keys2, matched=matched, bad1=bad1, bad2=bad2, index1=index1, index2=index2, Xw1=Xw1, Xw2=Xw2, sigma2=sigma2_levels,
                 pose1=np.concatenate([poses[0][0].reshape(-1), poses[0][1]]), pose2=np.concatenate([poses[1][0].reshape(-1), poses[1][1]]))
    for name, a in files.items():
        np.ascontiguousarray(a).tofile(os.path.join(d, name + ".bin"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        for k, v in dict(fx=s["K1"][0], fy=s["K1"][1], cx=s["K1"][2], cy=s["K1"][3], seed=4242, fix_scale=0).items():
            f.write("%s %r\n" % (k, float(v)))
    prog = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adapter_sim3_program.cc"), "-o", prog,
                           "-L", LIBDIR, "-loslam_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    r = subprocess.run([prog, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    res = dict(line.split() for line in open(os.path.join(d, "out_results.txt")))
    # the ctypes path on the same correspondences: iterate(5) until a Sim3 or no_more, twice
    pr = sim3.pack_problems([80], [s["K1"]], [s["K2"]], [4242], [0])
    arrays = (X1c, X2c, sigma2_levels[keys1["octave"][idx1[use]]], sigma2_levels[keys2["octave"][idx2[use]]])
    states = sim3.fresh_states(1)
    assert int(res["N"]) == 80 and int(res["mN1"]) == n1 and int(res["maxIts"]) == sc3.ransac_params(80)[0]
    for tag in "ab":
        calls = 0
        while True:
            out = solver.iterate_batch(pr, states, *arrays, 5)
            calls += 1
            if out["status"][0, 0] == 1 or out["status"][0, 3] == 1:
                break
        returned, n_in, _, no_more = out["status"][0].tolist()
        assert returned == 1   # (the scene has 64 true inliers of 80: both rounds find a Sim3)
        assert (int(res["found_" + tag]), int(res["bNoMore_" + tag]), int(res["nInliers_" + tag]), int(res["calls_" + tag])) == (returned, no_more, n_in, calls)
        assert int(res["iterations_" + tag]) == states["iterations_done"][0]
        assert np.array_equal(np.fromfile(os.path.join(d, "out_T12_%s.bin" % tag), np.float32).view(np.uint8), out["T12"][0].reshape(-1).view(np.uint8))
        vb = np.fromfile(os.path.join(d, "out_inliers_%s.bin" % tag), np.uint8)
        assert len(vb) == n1 and np.array_equal(vb[order], out["inliers"]) and vb.sum() == n_in and not vb[np.setdiff1d(np.arange(n1), order)].any()
    assert int(res["iterations_b"]) > int(res["iterations_a"])
    best = np.fromfile(os.path.join(d, "out_best.bin"), np.float32)
    st = states[0]
    assert np.array_equal(best.view(np.uint8), np.concatenate([st["R"].reshape(-1), st["t"], [st["s"]]]).astype(np.float32).view(np.uint8))
    assert int(res["bestInliers"]) == st["best_inliers"]
