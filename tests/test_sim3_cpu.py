"""CPU: the host side of the Sim3 solver (include/oslam_hip.h, "Sim3 solver") — SetRansacParameters and the draw rule against their restatement and the
known answers — and the restatement of tests/sim3_common.py pinned against the truth, so that the GPU tests may compare with it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pnp_common as pc
import sim3_common as sc3
from object_slam_amd import pnp, sim3   # (at import: every test of this file needs the operator's module, also those that pin the restatement it is compared with)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ransac_params_known_answers_and_restatement():
    # (0.99, 20, 300): src/LoopClosing.cc:276; computed with the float32 epsilon
    for N, (it, no_more) in {19: (0, True), 20: (1, False), 21: (3, False), 25: (7, False), 60: (123, False), 257: (300, False)}.items():
        r = sim3.ransac_params(N)
        assert (r["iterations"], r["no_more"]) == (it, no_more), (N, r)
        assert sc3.ransac_params(N) == (it, no_more)
    for kw in (dict(), dict(probability=0.99, min_inliers=6, max_iterations=300), dict(probability=0.9, min_inliers=0, max_iterations=40)):
        for N in range(0, 301):
            r = sim3.ransac_params(N, **kw)
            assert (r["iterations"], r["no_more"]) == sc3.ransac_params(N, **kw), (N, kw, r)
    assert sim3.ransac_params(2, min_inliers=0)["no_more"] and not sim3.ransac_params(3, min_inliers=0)["no_more"]   # N < 3 cannot draw
    assert sim3.REFERENCE_PARAMS == dict(probability=0.99, min_inliers=20, max_iterations=300)


def test_host_functions_refuse_bad_arguments():
    from object_slam_amd._lib import OslamError
    with pytest.raises(OslamError):
        sim3.ransac_params(-1)
    with pytest.raises(OslamError):
        sim3.draw(1, 0, 2)


def test_draw_rule_and_the_pnp_draw_is_unchanged():
    assert pc.swap_with_back(6, [5, 0, 0]) == [5, 0, 4]
    assert pc.swap_with_back(3, [0, 0, 0]) == [0, 2, 1]
    for seed in (0, 1, 12345, 0xffffffff):
        for N in (3, 4, 5, 9, 60, 257, 100000):
            for it in (0, 1, 34, 299):
                d = sc3.draw(seed, it, N)
                assert len(set(d)) == 3 and all(0 <= i < N for i in d)
                assert sim3.draw(seed, it, N).tolist() == d
                if N >= 4:   # the shared generator: the first three of PnP's four draws are these, and PnP's results are what they were
                    assert pnp.draw(seed, it, N).tolist() == pc.draw(seed, it, N) and pc.draw(seed, it, N)[:3] == d
    assert len({tuple(sc3.draw(7, it, 1000)) for it in range(50)}) == 50
    assert len({tuple(sc3.draw(s, 0, 1000)) for s in range(50)}) == 50


def test_thresholds_are_truncated():
    sigma2 = (np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)
    thr = sc3.max_errors(sigma2)
    assert thr.dtype == np.float32
    assert thr.tolist() == [float(int(9.210 * float(s))) for s in sigma2]
    assert thr[:2].tolist() == [9.0, 13.0]


def test_scene_generator():
    s = sc3.make_scene(3, 60, outlier_frac=0.2, scale=1.3)
    assert all(s[k].dtype == np.float32 for k in ("X1", "X2", "sigma2_1", "sigma2_2"))
    assert (~s["truth"]).sum() == 12 and not s["fix_scale"] and s["s"] == 1.3
    assert s["X2"][:, 2].min() >= 2.0 and s["X2"][:, 2].max() <= 6.0 and s["X1"][:, 2].min() > 0.5
    assert np.abs(s["t"]).max() <= 0.3 and np.arccos((np.trace(s["R"]) - 1) / 2) <= 0.4 + 1e-9
    X1_true = 1.3 * (s["X2"].astype(np.float64) @ s["R"].T) + s["t"]
    assert np.abs(X1_true - s["X1"])[s["truth"]].max() < 1e-6
    img = lambda X: np.stack([s["K1"][2] + s["K1"][0] * X[:, 0] / X[:, 2], s["K1"][3] + s["K1"][1] * X[:, 1] / X[:, 2]], 1)
    assert np.hypot(*(img(X1_true) - img(s["X1"].astype(np.float64)))[~s["truth"]].T).min() >= 40.0 - 1e-3
    for k in ("sigma2_1", "sigma2_2"):
        assert set(np.round(np.log(s[k]) / np.log(1.2) / 2).astype(int)) <= set(range(8))
    assert sc3.make_scene(4, 30)["fix_scale"] and sc3.make_scene(4, 30)["s"] == 1.0


def test_restatement_recovers_the_truth_from_a_noise_free_sample():
    worst = 0.0
    for seed, scale in ((11, None), (12, 1.3), (13, 0.7), (14, None)):
        s = sc3.make_scene(seed, 60, outlier_frac=0.2, scale=scale)
        good = np.nonzero(s["truth"])[0]
        idx = [int(good[0]), int(good[len(good) // 2]), int(good[-1])]
        R, t, sc, gap = sc3.compute_sim3(s["X1"][idx], s["X2"][idx], s["fix_scale"])
        assert gap > 1e-3
        worst = max(worst, np.abs(R - s["R"]).max(), np.abs(t - s["t"]).max(), abs(float(sc) - s["s"]))
        flags, _, _ = sc3.check_inliers(R, t, sc, s)
        assert np.array_equal(flags, s["truth"])
        if scale is None:
            assert sc == np.float32(1.0)
    print("worst |R - R_true|, |t - t_true|, |s - s_true|: %.3g" % worst)
    assert worst < 1e-4


def test_restatement_chunks_of_5_return_where_one_call_of_300_does():
    for sc, seed in ((sc3.make_scene(21, 60, outlier_frac=0.2), 5), (sc3.make_scene(22, 25, outlier_frac=0.12, scale=1.3), 6), (sc3.make_scene(23, 20), 7)):
        _, a = sc3.run_budget(sc, seed, 5)
        S, b = sc3.run_budget(sc, seed, 300)
        assert [r[:2] for r in a] == [r[:2] for r in b]
        for ra, rb in zip(a, b):
            assert np.array_equal(ra[2], rb[2]) and np.array_equal(ra[3], rb[3])
            assert np.array_equal(ra[3], sc["truth"])
        assert S.iterations_done == S.iterations
    assert len(b) == 0 and S.iterations == 1 and S.best_inliers == 20   # N = 20 = minInliers: `>` is strict, one iteration


def test_parity_scenes_have_few_undetermined_iterations():
    """The cap the GPU parity test relies on, on the restatement alone: iterations whose count a rounding may move, or whose hypothesis the
    eigen-solver chooses (sim3_common.undetermined), are at most 5 % of all iterations of the parity batch."""
    ref = sc3.parity_reference()
    total = sum(len(S.log) for S, _ in ref)
    und = sum(1 for S, _ in ref for e in S.log if e["undetermined"])
    print("undetermined: %d of %d iterations; returns per problem: %s" % (und, total, [len(r) for _, r in ref]))
    assert total == sum(sc3.ransac_params(N)[0] for N in sc3.PARITY_COUNTS)
    assert und * 20 <= total
    for (S, returns), N, scn in zip(ref, sc3.PARITY_COUNTS, sc3.parity_scenes()):
        if N >= 25:
            assert returns and all(np.array_equal(r[3], scn["truth"]) for r in returns)


def test_struct_mirrors_have_the_sizes_of_the_header(tmp_path):
    pairs = [("oslam_sim3_params_t", sim3.Params), ("oslam_sim3_problem_t", sim3.Problem), ("oslam_sim3_state_t", sim3.State), ("oslam_sim3_ransac_t", sim3.Ransac)]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "oslam_hip.h"\nint main(void) {\n' + "".join('    printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n, _ in pairs)
                   + "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    c_sizes = dict((l.split()[0], int(l.split()[1])) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, cls in pairs:
        assert C.sizeof(cls) == c_sizes[name], (name, C.sizeof(cls), c_sizes[name])
    assert sim3.PROBLEM_DTYPE.itemsize == c_sizes["oslam_sim3_problem_t"] and sim3.STATE_DTYPE.itemsize == c_sizes["oslam_sim3_state_t"]
    st = sim3.fresh_states(3)
    assert (st["best_iteration"] == -1).all() and not st["iterations_done"].any() and not st["best_inliers"].any() and not st["R"].any()


def test_no_device_is_an_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from object_slam_amd._lib import OSLAM_E_HIP, OslamError
    with pytest.raises(OslamError) as ei:
        sim3.Sim3Solver(4, 100, 300)
    assert ei.value.code == OSLAM_E_HIP and "no CPU fallback" in str(ei.value)
