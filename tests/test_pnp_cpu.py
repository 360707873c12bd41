"""CPU: the host side of the PnP solver (include/oslam_hip.h, "PnP solver") — SetRansacParameters and the draw rule against their restatement and the
known answers — and the restatement of tests/pnp_common.py pinned against the truth, so that the GPU tests may compare with it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pnp_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ransac_params_known_answers_and_restatement():
    from object_slam_amd import pnp
    # (0.99, 10, 300, 4, 0.5, 5.991): src/Tracking.cc:1660
    for N, (mi, it, no_more) in {60: (30, 35, False), 15: (10, 14, False), 10: (10, 1, False), 9: (10, 0, True)}.items():
        r = pnp.ransac_params(N)
        assert (r["min_inliers"], r["iterations"], r["no_more"]) == (mi, it, no_more), (N, r)
        assert pc.ransac_params(N)[0::2] == (mi, it) and pc.ransac_params(N)[3] == no_more
    for kw in (dict(), dict(probability=0.9, min_inliers=6, max_iterations=40, epsilon=0.3), dict(min_inliers=4, epsilon=0.05, max_iterations=300)):
        for N in range(4, 301):
            r = pnp.ransac_params(N, **kw)
            mi, eps, it, no_more = pc.ransac_params(N, **kw)
            assert (r["min_inliers"], r["iterations"], r["no_more"]) == (mi, it, no_more), (N, kw, r)
            assert r["epsilon"] == eps


def test_host_functions_refuse_bad_arguments():
    from object_slam_amd import pnp
    from object_slam_amd._lib import OslamError
    with pytest.raises(OslamError):
        pnp.ransac_params(-1)
    with pytest.raises(OslamError):
        pnp.draw(1, 0, 3)


def test_draw_rule():
    from object_slam_amd import pnp
    # the list 0..5, randi = 5, 0, 0, 2: take 5 (the back itself); take 0, 4 moves to slot 0; take that 4, 3 moves to slot 0; take 2
    assert pc.swap_with_back(6, [5, 0, 0, 2]) == [5, 0, 4, 2]
    assert pc.swap_with_back(4, [0, 0, 0, 0]) == [0, 3, 2, 1]
    for seed in (0, 1, 12345, 0xffffffff):
        for N in (4, 5, 9, 60, 257, 100000):
            for it in (0, 1, 34, 299):
                d = pc.draw(seed, it, N)
                assert len(set(d)) == 4 and all(0 <= i < N for i in d)
                assert pnp.draw(seed, it, N).tolist() == d
    # the draws of different iterations and seeds differ
    assert len({tuple(pc.draw(7, it, 1000)) for it in range(50)}) == 50
    assert len({tuple(pc.draw(s, 0, 1000)) for s in range(50)}) == 50


def test_scene_generator():
    s = pc.make_scene(3, 60, outlier_frac=0.2)
    assert s["P3Dw"].dtype == np.float32 and s["P2D"].dtype == np.float32 and s["sigma2"].dtype == np.float32
    assert (~s["truth"]).sum() == 12
    Xc = s["P3Dw"].astype(np.float64) @ s["R"].T + s["t"]
    assert Xc[:, 2].min() >= 2.0 - 1e-5 and Xc[:, 2].max() <= 6.0 + 1e-5
    assert np.linalg.norm(s["t"]) <= 0.3 * np.sqrt(3) and np.arccos((np.trace(s["R"]) - 1) / 2) <= 0.3 + 1e-9
    fl = pc.check_inliers(s["R"], s["t"], s["P3Dw"], s["P2D"], s["sigma2"], s["K"], 5.991)
    assert np.array_equal(fl, s["truth"])
    proj = np.stack([s["K"][2] + s["K"][0] * Xc[:, 0] / Xc[:, 2], s["K"][3] + s["K"][1] * Xc[:, 1] / Xc[:, 2]], 1)
    assert np.hypot(*(s["P2D"] - proj)[~s["truth"]].T).min() >= 20.0 - 1e-3
    assert set(np.round(np.log(s["sigma2"]) / np.log(1.2) / 2).astype(int)) <= set(range(8))


def test_restatement_compute_pose_recovers_the_true_pose():
    """Noise-free sets of n = 6 .. 79 points (inputs rounded to float32): worst difference from the true R and t measured here 3.3e-7."""
    worst = 0.0
    for n in range(6, 80):
        s = pc.make_scene(100 + n, n)
        for eig in ("eigh", "svd"):
            _, R, t = pc.compute_pose(s["P3Dw"], s["P2D"], s["K"], eig)
            worst = max(worst, np.abs(R - s["R"]).max(), np.abs(t - s["t"]).max())
    print("worst |R - R_true|, |t - t_true|: %.3g" % worst)
    assert worst < 1e-5


def test_restatement_iterate_finds_the_inlier_set():
    s = pc.make_scene(5, 60, outlier_frac=0.2)
    r = pc.iterate(s["P3Dw"], s["P2D"], s["sigma2"], s["K"], seed=11)
    assert r["kind"] == 1 and np.array_equal(r["inliers"], s["truth"]) and r["nInliers"] == 48 and r["iterations"] <= 35
    assert np.abs(r["Tcw"][:3, :3] - s["R"]).max() < 1e-4 and np.abs(r["Tcw"][:3, 3] - s["t"]).max() < 1e-4 * s["depth"]


def test_struct_mirrors_have_the_sizes_of_the_header(tmp_path):
    from object_slam_amd import pnp
    pairs = [("oslam_pnp_params_t", pnp.Params), ("oslam_pnp_problem_t", pnp.Problem), ("oslam_pnp_ransac_t", pnp.Ransac)]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "oslam_hip.h"\nint main(void) {\n' + "".join('    printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n, _ in pairs)
                   + "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    c_sizes = dict((l.split()[0], int(l.split()[1])) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, cls in pairs:
        assert C.sizeof(cls) == c_sizes[name], (name, C.sizeof(cls), c_sizes[name])
    assert pnp.PROBLEM_DTYPE.itemsize == c_sizes["oslam_pnp_problem_t"]


def test_no_device_is_an_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from object_slam_amd import pnp
    from object_slam_amd._lib import OSLAM_E_HIP, OslamError
    with pytest.raises(OslamError) as ei:
        pnp.PnPsolver(4, 100, 300)
    assert ei.value.code == OSLAM_E_HIP and "no CPU fallback" in str(ei.value)
