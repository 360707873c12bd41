"""CPU: the restatement of Optimizer::OptimizeSim3 in tests/sim3_opt_common.py against facts that do not depend on it (a series matrix exponential, a
hand-derived Jacobian, the truth of generated problems, hand-built known answers), the choice of the problems the GPU parity test uses, and the ctypes
mirrors and device-free refusals of include/oslam_hip.h, "OptimizeSim3"."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sim3_opt_common as soc
from object_slam_amd import sim3_opt   # (at import: every test of this file belongs to the operator, also those that pin the restatement it is compared with)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in soc.hand_cases()}


def _series_exp(u, terms=40):
    """exp of the 4 x 4 generator [[Omega + sigma I, upsilon], [0, 0]] by its power series: [[s R, t], [0, 1]]"""
    G = np.zeros((4, 4))
    G[:3, :3] = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]]) + u[6] * np.eye(3)
    G[:3, 3] = u[3:6]
    out, term = np.eye(4), np.eye(4)
    for k in range(1, terms):
        term = term @ G / k
        out = out + term
    return out


def test_exponential_map_equals_the_series_in_the_general_branch():
    rng = np.random.default_rng(1)
    for _ in range(20):
        u = np.concatenate([rng.uniform(-0.5, 0.5, 3), rng.uniform(-1, 1, 3), rng.uniform(-0.3, 0.3, 1)])
        assert soc.exp_branch(u) == (False, False)
        assert np.abs(soc.sim3_matrix(soc.sim3_exp(u)) - _series_exp(u)).max() < 1e-10


def test_exponential_map_reaches_its_four_branches_at_the_thresholds():
    lo, hi = 0.9e-5, 1.1e-5   # either side of eps = 1e-5
    ups = [0.3, -0.2, 0.5]
    seen = set()
    for sigma in (lo, hi):
        for theta in (lo, hi):
            u = [theta, 0.0, 0.0] + ups + [sigma]
            br = soc.exp_branch(u)
            seen.add(br)
            assert br == (sigma < soc.EPS, theta < soc.EPS)
            M, E = soc.sim3_matrix(soc.sim3_exp(u)), _series_exp(u)
            # R = I + Omega + Omega^2 has the coefficient 1 where the series has 1 / 2: theta^2 / 2 < 1e-10
            assert np.abs(M[:3, :3] - E[:3, :3]).max() < 1e-10
            if br == (False, True):
                # as published, B of this branch is ((sigma^2 / 2 - sigma + 1) s) / sigma^3 ~ 1 / sigma^3 where the series has ~ 1 / 6: with theta > 0 the
                # translation is off by ~ theta^2 / sigma^3 |upsilon|; with omega = 0 (Omega^2 = 0) the branch is exact
                assert np.abs(M[:3, 3] - E[:3, 3]).max() > 1e3
                u0 = [0.0, 0.0, 0.0] + ups + [sigma]
                assert soc.exp_branch(u0) == (False, True)
                assert np.abs(soc.sim3_matrix(soc.sim3_exp(u0)) - _series_exp(u0)).max() < 1e-10
            elif br[0]:
                # C = 1 where the series has (s - 1) / sigma = 1 + sigma / 2 + ...: off by sigma / 2 |upsilon| < eps / 2 * 0.5 (and A, B by less)
                assert np.abs(M[:3, 3] - E[:3, 3]).max() < 0.6 * soc.EPS * 0.5
            else:
                assert np.abs(M[:3, 3] - E[:3, 3]).max() < 1e-9
    assert len(seen) == 4
    # exactly at the threshold the comparisons are strict: theta == eps and |sigma| == eps take the general bodies
    assert soc.exp_branch([soc.EPS, 0, 0, 0, 0, 0, -soc.EPS]) == (False, False)


def test_sim3_product_and_inverse():
    rng = np.random.default_rng(2)
    for _ in range(10):
        S = soc.sim3_exp(np.concatenate([rng.uniform(-1, 1, 6), rng.uniform(-0.5, 0.5, 1)]))
        T = soc.sim3_exp(np.concatenate([rng.uniform(-1, 1, 6), rng.uniform(-0.5, 0.5, 1)]))
        assert np.abs(soc.sim3_matrix(soc.sim3_mul(S, soc.sim3_inv(S))) - np.eye(4)).max() < 1e-14
        assert np.abs(soc.sim3_matrix(soc.sim3_mul(S, T)) - soc.sim3_matrix(S) @ soc.sim3_matrix(T)).max() < 1e-14
        x = rng.uniform(-2, 2, 3)
        mapped = np.array(soc.quat_rot(S[0], list(x))) * S[2] + S[1]
        assert np.abs(mapped - (soc.sim3_matrix(S) @ np.append(x, 1))[:3]).max() < 1e-14
    # Eigen's matrix -> quaternion in all four cases of its trace test
    for r in ([0.1, 0.2, 0.3], [3.0, 0.1, 0.1], [0.1, 3.0, 0.1], [0.1, 0.1, 3.0]):
        R = soc.smc.rodrigues(np.array(r))
        assert np.abs(np.array(soc.quat_to_R(soc.quat_from_R(R.reshape(9)))).reshape(3, 3) - R).max() < 1e-14


def _analytic_jacobians(pb, S):
    """d e / d u of both edges under estimate <- exp(u) estimate.  y = S.map(P2): dy = [-[y]x | I | y] du; y = S^-1.map(P1): dy = -(1 / s) R^T [-[P1]x | I | P1] du."""
    R = np.array(soc.quat_to_R(S[0])).reshape(3, 3)
    skew = lambda v: np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])

    def dproj(y, k4):
        return np.array([[k4[0] / y[2], 0, -k4[0] * y[0] / y[2] ** 2], [0, k4[1] / y[2], -k4[1] * y[1] / y[2] ** 2]])
    J12, J21 = [], []
    for i in range(pb.n):
        y = S[2] * R @ pb.P2[i] + S[1]
        J12.append(-dproj(y, pb.K1) @ np.concatenate([-skew(y), np.eye(3), y[:, None]], 1))
        y = R.T @ (pb.P1[i] - S[1]) / S[2]
        J21.append(-dproj(y, pb.K2) @ (-(1 / S[2]) * R.T @ np.concatenate([-skew(pb.P1[i]), np.eye(3), pb.P1[i][:, None]], 1)))
    return np.array(J12), np.array(J21)


def test_numeric_jacobian_agrees_with_the_analytic_one():
    """delta = 1e-9 leaves the central difference the rounding of two error evaluations divided by 2e-9: a pixel coordinate below 1024 carries 2^-43 of
    rounding per operation, a handful of operations each: 8 * 2^-43 / 2e-9 < 5e-4 (the truncation error, ~ delta^2, is nothing beside it)."""
    for fix in (0, 1):
        p = soc.make_problem(31, 40, fix)
        pb = soc._Problem(p)
        S = soc.sim3_from_floats(p["s12"], p["R12"], p["t12"])
        N12, N21 = pb.jacobians(S, np.ones(pb.n, bool))
        A12, A21 = _analytic_jacobians(pb, S)
        if fix:
            assert (N12[:, :, 6] == 0).all() and (N21[:, :, 6] == 0).all()   # oplusImpl zeroes update[6]: both perturbed estimates are the same
            A12[:, :, 6] = A21[:, :, 6] = 0
        d = max(np.abs(N12 - A12).max(), np.abs(N21 - A21).max())
        print("fix_scale %d: largest |numeric - analytic| = %.3g, largest |J| = %.3g" % (fix, d, np.abs(A12).max()))
        assert d < 5e-4 and np.abs(A12).max() > 100


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_gives_the_known_answer(name):
    c = CASES[name]
    r = soc.optimize_sim3(c)
    e = c["expect"]
    assert r["ret"] == e["ret"] and r["written"] == e["written"] and r["nBad"] == e["nBad"] and r["inliers"].tolist() == list(e["inliers"])
    if "S12" in e:
        assert np.abs(r["S12"] - e["S12"]).max() <= 1e-12
    if name.startswith("exact") or name == "behind_camera":
        assert all(t[0] == 0.0 and t[1] == 0.0 for t in r["trace"])   # zero error throughout


def test_restatement_recovers_the_truth_of_generated_problems():
    """Observations are at most 0.5 pixels (times the octave's scale) off: 1e-3 rad at f = 512, 1e-4 over 100 pairs; ten times that is allowed, times the
    depth (7) for the translation.  The scale converges slower (see PARITY_SPECS): half a percent from a start 5 % off."""
    for seed, count, fix in ((17, 64, 1), (19, 129, 1), (7, 129, 0), (10, 2400, 0)):
        p = soc.make_problem(seed, count, fix)
        r = soc.optimize_sim3(p)
        eR, et, es = soc.sim3_error(r["S12"], p["truth"])
        print("%s: ret %d of %d, |dR| %.2e |dt| %.2e |ds / s| %.2e" % (p["name"], r["ret"], count, eR, et, es))
        assert np.array_equal(r["inliers"] == 0, p["gross"]) and r["ret"] == count - int(p["gross"].sum()) and r["nBad"] == int(p["gross"].sum())
        assert eR < 2e-3 and et < 1.4e-2 and es < 5e-3


def test_parity_problems_are_decided_away_from_every_threshold():
    """What makes element-for-element parity with the kernel a fair demand: in every problem of the GPU batch no chi2 is within a relative 1e-6 of th2 at
    either pass, no trial's rho is within 1e-6 of 0, and the forward, the reversed and the kernel's own edge order give the same flags, return values and
    accept sequences.  (The exact hand-built cases have F = F' = 0 in every trial — every error is exactly zero whatever the order — so their rho is
    exactly 0 by construction and not a near miss.)  Prints the largest difference of the Sim3, and of a trial's F and lambda, between the forward and the
    reversed order: the scale of reorder noise."""
    problems = soc.parity_problems()
    fwd, rev, wav = (soc.reference_of(problems, "parity", o) for o in ("forward", "reversed", "wavefront"))
    reorder, f_reorder, l_reorder = 0.0, 0.0, 0.0
    seen = dict(fix=set(), more=set(), counts=set())
    for p, a, b, w in zip(problems, fwd, rev, wav):
        for o in (b, w):
            assert a["ret"] == o["ret"] and a["nBad"] == o["nBad"] and a["written"] == o["written"] and np.array_equal(a["inliers"], o["inliers"]), p["name"]
            assert len(a["trace"]) == len(o["trace"]) and [t[4] for t in a["trace"]] == [t[4] for t in o["trace"]] and a["iterations"] == o["iterations"], p["name"]
        for r in (a, b, w):
            for c12, c21 in r["chi2"]:
                c = np.concatenate([c12, c21])
                assert len(c) == 0 or np.abs(c / float(soc.TH2) - 1.0).min() > 1e-6, p["name"]
            for t in r["trace"]:
                assert abs(t[2]) > 1e-6 or (t[0] == 0.0 and t[1] == 0.0), (p["name"], t)
        if a["written"]:
            reorder = max(reorder, float((np.abs(a["S12"] - b["S12"]) / np.maximum(1.0, np.abs(a["S12"]))).max()))
        for ta, tb in zip(a["trace"], b["trace"]):
            f_reorder = max(f_reorder, abs(ta[1] - tb[1]) / abs(ta[1]) if ta[1] != tb[1] else 0.0)
            l_reorder = max(l_reorder, abs(ta[3] - tb[3]) / abs(ta[3]) if ta[3] != tb[3] else 0.0)
        seen["counts"].add(a["count"])
        if a["written"]:
            seen["fix"].add(int(p["fix_scale"]))
            seen["more"].add(a["nBad"] > 0)
    print("largest relative difference between the forward and the reversed edge order: Sim3 %.3g, F of a trial %.3g, lambda of a trial %.3g" % (reorder, f_reorder, l_reorder))
    assert {0, 1, 9, 10, 11, 63, 64, 65, 129, 300, 2400} <= seen["counts"] and seen["fix"] == {0, 1} and seen["more"] == {False, True}
    assert reorder < 1e-5   # an order below the project's optimiser bound of 1e-4


def test_wavefront_order_is_a_reordering():
    """the kernel's order of the sums, restated: the same terms as the forward order, so on integers (every partial sum exact) the same result"""
    rng = np.random.default_rng(3)
    for m in (1, 63, 64, 65, 200):
        rows = np.sort(rng.permutation(300)[:m])
        terms = rng.integers(-1000, 1000, (m, 2, 5)).astype(np.float64)
        assert np.array_equal(soc._seq_sum(terms, "wavefront", rows), soc._seq_sum(terms, "forward")) and np.array_equal(soc._seq_sum(terms, "reversed"), terms.sum((0, 1)))
    assert np.array_equal(soc._seq_sum(np.zeros((0, 2, 3)), "wavefront", np.zeros(0, np.int64)), np.zeros(3))


def test_generator():
    p, q = soc.make_problem(5, 100, 0), soc.make_problem(5, 100, 0)
    assert all(np.array_equal(p[k], q[k]) for k in ("X3Dc1", "X3Dc2", "obs1", "obs2", "invSigma2_1", "invSigma2_2", "R12", "t12"))
    assert all(p[k].dtype == np.float32 for k in ("X3Dc1", "X3Dc2", "obs1", "obs2", "invSigma2_1", "invSigma2_2", "R12", "t12"))
    assert int(p["gross"].sum()) == 10 and abs(float(p["s12"]) / p["truth"][2] - 1) > 0.049
    R, t, s = p["truth"]
    assert np.abs(s * p["X3Dc2"].astype(np.float64) @ R.T + t - p["X3Dc1"]).max() < 1e-5
    pb = soc._Problem(dict(p, s12=s, R12=R, t12=t))
    c12, c21 = pb.chi2(soc.sim3_from_floats(s, R, t), np.ones(100, bool))
    ok = ~p["gross"]
    assert max(c12[ok].max(), c21[ok].max()) < 1.0 and np.maximum(c12, c21)[p["gross"]].min() > 600   # (float Sim3 of the truth)
    assert set(np.unique(p["invSigma2_1"])) <= set(soc.inv_level_sigma2(np.arange(8)).tolist()) and soc.inv_level_sigma2(1) == np.float32(1.0) / (np.float32(1.2) * np.float32(1.2))
    assert soc.make_problem(6, 100, 1)["s12"] == 1.0


def test_struct_mirrors_packing_and_refusals_without_a_device(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "oslam_hip.h"\nint main(void) {\n    printf("%zu %d\\n", sizeof(oslam_sim3_opt_problem_t), OSLAM_SIM3_OPT_TRACE_ROWS);\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, rows = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    assert C.sizeof(sim3_opt.Problem) == size == sim3_opt.PROBLEM_DTYPE.itemsize == 100 and rows == sim3_opt.TRACE_ROWS == 150
    pr = sim3_opt.pack_problems([3, 0, 5], [500, 501, 320, 240], [[400, 401, 300, 200]] * 3, [1.0, 1.1, 0.9], np.tile(np.eye(3), (3, 1, 1)), [[1, 2, 3]] * 3, [0, 1, 0])
    assert pr["offset"].tolist() == [0, 3, 3] and pr["th2"].tolist() == [10.0] * 3 and pr["s12"][1] == np.float32(1.1) and pr["fix_scale"].tolist() == [0, 1, 0]
    one = sim3_opt.Problem.from_buffer_copy(pr[2].tobytes())
    assert (one.count, one.offset, one.fx1, one.cy1, one.fx2, one.cy2, one.R12[4], one.R12[5], one.t12[2], one.th2, one.fix_scale) == (5, 3, 500.0, 240.0, 400.0, 200.0, 1.0, 0.0, 3.0, 10.0, 0)
    assert sim3_opt.pack_problems([2, 2], soc.K, soc.K, 1, np.eye(3), np.zeros(3), 0, offsets=[7, 0])["offset"].tolist() == [7, 0]
    # refusals that are decided before a device is looked for
    from object_slam_amd._lib import OSLAM_E_HIP, OSLAM_E_INVALID, OslamError
    for args in ((0, 100), (4, 0), (-1, 100)):
        with pytest.raises(OslamError) as ei:
            sim3_opt.Sim3Optimizer(*args)
        assert ei.value.code == OSLAM_E_INVALID
    L = sim3_opt._bind(sim3_opt.lib())
    assert L.oslam_sim3_opt_create(None, 4, 100, 0) == OSLAM_E_INVALID
    assert L.oslam_optimize_sim3_batch(None, 1, None, 0, None, None, None, None, None, None, None, None, None, None, None) == OSLAM_E_INVALID
    L.oslam_sim3_opt_destroy(None)
    import torch
    if not torch.cuda.is_available():   # without a device there is no handle: no CPU fallback
        with pytest.raises(OslamError) as ei:
            sim3_opt.Sim3Optimizer(4, 100)
        assert ei.value.code == OSLAM_E_HIP and "no CPU fallback" in str(ei.value)
