"""CPU: pins the numpy restatement of Optimizer::OptimizeEssentialGraph (tests/essential_graph_common.py) by facts that do not depend on it — the
logarithm inverts the exponential in all four branches, a consistent graph is a fixed point, the minimum scipy finds over the same residuals, what a fixed
scale, fixed vertices, duplicated edges and isolated vertices must do — and checks the host-side helpers of object_slam_amd/essential_graph.py (edge
selection, envelope) and the conditions the GPU test's comparison of Levenberg-Marquardt decisions relies on."""
import math

import numpy as np
import pytest

import essential_graph_common as egc
import sim3_opt_common as soc

BRANCH_UPDATES = {   # (|sigma| < eps, small angle): an update of each body of Sim3(Vector7d) and Sim3::log
    (False, False): [0.3, -0.2, 0.5, 1.0, 2.0, 3.0, 0.2],
    (True, False): [0.3, -0.2, 0.5, 1.0, 2.0, 3.0, 1e-7],
    (False, True): [1e-7, 2e-7, 0.0, 1.0, 2.0, 3.0, 0.2],
    (True, True): [1e-7, 0.0, -2e-7, 1.0, 2.0, 3.0, 1e-8],
}


@pytest.mark.parametrize("branch", sorted(BRANCH_UPDATES))
def test_log_inverts_exp_in_every_branch(branch):
    u = BRANCH_UPDATES[branch]
    S = soc.sim3_exp(u)
    assert soc.exp_branch(u) == branch and egc.log_branch(S) == branch
    back = egc.sim3_log1(S)
    assert np.abs(np.array(back) - u).max() <= 1e-12
    S2 = soc.sim3_exp(back)
    assert np.abs(egc.record(S2) - egc.record(S)).max() <= 1e-12


def test_log_of_a_general_sim3_is_the_matrix_logarithm():
    import scipy.linalg as sl
    S = soc.sim3_exp([0.4, 0.1, -0.7, 0.5, -1.5, 2.0, -0.3])
    M = soc.sim3_matrix(S)
    L = sl.logm(M).real
    u = egc.sim3_log1(S)
    assert abs(L[0, 0] - u[6]) < 1e-12 and abs(L[2, 1] - u[0]) < 1e-12 and abs(L[0, 2] - u[1]) < 1e-12 and abs(L[1, 0] - u[2]) < 1e-12
    assert np.abs(L[:3, 3] - u[3:6]).max() < 1e-12


def test_consistent_graph_is_a_fixed_point():
    p = egc.make_consistent()
    g = egc._Graph(p)
    F, H, b = g.build(list(g.Scw), "forward")
    assert F == 0.0 and not b.any()
    r = egc.optimize_essential_graph(p)
    assert len(r["trace"]) == 1 and r["trace"][0][2] == 0.0 and r["trace"][0][4] == 0.0 and r["status"].tolist() == [0, 5, 7, 257]
    assert all(np.array_equal(egc.record(a), egc.record(c)) for a, c in zip(r["est"], g.Scw))
    assert np.array_equal(r["Scw"][:, :9], p["Scw"][:, 1:10].astype(np.float64)) and np.array_equal(r["Scw"][:, 9:12], p["Scw"][:, 10:13].astype(np.float64))


@pytest.mark.parametrize("n", [3, 9, 17])
def test_final_cost_is_the_minimum_scipy_finds(n):
    from scipy.optimize import least_squares
    p = egc.make_ring(n, 20 + n, True)
    r = egc.optimize_essential_graph(p)
    g = r["graph"]
    final = [t for t in r["trace"] if t[4] == 1.0][-1][1]

    def estimates(x):
        est = list(g.Scw)
        for f, k in enumerate(g.free):
            est[k] = soc.sim3_oplus(g.Scw[k], list(x[6 * f:6 * f + 6]) + [0.0], True)
        return est
    sol = least_squares(lambda x: g.errors_at(estimates(x)).reshape(-1), np.zeros(6 * len(g.free)), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    cost = float((sol.fun ** 2).sum())
    print("ring %d: F0 %.6e, restatement %.9e, scipy %.9e" % (n, r["F0"], final, cost))
    assert r["F0"] > 1.5 * final and abs(final - cost) <= 1e-4 * max(1.0, cost)
    want = np.array([egc.record(S) for S in estimates(sol.x)])
    assert (np.abs(r["Scw"] - want) / np.maximum(1.0, np.abs(want))).max() <= 1e-4


def test_fix_scale_keeps_every_scale_and_a_free_scale_moves():
    p = egc.make_ring(9, 31, True)
    r = egc.optimize_essential_graph(p)
    assert np.array_equal(r["Scw"][:, 12], p["Scw"][:, 0].astype(np.float64)) and any(t[4] for t in r["trace"])
    q = egc.make_ring(9, 31, False, scale_drift=True)
    r = egc.optimize_essential_graph(q)
    moved = np.abs(r["Scw"][:, 12] - q["Scw"][:, 0].astype(np.float64))
    assert moved[0] == 0.0 and (moved[1:-1] > 1e-3).all()


def _unmoved(r, p, k):
    return np.array_equal(r["Scw"][k], egc.record(egc.sims_from_floats(p["Scw"])[k]))


def test_fixed_vertices_duplicates_and_isolated_vertices():
    # a fixed vertex in the middle, two fixed vertices: they return their input, the others move
    for fixed in ((6,), (0, 7)):
        p = egc.make_ring(12, 40, True, fixed=fixed)
        r = egc.optimize_essential_graph(p)
        assert r["status"][1] == 12 - len(fixed) and all(_unmoved(r, p, k) for k in fixed) and not any(_unmoved(r, p, k) for k in range(1, 12) if k not in fixed)
    # an edge between two fixed vertices adds to F only
    p = egc.make_ring(12, 41, True, fixed=(0, 11))   # (keyframe 11 has a non-corrected Sim3: the added edge of kind 1 has an error)
    q = dict(p, edges=np.concatenate([p["edges"], [[11, 0, 1]]]).astype(np.int32))
    g, h = egc._Graph(p), egc._Graph(q)
    F, H, b = g.build(list(g.Scw), "forward")
    F2, H2, b2 = h.build(list(h.Scw), "forward")
    assert F2 > F and np.array_equal(H, H2) and np.array_equal(b, b2)
    # a duplicated edge counts twice: F, H and b grow by that edge's share
    d = dict(p, edges=np.concatenate([p["edges"], p["edges"][5:6]]).astype(np.int32))
    one = dict(p, edges=p["edges"][5:6])
    Fd, Hd, bd = egc._Graph(d).build(list(g.Scw), "forward")
    F1, H1, b1 = egc._Graph(one).build(list(g.Scw), "forward")
    assert abs(Fd - (F + F1)) <= 1e-12 * Fd and np.allclose(Hd, H + H1, rtol=1e-12, atol=0) and np.allclose(bd, b + b1, rtol=1e-9, atol=1e-15)
    assert egc.optimize_essential_graph(d)["status"].tolist()[:3] == [0, 10, len(p["edges"]) + 1]
    # an isolated free vertex stays put (its block is lambda I, its b is zero)
    iso = egc.make_ring(9, 42, True)
    iso = dict(iso, Scw=np.concatenate([iso["Scw"], iso["Scw"][3:4]]), Snc=np.concatenate([iso["Snc"], iso["Snc"][3:4]]), has_nc=np.append(iso["has_nc"], 0).astype(np.uint8),
               fixed=np.append(iso["fixed"], 0).astype(np.uint8))
    r = egc.optimize_essential_graph(iso)
    assert r["status"][1] == 9 and _unmoved(r, iso, 9) and not _unmoved(r, iso, 4)


def test_invalid_and_empty_problems():
    p = egc.make_ring(9, 43, True)
    bad = dict(p, fixed=np.zeros(9, np.uint8))
    assert egc.optimize_essential_graph(bad)["status"].tolist() == [-1, 0, len(p["edges"]), 0]
    for k, col, v in ((2, 0, np.nan), (2, 0, 0.0), (3, 5, np.inf)):
        S = p["Scw"].copy()
        S[k, col] = v
        assert egc.optimize_essential_graph(dict(p, Scw=S))["status"][0] == -1
    e = p["edges"].copy()
    e[2, 1] = e[2, 0]
    assert egc.optimize_essential_graph(dict(p, edges=e))["status"][0] == -1
    r = egc.optimize_essential_graph(egc.empty_problem(4))
    assert r["status"].tolist() == [0, 3, 0, 0] and all(_unmoved(r, egc.empty_problem(4), k) for k in range(4))
    assert egc.optimize_essential_graph(egc.empty_problem(0))["status"].tolist() == [0, 0, 0, 0]


# ---- edge selection: one hand-built map per rule of src/Optimizer.cc:847-983 ----
def _chain(n):
    return dict(parent=[k - 1 for k in range(n)], children=[[k + 1] if k + 1 < n else [] for k in range(n)], loop_edges=[[] for _ in range(n)], covisibles=[[] for _ in range(n)],
                loop_connections={}, cur=n - 1, loop=0)


def _edges(m, weight=None):
    from object_slam_amd.essential_graph import essential_graph_edges
    a = essential_graph_edges(m["parent"], m["children"], m["loop_edges"], m["covisibles"], m["loop_connections"], m["cur"], m["loop"], weight)
    b = egc.essential_graph_edges(m["parent"], [set(c) for c in m["children"]], [set(c) for c in m["loop_edges"]], m["covisibles"], m["loop_connections"], m["cur"], m["loop"], weight)
    assert np.array_equal(a, b)
    return [tuple(int(v) for v in e) for e in a]


TREE4 = [(1, 0, 1), (2, 1, 1), (3, 2, 1)]


def test_edge_selection_rules():
    assert _edges(_chain(4)) == TREE4                                                     # the spanning tree alone, (child, parent)
    m = _chain(4); m["loop_connections"] = {3: [0, 1], 2: [0]}                              # loop connections come first, in ascending keyframe order;
    w = {(3, 0): 20, (3, 1): 100, (2, 0): 99}                                               # weight >= 100 keeps one, 99 drops one,
    assert _edges(m, lambda i, j: w[(i, j)]) == [(3, 0, 0), (3, 1, 0)] + TREE4              # and (cur, loop) is kept whatever its weight
    m = _chain(4); m["loop_connections"] = {2: [0]}
    assert _edges(m, lambda i, j: 20) == TREE4                                              # the same weight on another pair is dropped
    m = _chain(4); m["loop_edges"][3] = [0]; m["loop_edges"][0] = [3]
    assert _edges(m) == TREE4 + [(3, 0, 1)]                                                 # an old loop edge, from the larger id only, after the parent edge
    m = _chain(4); m["covisibles"][3] = [1, 0]; m["covisibles"][0] = [3]
    assert _edges(m) == TREE4 + [(3, 1, 1), (3, 0, 1)]                                      # covisibility edges to smaller ids, in the list's order
    m = _chain(4); m["covisibles"][3] = [2]; m["covisibles"][2] = [3, 1]
    assert _edges(m) == TREE4                                                               # not to the parent, not to a child (3 is 2's child; 1 is 2's parent)
    m = _chain(4); m["loop_edges"][3] = [0]; m["loop_edges"][0] = [3]; m["covisibles"][3] = [0]
    assert _edges(m) == TREE4 + [(3, 0, 1)]                                                 # not to one of this keyframe's loop edges (the loop edge itself stays)
    m = _chain(4); m["loop_connections"] = {3: [0]}; m["covisibles"][3] = [0, 1]
    assert _edges(m) == [(3, 0, 0)] + TREE4 + [(3, 1, 1)]                                   # not a pair that is in sInsertedEdges
    m = _chain(4); m["loop_connections"] = {0: [3]}; m["cur"], m["loop"] = 0, 3; m["covisibles"][3] = [0]
    assert _edges(m) == [(0, 3, 0)] + TREE4                                                 # sInsertedEdges holds (min, max): the pair is found from either end
    # duplicates the rules let through stay: only loop connections enter sInsertedEdges, so a covisible listed twice gives two edges, and a loop connection
    # that is also the parent edge gives the pair twice
    m = _chain(4); m["covisibles"][3] = [1, 1]
    assert _edges(m) == TREE4 + [(3, 1, 1), (3, 1, 1)]
    m = _chain(4); m["loop_connections"] = {3: [2]}
    assert _edges(m, lambda i, j: 150) == [(3, 2, 0)] + TREE4


def test_envelope_covers_every_edge_and_counts_its_blocks():
    from object_slam_amd import essential_graph as eg
    problems = [p for p in egc.parity_problems()]
    arrays, n_kf, n_ed = egc.concat_batch(problems)
    pr = eg.pack_problems(n_kf, n_ed, [p["fix_scale"] for p in problems])
    row_first, blocks = eg.envelope(pr, arrays["fixed"], arrays["edges"])
    for p, rec, nb in zip(problems, pr, blocks):
        o, n = rec["kf_offset"], rec["n_kf"]
        rf, fixed = row_first[o:o + n], np.asarray(p["fixed"]) != 0
        free = np.nonzero(~fixed)[0]
        first = {k: min([k] + [m for m in free if m >= rf[k]]) for k in free}
        for i, j, _ in p["edges"]:
            if not fixed[i] and not fixed[j]:
                assert first[max(i, j)] <= min(i, j)
        assert nb == sum(int(((free >= first[k]) & (free <= k)).sum()) for k in free), p["name"]
    j = [p["name"] for p in problems].index("arrow_17")
    o = pr["kf_offset"][j]
    assert row_first[o + 14:o + 17].tolist() == [1, 1, 0] and row_first[o + 13] == 10   # the arrow's last three rows are full (the last has the loop edge), the ring's are a band
    dpr, _ = eg.with_envelope(pr, arrays["fixed"], arrays["edges"])
    assert np.array_equal(dpr["env_offset"], np.concatenate([[0], np.cumsum(blocks)[:-1]])) and np.array_equal(dpr["env_blocks"], blocks)


def test_point_correction_closed_form():
    Scw = np.stack([egc.rec13(1.0, egc.rodrigues([0.1, -0.3, 0.2]), [1.0, -2.0, 0.5]), egc.rec13(1.0, np.eye(3), [0.0, 0.0, 0.0])])
    R2, t2, s2 = egc.rodrigues([-0.2, 0.1, 0.4]), np.array([0.3, 0.7, -1.1]), 1.25
    out = np.stack([np.concatenate([R2.reshape(9), t2, [s2]]), np.concatenate([np.eye(3).reshape(9), [0, 0, 0], [2.0]])])
    P = np.array([[1.0, 2.0, 3.0], [-4.0, 0.5, 8.0], [0.25, 0.5, 1.0], [9.0, 9.0, 9.0]], np.float32)
    got = egc.correct_points(Scw, out, [0, 0, 1, -1], P, P_out=np.full_like(P, 5.0))
    R1, t1 = Scw[0, 1:10].astype(np.float64).reshape(3, 3), Scw[0, 10:13].astype(np.float64)
    for m in (0, 1):
        want = R2.T @ ((R1 @ P[m].astype(np.float64) + t1) - t2) / s2
        assert np.abs(got[m] - want).max() <= 1e-6 * max(1.0, np.abs(want).max())
    assert np.array_equal(got[2], np.array([0.125, 0.25, 0.5], np.float32)) and np.array_equal(got[3], np.full(3, 5.0, np.float32))   # identity to scale 2; a skipped point


def test_parity_cases_meet_the_conditions_of_the_decision_comparison():
    """What test_essential_graph_gpu.py relies on, for the restatement alone: every case with F0 > 0 has a decisive accepted trial, the excluded trials all
    lie after the last one, forward and reversed edge order give the same poses to far below 1e-4, the fixed-scale cases first converge and then end on
    the tenth rejected trial, and the free-scale cases reject second-iteration trials by a large margin while lambda grows."""
    problems = egc.parity_problems()
    fwd, rev = egc.reference_of(problems, "parity"), egc.reference_of(problems, "parity", "reversed")
    for p, r, rv in zip(problems, fwd, rev):
        assert r["status"].tolist()[:3] == rv["status"].tolist()[:3]
        if not r["trace"] or not r["F0"] > 0:
            continue
        dec = egc.decisive_trials(r, rv)
        acc = [k for k, t in enumerate(r["trace"]) if dec[k] and t[4] == 1.0]
        assert acc, p["name"]
        assert all(k > acc[-1] for k, d in enumerate(dec) if not d), p["name"]
        assert (np.abs(r["Scw"] - rv["Scw"]) / np.maximum(1.0, np.abs(r["Scw"]))).max() < 1e-5, p["name"]
        last = r["trace"][-10:]
        if p["fix_scale"]:
            assert len(last) == 10 and all(t[4] == 0.0 for t in last) and r["trace"][-1][0] < 0.5 * r["F0"], p["name"]
            assert all(abs(t[0] - t[1]) <= 1e-9 * t[0] for t in last), p["name"]   # rejected at rounding level
        elif p["name"].startswith("free"):
            assert all(t[4] == 0.0 and t[1] > 1.05 * t[0] for t in last) and last[-1][3] > 1e6 * last[0][3], p["name"]


def test_problem_record_mirrors_the_header(tmp_path):
    import ctypes as C
    import os
    import subprocess
    from object_slam_amd import essential_graph as eg
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "oslam_hip.h"\nint main(void) { printf("%zu %zu %d\\n", sizeof(oslam_essential_graph_problem_t), '
                   'offsetof(oslam_essential_graph_problem_t, env_offset), OSLAM_ESSENTIAL_GRAPH_TRACE_ROWS); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), "-o", str(exe), str(src)])
    size, off, rows = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert C.sizeof(eg.Problem) == size == eg.PROBLEM_DTYPE.itemsize and eg.Problem.env_offset.offset == off == eg.PROBLEM_DTYPE.fields["env_offset"][1] and rows == eg.TRACE_ROWS
