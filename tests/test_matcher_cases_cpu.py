"""CPU: the restatements of the frame matcher's searches in tests/matcher_common.py against the answers written in the case tables and against the oracle
(oracle/matcher_oracle.cc, a second transcription of the same reference text), so that the GPU tests may compare the kernels with them; that the hand-built cases are
what their comments say; that every decision of every restatement is taken by some case; and what the random inputs of tests/test_matcher_gpu.py reach."""
import collections

import numpy as np
import pytest

import matcher_common as mc
import sim3_match_common as smc
from batch_common import SCALE, bow_pair, rand_frame, rand_queries
from object_slam_amd.matcher import feature_vector

f32, f64 = np.float32, np.float64
SEARCH = {c["name"]: c for c in mc.cached(mc.search_cases)}
PROJECT = {c["name"]: c for c in mc.cached(mc.project_last_cases)}
FUSE = {c["name"]: c for c in mc.cached(mc.fuse_cases)}
BOW = {c["name"]: c for c in mc.cached(mc.bow_cases)}
TRI = {c["name"]: c for c in mc.cached(mc.tri_cases)}
FLOAT_FIELDS, INT_FIELDS, same_records = mc.FLOAT_FIELDS, mc.INT_FIELDS, mc.same_records


def _oracle_search(oracle, c, queries=None, frame=None):
    fr = c["frame"] if frame is None else frame
    nm, qm, qd, km = oracle.search_by_projection(fr["k"], fr["uR"], fr["desc"], fr["blocked"], fr["bounds"], c["queries"] if queries is None else queries, c["nnratio"], c["use_ratio"], c["check_ori"])
    return qm, qd, km, nm


def _restated(c):
    d = {}
    r = mc.restate_search(c["frame"], c["queries"], c["nnratio"], c["use_ratio"], c["check_ori"], detail=d)
    return r, d


@pytest.mark.parametrize("name", sorted(SEARCH))
def test_search_restatement_table_and_oracle_agree(oracle, name):
    c = SEARCH[name]
    (qm, qd, km, n), d = _restated(c)
    e = c["expect"]
    assert qm.tolist() == e["qm"] and qd.tolist() == e["qd"] and km.tolist() == e["km"] and n == e["n"] and d["codes"] == e["codes"]
    oqm, oqd, okm, on = _oracle_search(oracle, c)
    assert np.array_equal(oqm, qm) and np.array_equal(oqd, qd) and np.array_equal(okm, km) and on == n
    # the pass structure of the operator ends at the sequential answer, after the passes the table names
    passes, fix = mc.replay_passes(c["frame"], c["queries"], d["gated"], c["nnratio"], c["use_ratio"])
    assert np.array_equal(fix, qm) and (c["passes"] is None or passes == c["passes"]), (passes, c["passes"])
    counts = mc.candidate_counts(c["frame"], c["queries"])
    assert [int(v) for v in counts[counts >= 0]] == [len(gl) for gl, code in zip(d["gated"], d["codes"]) if code != mc.NOT_IN_VIEW]


@pytest.mark.parametrize("name", sorted(PROJECT))
def test_project_last_restatement_table_and_oracle_agree(oracle, name):
    c = PROJECT[name]
    q = mc.restate_project_last(c["Xw"], c["has_mp"], c["last_keys"], c["mp_desc"], c["Tcw"], c["Tlw"], c["cam"], c["bounds"], c["sf"], c["th"], c["bMono"])
    assert same_records(q, c["expect"]), [(f, q[f].tolist(), c["expect"][f].tolist()) for f in FLOAT_FIELDS + INT_FIELDS if not np.array_equal(q[f], c["expect"][f])]
    assert np.array_equal(q["desc"][(q["flags"] & 1) == 0], np.zeros((int(((q["flags"] & 1) == 0).sum()), 32), np.uint8))
    oq = oracle.project_last_frame(c["Xw"], c["has_mp"], c["last_keys"], c["mp_desc"], c["Tcw"], c["Tlw"], c["cam"], c["bounds"], c["sf"], c["th"], c["bMono"])
    assert same_records(oq, q)
    # the search that follows (:1394-1467, no ratio test, orientation checked): restatement == oracle, and the level windows decide as the table says
    sc = dict(frame=c["cur"], queries=q, nnratio=0.9, use_ratio=False, check_ori=True)
    (qm, qd, km, n), d = _restated(sc)
    oqm, oqd, okm, on = _oracle_search(oracle, sc)
    assert np.array_equal(oqm, qm) and np.array_equal(oqd, qd) and np.array_equal(okm, km) and on == n
    for row, (k, dist) in mc.PL_SEARCH[c["window"]].items():
        assert (qm[row], qd[row]) == (k, dist), (row, qm[row], qd[row])
    assert d["codes"][2] in (mc.WINDOW_OFF_GRID, mc.EMPTY_AREA) and qm[2] == -1      # the NaN projection finds nothing


@pytest.mark.parametrize("name", sorted(FUSE))
def test_fuse_restatement_table_and_oracle_agree(oracle, name):
    c = FUSE[name]
    d = {}
    qm, qd, n = mc.restate_fuse(c["frame"], c["queries"], c["inv"], detail=d)
    e = c["expect"]
    assert qm.tolist() == e["qm"] and qd.tolist() == e["qd"] and n == e["n"] and d["codes"] == e["codes"]
    fr = c["frame"]
    on, oqm, oqd = oracle.fuse_search(fr["k"], fr["uR"], fr["desc"], fr["bounds"], c["queries"], c["inv"])
    assert np.array_equal(oqm, qm) and np.array_equal(oqd, qd) and on == n


@pytest.mark.parametrize("name", sorted(BOW))
def test_bow_restatement_table_and_oracle_agree(oracle, name):
    c = BOW[name]
    d = {}
    n, mf = mc.restate_bow_frame(c["keys1"], c["desc1"], c["valid1"], feature_vector(c["node1"]), c["keys2"], c["desc2"], feature_vector(c["node2"]), c["nnratio"], c["checkOri"], detail=d)
    assert mf.tolist() == c["expect"].tolist() and n == c["n"] and d["codes"] == c["codes"]
    on, omf = oracle.search_by_bow(c["keys1"], c["desc1"], c["valid1"], c["node1"], c["keys2"], c["desc2"], c["node2"], c["nnratio"], c["checkOri"])
    assert np.array_equal(omf, mf) and on == n


def _tri_restated(c, detail=None):
    return mc.restate_triangulation(c["keys1"], c["desc1"], c["uR1"], c["mp1"], feature_vector(c["node1"]), c["keys2"], c["desc2"], c["uR2"], c["mp2"], feature_vector(c["node2"]),
                                    c["F12"], c["ex"], c["ey"], c["sf"], c["sigma2"], c["only_stereo"], c["checkOri"], detail=detail)


@pytest.mark.parametrize("name", sorted(TRI))
def test_triangulation_restatement_table_and_oracle_agree(oracle, name):
    c = TRI[name]
    d = {}
    n, m12 = _tri_restated(c, d)
    assert m12.tolist() == c["expect"].tolist() and n == c["n"] and d["codes"] == c["codes"]
    on, om12 = oracle.search_for_triangulation(c["keys1"], c["desc1"], c["uR1"], c["mp1"], c["node1"], c["keys2"], c["desc2"], c["uR2"], c["mp2"], c["node2"], c["F12"], c["ex"], c["ey"],
                                               c["sf"], c["sigma2"], c["only_stereo"], c["checkOri"])
    assert np.array_equal(om12, m12) and on == n


def test_cases_are_what_their_comments_say():
    pop = mc._pop
    # the float identities the tables lean on
    assert f32(0.9) * f32(50) == f32(45) and f64(f32(0.9)) * 50 < 45 and f32(0.8) * f32(50) == f32(40) and f64(f32(0.8)) * 50 > 40
    assert f64(f32(7.8)) > 7.8 and f64(mc.below(7.8)) < 7.8 and f64(f32(5.99)) < 5.99 and f64(mc.above(5.99)) > 5.99
    assert f32(15) * (f32(1) / f32(30)) == f32(0.5) and f32(0.1) * f32(10) == f32(1) and f32(1) < f32(0.1) * f32(11)
    assert mc.lcc.rot_bin(15.0, 0.0) == 1 and (mc.lcc.rot_bin(165.0, 0.0), mc.lcc.rot_bin(285.0, 0.0)) == (6, 10) and mc.lcc.rot_bin(10.0, 350.0) == 1
    assert f32(0.0) - f32(1e-6) < 0 and (f32(0.0) - f32(1e-6)) + f32(360.0) == f32(360.0) and mc.lcc.rot_bin(0.0, 1e-6) == 12 and mc.lcc.rot_bin(360.0, 0.0) == 12
    assert mc.lcc.three_maxima([0, 0, 2, 0, 2, 0, 2, 0, 2] + [0] * 21) == (2, 4, 6) and mc.lcc.three_maxima([10, 0, 0, 1, 0, 0, 1] + [0] * 23) == (0, 3, 6)
    assert mc.lcc.three_maxima([11, 0, 0, 1, 0, 0, 1] + [0] * 23) == (0, -1, -1)
    # grid: the half cell, the cells beyond the grid, the two tie cells, under both bounds
    for tag, bd in (("", mc.BOUNDS_A), ("_b", mc.BOUNDS_B)):
        g = mc.Grid(SEARCH["grid_half" + tag]["frame"]["k"], bd)
        assert (g.x[0] - g.minX) * g.invW == f32(10.5) and (g.px.tolist(), g.py.tolist()) == ([11, 10], [10, 12])
        assert np.rint(f64(10.5)) == 10     # (half to even would say column 10)
        K = SEARCH["grid_edge" + tag]["frame"]["k"]
        g = mc.Grid(K, bd)
        raw = smc._round_half_away((K["x"] - g.minX) * g.invW).astype(int).tolist(), smc._round_half_away((K["y"] - g.minY) * g.invH).astype(int).tolist()
        assert raw[0][0] == 64 and raw[0][1] == 63 and raw[1][2] == 48 and raw[1][3] == 47 and raw[0][4] == -1 and raw[0][5] == 0
        assert g.px.tolist() == [-1, 63, -1, 10, -1, 0] and K["x"][5] < g.minX          # in no cell: 0, 2, 4; keypoint 5 is outside the image and inside the grid
        q = SEARCH["grid_edge" + tag]["queries"]
        for j in (0, 1, 2):   # the keypoint that is in no cell lies inside the window
            assert abs(K["x"][2 * j] - q["u"][j]) < q["radius"][j] and abs(K["y"][2 * j] - q["v"][j]) < q["radius"][j]
        g = mc.Grid(SEARCH["tie_cells" + tag]["frame"]["k"], bd)
        assert (g.px.tolist(), g.py.tolist()) == ([11, 9], [9, 11])
        K, q = SEARCH["window_edge" + tag]["frame"]["k"], SEARCH["window_edge" + tag]["queries"]
        assert K["x"][0] - q["u"][0] == q["radius"][0] and 0 < q["radius"][1] - (K["x"][1] - q["u"][1]) < 1e-4 and K["y"][2] - q["v"][2] == q["radius"][2]
        assert 0 < q["radius"][3] - (q["v"][3] - K["y"][3]) < 1e-4
        # the chains: every query has exactly n candidates, index order is the reverse of the visiting order, n + 1 passes
        for n in (16, 17, 48, 49):
            c = SEARCH["chain_%d%s" % (n, tag)]
            _, d = _restated(c)
            assert len(d["gated"]) == n and all(len(gl) == n for gl in d["gated"]) and [k for k, _ in d["gated"][0]] == list(range(n - 1, -1, -1))
            assert [dist for _, dist in d["gated"][0]] == list(range(n, 0, -1))
            assert mc.replay_passes(c["frame"], c["queries"], d["gated"], c["nnratio"], c["use_ratio"])[0] == n + 1
    assert mc.BOUNDS_B[0] < 0 and mc.BOUNDS_B[1] < 0 and all(float(v) != int(v) for v in mc.BOUNDS_B)
    # distances
    c = SEARCH["chain"]
    dd = [[pop(c["queries"]["desc"][i], c["frame"]["desc"][k]) for k in range(5)] for i in range(5)]
    assert dd[0][0] == 0 and all(dd[j][j - 1] == 6 and dd[j][j] == 14 and min(dd[j][k] for k in range(5) if k not in (j - 1, j)) == 26 for j in range(1, 5))
    c = SEARCH["ratio_after_claim"]
    assert [[pop(c["queries"]["desc"][i], c["frame"]["desc"][k]) for k in range(3)] for i in range(2)] == [[0, 5, 15], [45, 40, 60]]
    c = SEARCH["ratio_09"]
    assert [pop(c["queries"]["desc"][0], c["frame"]["desc"][k]) for k in range(7)] == [45, 50, 45, 50, 45, 45, 45] and c["frame"]["k"]["octave"].tolist() == [0, 0, 0, 1, 0, 0, 0]
    c = SEARCH["th_high"]
    assert [pop(c["queries"]["desc"][k], c["frame"]["desc"][k]) for k in range(2)] == [100, 101]
    c = SEARCH["tie_cell30"]
    g = mc.Grid(c["frame"]["k"], mc.BOUNDS_A)
    assert set(g.px.tolist()) == {10} and set(g.py.tolist()) == {10} and len(g.px) == 30 and not np.all(np.diff(c["frame"]["k"]["x"]) > 0)
    c = SEARCH["uright"]
    assert abs(c["queries"]["ur"][0] - c["frame"]["uR"][0]) == c["queries"]["radius"][0] and abs(c["queries"]["ur"][1] - c["frame"]["uR"][1]) == mc.above(10.0)
    assert c["frame"]["uR"][2] == 0.0 and SEARCH["mono"]["frame"]["uR"] is None
    # second_stride: the chain's queries are a thread's second (index >= 1024), the chain's keypoints beyond index 1024 in the second case
    for name in ("second_stride_queries", "second_stride_keypoints"):
        c = SEARCH[name]
        assert len(c["queries"]) == 1100 and not c["queries"]["flags"][:1090].any() and (c["queries"]["flags"][1090:] == 3).all()
    assert len(SEARCH["second_stride_keypoints"]["frame"]["k"]) == 1100 and len(SEARCH["second_stride_queries"]["frame"]["k"]) == 10
    # every angle sent to the GPU is finite and inside [0, 360)
    for c in SEARCH.values():
        for a in (c["frame"]["k"]["angle"], c["queries"]["angle"]):
            assert np.isfinite(a).all() and (a >= 0).all() and (a < 360).all()
    # project_last: tlc.z a float beyond b, at b, and the projections on the bounds
    c = PROJECT["project_forward"]
    assert c["Tlw"][2, 3] == mc.above(0.5) > f32(c["cam"][5]) == PROJECT["project_at_b"]["Tlw"][2, 3] and PROJECT["project_backward"]["Tlw"][2, 3] == mc.below(-0.5)
    e = c["expect"]
    assert (e["u"][4], e["u"][6], e["v"][8], e["v"][10]) == (0.0, 640.0, 0.0, 480.0) and np.isnan(e["u"][2]) and e["flags"][2] == 1
    eb = PROJECT["project_forward_b"]["expect"]
    assert (eb["u"][5], eb["u"][7], eb["v"][9], eb["v"][11]) == (-2.0 ** -15, mc.above(640.0), -2.0 ** -16, mc.above(480.0)) and not e["flags"][[5, 7, 9, 11]].any()
    assert e["radius"][13] == f32(15.0) * mc.SF[3] and PROJECT["project_at_b"]["expect"]["radius"][14] == f32(7.0) * mc.SF[7]
    assert (e["minLevel"][12], e["maxLevel"][12]) == (0, -1) and e["flags"].tolist()[12:] == [3, 1, 3]
    # Fuse: e2 == 1 at the chi2 boundaries
    c = FUSE["fuse"]
    K, q = c["frame"]["k"], c["queries"]
    for j in (6, 7, 8, 9):
        assert (q["u"][j] - K["x"][j]) ** 2 + (q["v"][j] - K["y"][j]) ** 2 == 1.0 and K["octave"][j] == j - 6
    assert c["frame"]["uR"][6] == q["ur"][6] == 50.0 and c["frame"]["uR"][4] == 0.0 and c["frame"]["uR"][5] == -1.0
    g = mc.Grid(K, mc.BOUNDS_A)
    assert (g.px[12], g.py[12], g.px[13], g.py[13]) == (29, 8, 28, 9) and pop(c["frame"]["desc"][12], q["desc"][12]) == pop(c["frame"]["desc"][13], q["desc"][12]) == 20
    # triangulation: the epipolar boundary is decided differently by a float comparison; the epipole gate at equality
    d = mc.TRI_D
    assert d * d == f32(3.84) and f64(d * d) < 3.84 * f64(f32(1.0)) and not (d * d < f32(3.84 * 1.0)) and f64(mc.above(d) * mc.above(d)) > 3.84
    c = TRI["epipole"]
    dx = f32(c["ex"]) - c["keys2"]["x"][:3]
    assert dx[0] * dx[0] == f32(100) * mc.SF[0] and dx[1] * dx[1] < f32(100) and f32(100) < dx[2] * dx[2] < f32(100) * mc.SF[1]
    c = TRI["epipolar"]
    assert mc.check_dist_epipolar_line(c["keys1"][0], c["keys2"][0], c["F12"], c["sigma2"]) is True and mc.check_dist_epipolar_line(c["keys1"][1], c["keys2"][1], c["F12"], c["sigma2"]) is False
    assert mc.check_dist_epipolar_line(TRI["den_zero"]["keys1"][0], TRI["den_zero"]["keys2"][0], TRI["den_zero"]["F12"], c["sigma2"]) is None


def _coverage():
    out = {}
    cnt = collections.Counter()
    for c in SEARCH.values():
        cnt.update(_restated(c)[1]["codes"])
    out["search"] = (len(SEARCH), mc.SEARCH_CODES, cnt)
    cnt = collections.Counter()
    for c in FUSE.values():
        d = {}
        mc.restate_fuse(c["frame"], c["queries"], c["inv"], detail=d)
        cnt.update(d["codes"])
    out["fuse"] = (len(FUSE), mc.FUSE_CODES, cnt)
    cnt = collections.Counter()
    for c in BOW.values():
        d = {}
        mc.restate_bow_frame(c["keys1"], c["desc1"], c["valid1"], feature_vector(c["node1"]), c["keys2"], c["desc2"], feature_vector(c["node2"]), c["nnratio"], c["checkOri"], detail=d)
        cnt.update(d["codes"])
    out["bow"] = (len(BOW), mc.BOW_CODES, cnt)
    cnt = collections.Counter()
    for c in TRI.values():
        d = {}
        _tri_restated(c, d)
        cnt.update(d["codes"])
    out["tri"] = (len(TRI), mc.TRI_CODES, cnt)
    return out


def test_every_decision_is_taken_by_some_case():
    for op, (n_cases, codes, cnt) in _coverage().items():
        print("%s: %d cases; %s" % (op, n_cases, ", ".join("%s %d" % (k, cnt[k]) for k in codes)))
        assert all(cnt[k] >= 1 for k in codes), (op, cnt)
        assert dict(cnt) == WANT_COVERAGE[op], (op, dict(cnt))
    names = [c["name"] for c in mc.cached(mc.project_last_cases)]
    print("project_last: %d cases: %s" % (len(names), ", ".join(names)))
    flags = np.stack([PROJECT[n]["expect"]["flags"] for n in names])
    assert (flags == 0).any() and (flags == 1).any() and (flags == 3).any()
    windows = {(int(PROJECT[n]["expect"]["minLevel"][13]), int(PROJECT[n]["expect"]["maxLevel"][13])) for n in names}
    assert windows == {(3, -1), (0, 3), (2, 4)}


# the number of queries (keypoints of side 1) that end at each decision, over all hand-built cases of an operator: a case that stops taking its decision shows here
WANT_COVERAGE = dict(
    search=dict(NOT_IN_VIEW=2180, WINDOW_OFF_GRID=8, EMPTY_AREA=8, ALL_SKIPPED=2, TOO_FAR=1, RATIO=4, ACCEPTED=396, ACCEPTED_OVER_NONBLOCKING=2, ROT_REMOVED=9),
    fuse=dict(NOT_IN_VIEW=1, EMPTY_AREA=1, ALL_GATED_LEVEL=2, ALL_GATED_CHI2=3, TOO_FAR=1, ACCEPTED=8),
    bow=dict(NO_MAPPOINT=1, NODE_ABSENT=2, TOO_FAR=2, RATIO=1, ACCEPTED=20, ROT_REMOVED=1),
    tri=dict(HAS_MAPPOINT=1, NOT_STEREO=1, NODE_ABSENT=1, NO_CANDIDATE=1, TOO_FAR=1, EPIPOLE=2, DEN_ZERO=1, EPIPOLAR=1, ACCEPTED=24, ROT_REMOVED=1))


@pytest.mark.parametrize("seed", range(4))
def test_restatements_equal_the_oracle_on_small_random_inputs(oracle, seed):
    rng = np.random.default_rng(700 + seed)
    N, M = [(300, 400), (200, 333), (120, 50), (257, 129)][seed]
    k, uR, desc = rand_frame(rng, N, clustered=(seed % 2 == 1))
    blocked = (rng.random(N) < 0.1).astype(np.uint8)
    q = rand_queries(rng, k, uR, desc, M, 0.08, few_desc=(seed == 1))
    for bounds in (mc.BOUNDS_A, mc.BOUNDS_B):
        fr = dict(k=k, uR=uR, desc=desc, blocked=blocked, bounds=bounds)
        for use_ratio, check_ori in ((True, False), (False, True)):
            c = dict(frame=fr, queries=q, nnratio=0.8, use_ratio=use_ratio, check_ori=check_ori)
            (qm, qd, km, n), d = _restated(c)
            oqm, oqd, okm, on = _oracle_search(oracle, c)
            assert np.array_equal(oqm, qm) and np.array_equal(oqd, qd) and np.array_equal(okm, km) and on == n and (n > 0 or N < 100)
            passes, fix = mc.replay_passes(fr, q, d["gated"], 0.8, use_ratio)
            assert np.array_equal(fix, qm)
        # Fuse over the same frame
        qf = q.copy()
        qf["radius"] = (3.0 * SCALE[np.clip(qf["maxLevel"], 0, 7)]).astype(f32)
        inv = (1.0 / (SCALE * SCALE)).astype(f32)
        fqm, fqd, fn = mc.restate_fuse(fr, qf, inv)
        on, oqm, oqd = oracle.fuse_search(k, uR, desc, bounds, qf, inv)
        assert np.array_equal(oqm, fqm) and np.array_equal(oqd, fqd) and on == fn
    # the BoW-guided searches
    N1, N2, nn = [(300, 280, 40), (200, 300, 12), (50, 80, 5), (257, 129, 60)][seed]
    k1, uR1, d1, node1, k2, uR2, d2, node2 = bow_pair(rng, N1, N2, nn)
    valid1 = (rng.random(N1) < 0.8).astype(np.uint8)
    for ratio, ori in ((0.7, True), (0.9, False)):
        n, mf = mc.restate_bow_frame(k1, d1, valid1, feature_vector(node1), k2, d2, feature_vector(node2), ratio, ori)
        on, omf = oracle.search_by_bow(k1, d1, valid1, node1, k2, d2, node2, ratio, ori)
        assert np.array_equal(omf, mf) and on == n
    mp1, mp2 = (rng.random(N1) < 0.4).astype(np.uint8), (rng.random(N2) < 0.4).astype(np.uint8)
    F12 = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], f32) + rng.normal(0, 1e-7, (3, 3)).astype(f32)
    sigma2 = (SCALE * SCALE).astype(f32)
    for only_stereo in (False, True):
        n, m12 = mc.restate_triangulation(k1, d1, uR1, mp1, feature_vector(node1), k2, d2, uR2, mp2, feature_vector(node2), F12, 700.0, 240.0, SCALE, sigma2, only_stereo, True)
        on, om12 = oracle.search_for_triangulation(k1, d1, uR1, mp1, node1, k2, d2, uR2, mp2, node2, F12, 700.0, 240.0, SCALE, sigma2, only_stereo, True)
        assert np.array_equal(om12, m12) and on == n


def test_what_the_random_gpu_inputs_reach():
    """From the restatement's candidate test alone: how many queries of the inputs of tests/test_matcher_gpu.py::test_search_window_random have more candidates than
    the register cache (16) and than the candidate list (48) of the kernel holds.  Seeds 1, 4 and 5 get past 48, at N = 800 .. 2400, and no seed says which path a
    failure is on: that is what the chain_16 / 17 / 48 / 49 cases are for."""
    beyond = {}
    for seed in range(6):
        rng = np.random.default_rng(seed)
        N, M = [(1000, 1500), (2000, 4000), (300, 50), (1, 1), (2400, 4096), (800, 3000)][seed]
        k, uR, desc = rand_frame(rng, N, clustered=(seed % 2 == 1))
        blocked = (rng.random(N) < 0.1).astype(np.uint8)
        q = rand_queries(rng, k, uR, desc, M, 0.08, few_desc=(seed in (1, 5)))
        counts = mc.candidate_counts(dict(k=k, uR=uR, desc=desc, blocked=blocked, bounds=mc.BOUNDS_A), q)
        beyond[seed] = (int((counts > 16).sum()), int((counts > 48).sum()), int(counts.max()))
        print("seed %d: N %4d M %4d: %4d queries with more than 16 candidates, %4d with more than 48, at most %d" % ((seed, N, M) + beyond[seed]))
    assert all(beyond[s][0] > 0 for s in (0, 1, 4, 5)) and beyond[3][:2] == (0, 0)
    assert all(beyond[s][1] > 0 for s in (1, 4, 5)) and all(beyond[s][1] == 0 for s in (0, 2, 3))
