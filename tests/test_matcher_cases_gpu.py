"""GPU: the frame matcher's kernels (k_search_window, k_project_last, modes 0 and 1 of bow_body) on the hand-built cases of tests/matcher_common.py, against the numpy
restatements there and against the answers written in the tables: every output entry, every count and every float32 bit pattern, no tolerance.  Through the host
entry points case by case, and through the batched device entry points with the cases of one setting as the elements of one launch."""
import ctypes as C

import numpy as np
import pytest

import matcher_common as mc
from batch_common import match_frames, upload_frames
from object_slam_amd import KP_DTYPE, QUERY_DTYPE, BowMatcher, ORBmatcher
from object_slam_amd._lib import check, ptr
from object_slam_amd.matcher import feature_vector

pytestmark = pytest.mark.gpu
f32 = np.float32
MAX_KPS = MAX_Q = 1200
MAX_BATCH = 24
SEARCH = {c["name"]: c for c in mc.cached(mc.search_cases)}
PROJECT = {c["name"]: c for c in mc.cached(mc.project_last_cases)}
FUSE = {c["name"]: c for c in mc.cached(mc.fuse_cases)}
BOW = {c["name"]: c for c in mc.cached(mc.bow_cases)}
TRI = {c["name"]: c for c in mc.cached(mc.tri_cases)}
_ref = {}


def reference(c):
    """(q_match, q_dist, kp_match, nmatches, passes) of a window-search case from the restatement, computed once"""
    if c["name"] not in _ref:
        d = {}
        r = mc.restate_search(c["frame"], c["queries"], c["nnratio"], c["use_ratio"], c["check_ori"], detail=d)
        _ref[c["name"]] = r + (mc.replay_passes(c["frame"], c["queries"], d["gated"], c["nnratio"], c["use_ratio"])[0],)
    return _ref[c["name"]]


@pytest.fixture(scope="module")
def matcher():
    m = ORBmatcher(0.8, True, max_keypoints=MAX_KPS, max_queries=MAX_Q, max_batch=MAX_BATCH)
    yield m
    m.close()


@pytest.fixture(scope="module")
def bow():
    bm = BowMatcher()
    yield bm
    bm.close()


def _differs(name, got, want):
    """the outputs that differ, by name and count"""
    out = [(name, f, int((np.asarray(g) != np.asarray(w)).sum())) for f, g, w in zip(("q_match", "q_dist", "kp_match"), got[:3], want[:3]) if not np.array_equal(g, w)]
    return out + [(name, f, int(g), int(w)) for f, g, w in zip(("nmatches", "passes"), got[3:], want[3:]) if g != w]


# ---- host entry points ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SEARCH))
def test_search_window(matcher, name):
    c = SEARCH[name]
    fr, e = c["frame"], c["expect"]
    matcher.mfNNratio = c["nnratio"]
    nm, qm, qd, km = matcher.search_window(fr["k"], fr["uR"], fr["desc"], fr["blocked"], fr["bounds"], c["queries"], c["use_ratio"], c["check_ori"])
    passes = matcher.fetch(0, MAX_Q, 0, MAX_KPS, 0)[4]
    want = reference(c)
    print("%-26s n_kps %4d n_q %4d nmatches %3d (restatement %3d) passes %2d (replay %2d)" % (name, len(fr["k"]), len(c["queries"]), nm, want[3], passes, want[4]))
    assert not _differs(name, (qm, qd, km, nm, passes), want)
    assert qm.tolist() == e["qm"] and qd.tolist() == e["qd"] and km.tolist() == e["km"] and nm == e["n"] and (c["passes"] is None or passes == c["passes"])


@pytest.mark.parametrize("name", sorted(PROJECT))
def test_search_last_frame(matcher, name):
    c = PROJECT[name]
    cur, n = c["cur"], len(c["last_keys"])
    matcher.mbCheckOrientation = True
    nm, qm, qd, km = matcher.search_last_frame(cur["k"], cur["uR"], cur["desc"], cur["blocked"], cur["bounds"], c["Xw"], c["has_mp"], c["last_keys"], c["mp_desc"], c["Tcw"], c["Tlw"], c["cam"],
                                               c["sf"], c["th"], c["bMono"])
    gq = matcher.debug_queries(n, q_stride=MAX_Q)
    want_q = mc.restate_project_last(c["Xw"], c["has_mp"], c["last_keys"], c["mp_desc"], c["Tcw"], c["Tlw"], c["cam"], c["bounds"], c["sf"], c["th"], c["bMono"])
    for f in mc.FLOAT_FIELDS:
        assert mc.same_f32(gq[f], want_q[f]), (f, gq[f].tolist(), want_q[f].tolist())
    for f in mc.INT_FIELDS:
        assert np.array_equal(gq[f], want_q[f]), (f, gq[f].tolist(), want_q[f].tolist())
    assert np.array_equal(gq["desc"], want_q["desc"])       # (zeros where the keypoint does not reach the search)
    assert mc.same_records(gq, c["expect"])
    wm, wd, wk, wn = mc.restate_search(cur, want_q, 0.0, False, True)
    assert not _differs(name, (qm, qd, km, nm), (wm, wd, wk, wn))
    for row, (k, dist) in mc.PL_SEARCH[c["window"]].items():
        assert (qm[row], qd[row]) == (k, dist), (row, qm[row], qd[row])


@pytest.mark.parametrize("name", sorted(FUSE))
def test_fuse_search(matcher, name):
    c = FUSE[name]
    fr, e = c["frame"], c["expect"]
    nf, qm, qd = matcher.fuse_search(fr["k"], fr["uR"], fr["desc"], fr["bounds"], c["queries"], c["inv"])
    wm, wd, wn = mc.restate_fuse(fr, c["queries"], c["inv"])
    assert np.array_equal(qm, wm) and np.array_equal(qd, wd) and nf == wn, (qm.tolist(), wm.tolist())
    assert qm.tolist() == e["qm"] and qd.tolist() == e["qd"] and nf == e["n"]
    assert matcher.fetch(0, MAX_Q, 0, MAX_KPS, 0)[4] == 1       # no claims: one pass


@pytest.mark.parametrize("name", sorted(BOW))
def test_search_by_bow(bow, name):
    c = BOW[name]
    nm, mf = bow.SearchByBoW(c["keys1"], c["desc1"], c["valid1"], c["node1"], c["keys2"], c["desc2"], c["node2"], c["nnratio"], c["checkOri"])
    wn, wf = mc.restate_bow_frame(c["keys1"], c["desc1"], c["valid1"], feature_vector(c["node1"]), c["keys2"], c["desc2"], feature_vector(c["node2"]), c["nnratio"], c["checkOri"])
    assert np.array_equal(mf, wf) and nm == wn, (mf.tolist(), wf.tolist())
    assert mf.tolist() == c["expect"].tolist() and nm == c["n"]


@pytest.mark.parametrize("name", sorted(TRI))
def test_search_for_triangulation(bow, name):
    c = TRI[name]
    nm, m12 = bow.SearchForTriangulation(c["keys1"], c["desc1"], c["uR1"], c["mp1"], c["node1"], c["keys2"], c["desc2"], c["uR2"], c["mp2"], c["node2"], c["F12"], c["ex"], c["ey"], c["sf"],
                                         c["sigma2"], c["only_stereo"], c["checkOri"])
    wn, w12 = mc.restate_triangulation(c["keys1"], c["desc1"], c["uR1"], c["mp1"], feature_vector(c["node1"]), c["keys2"], c["desc2"], c["uR2"], c["mp2"], feature_vector(c["node2"]),
                                       c["F12"], c["ex"], c["ey"], c["sf"], c["sigma2"], c["only_stereo"], c["checkOri"])
    assert np.array_equal(m12, w12) and nm == wn, (m12.tolist(), w12.tolist())
    assert m12.tolist() == c["expect"].tolist() and nm == c["n"]


# ---- batched device entry points ----------------------------------------------------------------------------------------------------------------
def _element(frame, queries, ks, qs):
    """rows of `ks` keypoints and `qs` queries.  The rows beyond the element's counts hold a keypoint and a query that would match each other and anything near
    (100, 100): a kernel that reads beyond n_kps or n_q gives another answer."""
    nk, nq = len(frame["k"]), len(queries)
    k = np.zeros(ks, KP_DTYPE)
    k["x"], k["y"], k["class_id"] = 100.0, 100.0, -1
    k[:nk] = frame["k"]
    uR, desc, blocked = np.full(ks, -1, f32), np.zeros((ks, 32), np.uint8), np.zeros(ks, np.uint8)
    desc[:nk], blocked[:nk] = frame["desc"], frame["blocked"]
    if frame["uR"] is not None:
        uR[:nk] = frame["uR"]
    q = np.zeros(qs, QUERY_DTYPE)
    q["u"], q["v"], q["radius"], q["minLevel"], q["maxLevel"], q["flags"] = 100.0, 100.0, 50.0, -1, -1, 3
    q[:nq] = queries
    return dict(k=k, uR=uR, desc=desc, blocked=blocked, q=q, nk=nk, nq=nq)


def _groups():
    """the window-search cases by what a launch fixes: (bounds, nnratio, use_ratio, check_ori) -> cases, the first case again at the last index"""
    groups = {}
    for name in sorted(SEARCH):
        c = SEARCH[name]
        groups.setdefault((c["frame"]["bounds"], c["nnratio"], c["use_ratio"], c["check_ori"]), []).append(c)
    return {key: cs + [cs[0]] for key, cs in groups.items()}


def test_search_batch_device(matcher):
    """Every window-search case as an element of a search_batch_device launch, one launch per setting (the bounds, nnratio and the two switches are arguments of the
    launch).  The elements have different n_kps and n_q, and the first case is repeated at the last index: the per-element strides of the inputs and of the outputs
    show at b >= 1.  fetch's iterations are the passes of the replay.  (The strides of the candidate lists and of their counts do not show in any output: lists
    that overlap are written and read back by one workgroup each, through its own cache.)"""
    import torch
    groups = _groups()
    assert sum(len(cs) - 1 for cs in groups.values()) == len(SEARCH) and max(len(cs) for cs in groups.values()) <= MAX_BATCH
    bad = []
    for (bounds, nnratio, use_ratio, check_ori), cs in sorted(groups.items(), key=lambda kv: str(kv[0])):
        ks, qs = max(len(c["frame"]["k"]) for c in cs), max(len(c["queries"]) for c in cs)
        assert 1 <= ks <= MAX_KPS and 1 <= qs <= MAX_Q
        els = [_element(c["frame"], c["queries"], ks, qs) for c in cs]
        D = upload_frames(els)
        torch.cuda.synchronize()
        matcher.mfNNratio = nnratio
        matcher.search_batch_device(match_frames(D, 0, ks, bounds), D["q"].data_ptr(), qs, D["nq"].data_ptr(), 0, len(cs), use_ratio, check_ori)
        for b, (c, e) in enumerate(zip(cs, els)):
            nm, qm, qd, km, passes = matcher.fetch(b, qs, e["nq"], ks, e["nk"])
            print("bounds %s nnratio %.1f ratio %d ori %d  b %2d %-26s nmatches %3d passes %2d" % (bounds[:2], nnratio, use_ratio, check_ori, b, c["name"], nm, passes))
            bad += _differs("%s at %d" % (c["name"], b), (qm, qd, km, nm, passes), reference(c))
        assert len({(e["nk"], e["nq"]) for e in els}) > 1 or len(cs) == 2
    assert not bad, bad


def test_fuse_batch_device(matcher):
    """The Fuse case through oslam_match_fuse_batch_device at batch indices 0 and 2, with a part of it (five keypoints, four queries) between them"""
    import torch
    c = FUSE["fuse"]
    fr = c["frame"]
    part = dict(k=fr["k"][:5], uR=fr["uR"][:5], desc=fr["desc"][:5], blocked=fr["blocked"][:5], bounds=fr["bounds"])
    problems = [(fr, c["queries"]), (part, c["queries"][:4]), (fr, c["queries"])]
    ks, qs = len(fr["k"]), len(c["queries"])
    els = [_element(f, q, ks, qs) for f, q in problems]
    D = upload_frames(els)
    torch.cuda.synchronize()
    frames = match_frames(D, 0, ks, fr["bounds"])
    inv = np.ascontiguousarray(c["inv"], f32)
    check(matcher.L.oslam_match_fuse_batch_device(matcher.h, C.byref(frames), C.c_void_p(D["q"].data_ptr()), qs, C.c_void_p(D["nq"].data_ptr()), 0, len(els), ptr(inv), len(inv), None))
    for b, ((f, q), e) in enumerate(zip(problems, els)):
        nf, qm, qd, _, passes = matcher.fetch(b, qs, e["nq"], ks, e["nk"])
        wm, wd, wn = mc.restate_fuse(f, q, c["inv"])
        assert np.array_equal(qm, wm) and np.array_equal(qd, wd) and nf == wn and passes == 1, (b, qm.tolist(), wm.tolist())
    assert wn == c["expect"]["n"]
