"""GPU: ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (reference src/ORBmatcher.cc:522-655), mode 2 of the BoW matcher kernel, against the
restatement of tests/loop_closing_common.py, element for element: the hand cases that carry their answers, generated pairs at the sizes where the kernel
takes another path (an empty side, one keypoint, several candidates per node so that claims chain, the LDS capacity, more queries than threads), checkOri
off and on; one batch that mixes the three modes; the resident entry point; a second call."""
import ctypes as C

import numpy as np
import pytest

import loop_closing_common as lcc
from batch_common import SCALE, dev
from object_slam_amd import BowMatcher, KP_DTYPE, feature_vector
from object_slam_amd._lib import check, lib
from object_slam_amd.matcher import BowJob, BowResident

pytestmark = pytest.mark.gpu

MAX_KPS = 2400
SIGMA2 = (SCALE * SCALE).astype(np.float32)
F12 = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
GUARD = 8
KEYS = ("keys1", "desc1", "valid1", "node1", "keys2", "desc2", "valid2", "node2")


@pytest.fixture(scope="module")
def bow():
    m = BowMatcher(MAX_KPS)
    yield m
    m.close()


def test_hand_cases(bow):
    for c in lcc.bow_kf_hand_cases():
        nm, m = bow.SearchByBoWKF(*[c[k] for k in KEYS], nnratio=c["nnratio"], checkOri=c["checkOri"])
        np.testing.assert_array_equal(m, c["expect"], err_msg=c["name"])
        assert nm == c["nmatches"], c["name"]


# (N1, N2, nodes, clusters): an empty side either way, one keypoint, several candidates per node so that claims chain, the LDS capacity, nq = 1500 > 1024 threads
SIZES = [(0, 50, 5, 0), (50, 0, 5, 0), (1, 1, 1, 0), (300, 280, 40, 90), (2400, 2400, 300, 700), (1500, 900, 120, 350)]


@pytest.fixture(scope="module")
def pairs():
    rng = np.random.default_rng(77)
    out = []
    for N1, N2, nn, cl in SIZES:
        p = lcc.bow_kf_pair(rng, N1, N2, nn, clusters=cl)
        out.append((p, {ori: lcc.search_by_bow_kf(**p, nnratio=0.75, checkOri=ori) for ori in (False, True)}))
    return out


@pytest.mark.parametrize("i", range(len(SIZES)))
def test_generated_pairs(bow, pairs, i):
    p, ref = pairs[i]
    for ori in (False, True):
        nm, m = bow.SearchByBoWKF(*[p[k] for k in KEYS], nnratio=0.75, checkOri=ori)
        np.testing.assert_array_equal(m, ref[ori][1], err_msg="%s ori %d" % (SIZES[i], ori))
        assert nm == ref[ori][0]
        nm2, m2 = bow.SearchByBoWKF(*[p[k] for k in KEYS], nnratio=0.75, checkOri=ori)   # a second call gives the same bytes
        assert nm2 == nm and np.array_equal(m2, m)
    if SIZES[i][0] >= 300:
        assert ref[True][0] > 20 and (ref[True][1] == -2).any()
    if SIZES[i][0] == 300:
        # claims chain: some query was accepted on another keypoint than the one it would have taken with nothing matched before it
        chained = 0
        for q in np.nonzero(ref[False][1] >= 0)[0]:
            only = np.zeros(len(p["keys1"]), np.uint8)
            only[q] = 1
            chained += int(lcc.search_by_bow_kf(**dict(p, valid1=only), nnratio=0.75, checkOri=False)[1][q] != ref[False][1][q])
        assert chained > 0


def _job(keep, mode, p, flag1, mp2, ratio, ori, resident=False):
    job = BowJob()
    a = lambda x, dt: keep.append(np.ascontiguousarray(x, dt)) or keep[-1]
    blank = lambda x, dt: keep.append(np.zeros_like(np.ascontiguousarray(x, dt))) or keep[-1]
    pick = blank if resident else a
    qi, qn, _, _, _ = feature_vector(p["node1"])
    _, _, nodes, start, items = feature_vector(p["node2"])
    s1, s2 = job.s1, job.s2
    s1.N, s1.keys, s1.desc, s1.flag = len(p["keys1"]), pick(p["keys1"], KP_DTYPE).ctypes.data, pick(p["desc1"], np.uint8).ctypes.data, a(flag1, np.uint8).ctypes.data
    s1.nq, s1.q_idx, s1.q_node = len(qi), a(qi, np.int32).ctypes.data, a(qn, np.uint32).ctypes.data
    s2.N, s2.keys, s2.desc = len(p["keys2"]), pick(p["keys2"], KP_DTYPE).ctypes.data, pick(p["desc2"], np.uint8).ctypes.data
    s2.has_mp = a(mp2, np.uint8).ctypes.data if mode else None
    s2.nNodes, s2.nodes, s2.start, s2.items = len(nodes), a(nodes, np.uint32).ctypes.data, a(start, np.int32).ctypes.data, a(items, np.int32).ctypes.data
    job.triangulation, job.nnratio, job.checkOri = mode, ratio, int(ori)
    job.F12[:] = [float(v) for v in F12.reshape(-1)]
    job.ex, job.ey = 700.0, 240.0
    nout = s2.N if mode == 0 else s1.N
    out = a(np.full(nout + GUARD, -1, np.int32), np.int32)
    job.match, job.nmatches = out.ctypes.data, 12345
    return job, out, nout


def _run(L, h, specs, resident=None):
    keep, structs, outs = [], [], []
    for i, s in enumerate(specs):
        st, out, nout = _job(keep, *s, resident=bool(resident and resident[i] is not None))
        structs.append(st); outs.append((out, nout))
    arr = (BowJob * len(specs))(*structs)
    sf, s2 = np.ascontiguousarray(SCALE), np.ascontiguousarray(SIGMA2)
    if resident is None:
        check(L.oslam_match_bow_batch(h, len(specs), arr, C.c_void_p(sf.ctypes.data), C.c_void_p(s2.ctypes.data), 8))
    else:
        res = (BowResident * len(specs))()
        for i, r in enumerate(resident):
            if r is not None:
                res[i].d_keys1, res[i].d_desc1, res[i].d_keys2, res[i].d_desc2 = [t.data_ptr() for t in r]
        check(L.oslam_match_bow_batch_resident(h, len(specs), arr, res, C.c_void_p(sf.ctypes.data), C.c_void_p(s2.ctypes.data), 8))
    got = []
    for i, (out, nout) in enumerate(outs):
        assert (out[nout:] == -1).all()   # nothing behind match [nout]
        got.append((arr[i].nmatches, out[:nout].copy()))
    return got


def test_batch_mixes_the_three_modes(bow):
    """Six jobs, modes 0 1 2 0 1 2 in one oslam_match_bow_batch: the mode-0 and mode-1 results equal those of the same jobs sent without the mode-2 ones, the
    mode-2 results equal the single-pair entry point (and so the restatement); the resident entry point and a second call give the same bytes."""
    rng = np.random.default_rng(9)
    L, h = lib(), bow.h
    specs = []
    for mode, (N1, N2, nn) in zip([0, 1, 2, 0, 1, 2], [(200, 150, 12), (320, 400, 20), (300, 280, 40), (64, 90, 6), (17, 30, 3), (640, 600, 60)]):
        p = lcc.bow_kf_pair(rng, N1, N2, nn, clusters=(N1 // 3 if mode == 2 else 0))
        specs.append((mode, p, (rng.random(N1) < (0.4 if mode == 1 else 0.8)).astype(np.uint8), (rng.random(N2) < (0.4 if mode == 1 else 0.8)).astype(np.uint8), (0.7, 0.75, 0.9)[mode],
                      mode != 1 or N1 > 100))
    got = _run(L, h, specs)
    old = [i for i, s in enumerate(specs) if s[0] != 2]
    without = _run(L, h, [specs[i] for i in old])
    for j, i in enumerate(old):
        assert without[j][0] == got[i][0] and np.array_equal(without[j][1], got[i][1]), i
    assert all(got[i][0] > 5 for i in (0, 2, 5)), [g[0] for g in got]
    for i, s in enumerate(specs):
        if s[0] != 2:
            continue
        _, p, f1, mp2, ratio, ori = s
        nm, m = bow.SearchByBoWKF(p["keys1"], p["desc1"], f1, p["node1"], p["keys2"], p["desc2"], mp2, p["node2"], nnratio=ratio, checkOri=ori)
        rnm, rm = lcc.search_by_bow_kf(p["keys1"], p["desc1"], f1, p["node1"], p["keys2"], p["desc2"], mp2, p["node2"], nnratio=ratio, checkOri=ori)
        assert nm == got[i][0] == rnm and np.array_equal(m, got[i][1]) and np.array_equal(m, rm), i
    again = _run(L, h, specs)
    rev = _run(L, h, specs[::-1])[::-1]
    import torch
    resident = [(dev(s[1]["keys1"]), dev(s[1]["desc1"]), dev(s[1]["keys2"]), dev(s[1]["desc2"])) if i in (2, 3, 5) else None for i, s in enumerate(specs)]
    torch.cuda.synchronize()
    res = _run(L, h, specs, resident)   # the host arrays of a resident job are zeroed: the result proves which memory the kernel read
    for i in range(len(specs)):
        for other in (again, rev, res):
            assert other[i][0] == got[i][0] and np.array_equal(other[i][1], got[i][1]), i
