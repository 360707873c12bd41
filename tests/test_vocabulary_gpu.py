"""GPU: the vocabulary kernel (oslam_voc_transform_device) against the numpy restatement of tests/voc_common.py and against the host descent; real extractor
output through transform / vectors into SearchByBoW; the tracking driver over the HIP operator table against the oracle's table, both with a vocabulary;
the dataset runner with a vocabulary file; the C++ adapter's ORBVocabulary against the ctypes path.  All ids are compared for equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import voc_common as V
from object_slam_amd import slam
from object_slam_amd.vocabulary import Vocabulary, save_text

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "object_slam_amd")
sys.path.insert(0, os.path.join(ROOT, "examples"))

CASES = {"A": V.tree_A, "B": V.tree_B, "C20x2": lambda: V.trees_C()[0], "C3x10": lambda: V.trees_C()[1], "D": lambda: V.tree_D(0)}
_cache = {}


def tree(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def load(t, tmp_path, name="voc.txt"):
    p = str(tmp_path / name)
    save_text(p, *t.arrays())
    return Vocabulary.load(p), p


@pytest.mark.parametrize("name", list(CASES))
def test_transform_device_matches_the_restatement(name, tmp_path):
    """Batches of 4 arrays with counts {stride, 17, 0, 1}, strides 300 and 2400, levelsup in {0, 2, 4, L, L + 1}."""
    t = tree(name)
    v, _ = load(t, tmp_path)
    feats, n_ties = V.make_descriptors(t, 2400 + 17 + 1, seed=6)
    order = np.random.default_rng(1).permutation(len(feats))      # (ties and centres spread over the arrays)
    feats = feats[order]
    levelsups = sorted({0, 2, 4, t.L, t.L + 1})
    want, paths = V.ref_transform_many(t, feats, levelsups)
    assert n_ties >= 2
    if name == "B":
        assert any(len(p) < t.L for p in paths)      # leaves above nid_level
    for stride in (300, 2400):
        pick = [np.arange(0, stride), np.arange(2400, 2417), np.arange(0, 0), np.arange(2417, 2418)]
        for lu in levelsups:
            word, node, weight = v.transform([feats[i] for i in pick], levelsup=lu, stride=stride)
            for a, idx in enumerate(pick):
                assert np.array_equal(word[a], want[lu][0][idx]), (stride, lu, a)
                assert np.array_equal(node[a], want[lu][1][idx]), (stride, lu, a)
                assert np.array_equal(weight[a].view(np.uint64), want[lu][2][idx].view(np.uint64)), (stride, lu, a)
            # nothing is written beyond an array's count
            fw, fn, fwt = v._last_full
            for a, idx in enumerate(pick):
                assert (fw[a, len(idx):] == 0xffffffff).all() and (fn[a, len(idx):] == 0xffffffff).all() and np.isnan(fwt[a, len(idx):]).all()
    # the host-pointer entry point runs the same kernel
    w1, n1, wt1 = v.transform_array(feats[:500], levelsup=4)
    assert np.array_equal(w1, want[4][0][:500]) and np.array_equal(n1, want[4][1][:500]) and np.array_equal(wt1, want[4][2][:500])


def test_transform_device_matches_the_host_descent_on_50000_descriptors(tmp_path):
    t = tree("B")
    v, _ = load(t, tmp_path)
    rng = np.random.default_rng(77)
    feats = rng.integers(0, 256, (50000, 32), dtype=np.uint8)
    near = t.desc[rng.integers(0, t.n, 25000)].copy()                 # half of them near centres: deep paths, twins
    near ^= np.packbits(rng.random((25000, 256)) < 0.04, axis=1)
    feats[25000:] = near
    arrays = [feats[i * 2000:(i + 1) * 2000] for i in range(25)]
    for lu in (0, 4):
        word, node, weight = v.transform(arrays, levelsup=lu, stride=2000)
        hw, hn, hwt = v.transform_host(feats, levelsup=lu)
        assert np.array_equal(np.concatenate(word), hw) and np.array_equal(np.concatenate(node), hn)
        assert np.array_equal(np.concatenate(weight).view(np.uint64), hwt.view(np.uint64))
    assert len(set(hw.tolist())) > 3000


def test_real_descriptors_through_transform_vectors_and_search_by_bow(oracle, tmp_path):
    """Descriptors of two synthetic frames -> transform (kernel) -> vectors -> oslam_match_search_by_bow with those FeatureVectors; the oracle matcher's
    SearchByBoW on the same FeatureVectors must give the same matches, index for index (as test_matcher_gpu.test_search_by_bow does with seeded ones)."""
    import ctypes as C
    from object_slam_amd import ORBextractor, feature_vector, synth
    from object_slam_amd._lib import check, lib, ptr
    from object_slam_amd.matcher import BowSide1, BowSide2
    t = tree("B")
    v, _ = load(t, tmp_path)
    frames, _ = synth.make_stream(2, 640, 480, seed=21)
    ex = ORBextractor(1000, 1.2, 8, 20, 7, 640, 480)
    k1, d1 = ex(frames[0])
    k2, d2 = ex(frames[1])
    sides = []
    for d in (d1, d2):
        word, node, weight = v.transform(d, levelsup=4)
        hw, hn, _ = v.transform_host(d, levelsup=4)
        assert np.array_equal(word, hw) and np.array_equal(node, hn) and (weight > 0).all()
        bi, bv, fn, fs, fi = v.vectors(word, node, weight)
        qi, qn, nodes, start, items = feature_vector(node)      # B has no zero-weight word: the FeatureVector holds every keypoint
        assert np.array_equal(fi, qi) and np.array_equal(fn, nodes) and np.array_equal(fs, start) and len(fn) > 10
        assert abs(bv.sum() - 1.0) < 1e-12
        sides.append((node, fn, fs, fi, np.repeat(fn, np.diff(fs)).astype(np.uint32)))
    valid1 = np.ones(len(k1), np.uint8)
    L = lib()
    bow = C.c_void_p()
    check(L.oslam_bow_create(C.byref(bow), 2400, 0))
    k1c, d1c, k2c, d2c = np.ascontiguousarray(k1), np.ascontiguousarray(d1), np.ascontiguousarray(k2), np.ascontiguousarray(d2)
    s1, s2 = BowSide1(), BowSide2()
    s1.N, s1.keys, s1.desc, s1.flag = len(k1c), k1c.ctypes.data, d1c.ctypes.data, valid1.ctypes.data
    s1.nq, s1.q_idx, s1.q_node = len(sides[0][3]), sides[0][3].ctypes.data, sides[0][4].ctypes.data
    s2.N, s2.keys, s2.desc = len(k2c), k2c.ctypes.data, d2c.ctypes.data
    s2.nNodes, s2.nodes, s2.start, s2.items = len(sides[1][1]), sides[1][1].ctypes.data, sides[1][2].ctypes.data, sides[1][3].ctypes.data
    for ratio, ori in ((0.7, True), (0.9, False)):
        out = np.full(len(k2c), -1, np.int32)
        nm = C.c_int(0)
        check(L.oslam_match_search_by_bow(bow, C.byref(s1), C.byref(s2), C.c_float(ratio), int(ori), ptr(out), C.byref(nm)))
        onm, omf = oracle.search_by_bow(k1, d1, valid1, sides[0][0], k2, d2, sides[1][0], ratio, ori)
        assert np.array_equal(out, omf)
        assert nm.value == onm and onm > 50, onm
    L.oslam_bow_destroy(bow)


@pytest.mark.parametrize("lm", [slam.LM_SYNC, slam.LM_DEFERRED], ids=["sync", "deferred"])
def test_hip_driver_matches_oracle_driver_with_a_vocabulary(oracle, lm, tmp_path):
    """test_slam_driver_gpu.test_hip_driver_matches_oracle_driver with vocabulary B set on both sides (HIP table: voc_nodes_keyed = the kernel over the
    resident descriptors; oracle table: the host descent) — the same comparisons and tolerances; a third run without a vocabulary equals a handle that
    never heard of one."""
    from slam_common import H, W, ate, make_streams, oracle_ops, run
    t = tree("B")
    v, _ = load(t, tmp_path)
    n, S = 30, 3
    streams = make_streams(S, n)
    cfg = slam.make_config(W, H, S, local_mapping=lm)
    hip = slam.System(cfg, vocabulary=v)
    ph, sh = run(hip, streams, n)
    cfg_o = slam.make_config(W, H, S, local_mapping=lm)
    ora = slam.System(cfg_o, oracle_ops(cfg_o), vocabulary=v)
    po, so = run(ora, streams, n)
    assert np.array_equal(sh, so) and (sh == slam.OK).all()
    level2 = {i for i in range(1, t.n + 1) if t.depth[i] == 2}
    for s in range(S):
        a, b = hip.stats(s), ora.stats(s)
        assert a["map_violations"] == 0
        assert a == b, (s, a, b)     # same keyframes, points, fusions, cullings, inlier counts
        ah, Th = ate(hip, cfg, streams, s)
        ao, To = ate(ora, cfg_o, streams, s)
        assert ah < 0.01 and ao < 0.01
        assert np.abs(Th - To).max() < 2e-4, np.abs(Th - To).max()      # 1e-4 relative on a ~2 m scene
        for kf in range(a["keyframes_created"]):     # the same FeatureVector nodes, and nodes of B at depth L - 4
            nh, no = hip.debug_bow_nodes(s, kf), ora.debug_bow_nodes(s, kf)
            assert len(nh) > 0 and set(nh.tolist()) <= level2
            assert len(no) == 0 or np.array_equal(nh, no)
    d = np.abs(ph - po).max()
    assert d < 2e-4, d
    # vocabulary=None: today's result exactly
    plain = slam.System(slam.make_config(W, H, S, local_mapping=lm))
    pp, sp = run(plain, streams, n)
    none = slam.System(slam.make_config(W, H, S, local_mapping=lm), vocabulary=None)
    none.set_vocabulary(None)
    pn, sn = run(none, streams, n)
    assert np.array_equal(pp, pn) and np.array_equal(sp, sn)
    for s in range(S):
        assert plain.stats(s) == none.stats(s)
        assert np.array_equal(plain.trajectory(s)[1], none.trajectory(s)[1])
        ids = np.concatenate([none.debug_bow_nodes(s, kf) for kf in range(none.stats(s)["keyframes_created"])])
        assert ids.min() >= 11 and ids.max() <= 110


def test_rgbd_tum_runner_loads_and_reports_the_vocabulary(tmp_path, capsys):
    import rgbd_tum
    from dataset_layout import write_tum_sequence
    from object_slam_amd import scene
    n = 10
    q = scene.make_rgbd_sequence(0, n, speed=2.0)
    root = str(tmp_path / "seq")
    sp, ap, stamps = write_tum_sequence(root, q, slam.TUM2, n)
    t = tree("A")
    _, vp = load(t, tmp_path, "ORBvoc.txt")
    out = str(tmp_path / "out")
    assert rgbd_tum.main([vp, sp, root, ap, "--out", out, "--no-sleep"]) == 0
    txt = capsys.readouterr().out
    assert "Loading ORB Vocabulary" in txt and "Vocabulary loaded!" in txt and vp in txt and "1110 nodes" in txt and "substitute" not in txt
    assert np.loadtxt(os.path.join(out, "CameraTrajectory.txt"), ndmin=2).shape == (n, 8)
    # a path that does not exist: the substitute, and a line that says so
    assert rgbd_tum.main([str(tmp_path / "none.txt"), sp, root, ap, "--out", out, "--no-sleep"]) == 0
    assert "substitute vocabulary" in capsys.readouterr().out
    # a file that exists and does not parse: exit code 1 with the reference's message
    bad = tmp_path / "bad.txt"
    bad.write_text("\n".join(open(vp).read().splitlines()[:700]) + "\n1 0 3 4\n")
    assert rgbd_tum.main([str(bad), sp, root, ap, "--out", out, "--no-sleep"]) == 1
    err = capsys.readouterr().err
    assert "Wrong path to vocabulary" in err and "Failed to open" in err and "line 701" in err


def test_adapter_voc_program_matches_ctypes_path(tmp_path):
    from object_slam_amd import BowMatcher, ORBextractor, synth
    d = str(tmp_path)
    t = tree("B")
    v, _ = load(t, tmp_path, "voc.txt")
    frames, _ = synth.make_stream(2, 640, 480, seed=33)
    ex = ORBextractor(1000, 1.2, 8, 20, 7, 640, 480)
    kA, dA = ex(frames[0])
    kB, dB = ex(frames[1])
    for name, a in (("keysA", kA), ("keysB", kB), ("descA", dA), ("descB", dB)):
        np.ascontiguousarray(a).tofile(os.path.join(d, name + ".bin"))
    prog = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adapter_voc_program.cc"), "-o", prog,
                           "-L", LIBDIR, "-loslam_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    r = subprocess.run([prog, d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    get = lambda name, dt: np.fromfile(os.path.join(d, "out_" + name + ".bin"), dt)
    res = dict(line.split() for line in open(os.path.join(d, "out_results.txt")))
    vecs = {}
    for tag, desc in (("A", dA), ("B", dB)):
        word, node, weight = v.transform(desc, levelsup=4)
        bi, bv, fn, fs, fi = v.vectors(word, node, weight)
        vecs[tag] = (bi, bv, node)
        assert np.array_equal(get(tag + "_bow_ids", np.uint32), bi) and np.array_equal(get(tag + "_bow_vals", np.float64).view(np.uint64), bv.view(np.uint64))
        assert np.array_equal(get(tag + "_fv_nodes", np.uint32), fn) and np.array_equal(get(tag + "_fv_count", np.uint32), np.diff(fs)) and np.array_equal(get(tag + "_fv_items", np.uint32), fi)
    assert np.array_equal(get("A_qidx", np.int32), v.vectors(*v.transform(dA, levelsup=4))[4])
    assert float(res["scoreAB"]) == v.score(vecs["A"][:2], vecs["B"][:2]) and abs(float(res["scoreAA"]) - 1.0) < 1e-12
    bw = BowMatcher()
    nb, bm = bw.SearchByBoW(kA, dA, np.ones(len(kA), np.uint8), vecs["A"][2], kB, dB, vecs["B"][2], nnratio=0.7, checkOri=True)
    assert int(res["nbow"]) == nb > 50 and np.array_equal(get("bow_match", np.int32), bm)
    # a file that does not parse is refused (System.cc:69-74), with the line in oslam_last_error()
    bad = tmp_path / "bad.txt"
    bad.write_text("10 6 0 0\n0 0 1 2 3\n")
    r = subprocess.run([prog, d, str(bad)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("refused") and "line 2" in r.stdout
