"""CPU: the ORB vocabulary (include/oslam_hip.h "ORB vocabulary", object_slam_amd/vocabulary.py) — text loader, refusal of malformed files, host descent,
BowVector / FeatureVector assembly and the L1 score against the numpy restatement of tests/voc_common.py, and the tracking driver over the oracle's
operator table with a vocabulary set.  Ids are compared for equality; BowVector values and scores to 1e-12 relative (the same IEEE double operations on
both sides up to the order of the normalisation sum: at most a few thousand addends of O(1) magnitude)."""
import numpy as np
import pytest

import voc_common as V
from object_slam_amd import OslamError, slam
from object_slam_amd._lib import OSLAM_E_INVALID
from object_slam_amd.vocabulary import Vocabulary, save_text

CASES = {"A": V.tree_A, "B": V.tree_B, "C20x2": lambda: V.trees_C()[0], "C3x10": lambda: V.trees_C()[1], "D0": lambda: V.tree_D(0), "D1": lambda: V.tree_D(1),
         "D2": lambda: V.tree_D(2), "D3": lambda: V.tree_D(3)}
_cache = {}


def tree(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def load(t, tmp_path, name="voc.txt"):
    p = str(tmp_path / name)
    save_text(p, *t.arrays())
    return Vocabulary.load(p)


def test_case_shapes():
    """The generated trees are what the tests below assume of them."""
    a, b = tree("A"), tree("B")
    assert a.n == 1110
    assert 12000 < b.n < 40000, b.n
    leaf_depths = {b.depth[i] for i in range(1, b.n + 1) if b.is_leaf[i - 1]}
    assert leaf_depths == {2, 3, 4, 5, 6}, leaf_depths
    assert {len(c) for c in b.children.values()} >= set(range(1, 11))
    assert tree("C20x2").n == 420 and tree("C3x10").n == sum(3 ** d for d in range(1, 11))


@pytest.mark.parametrize("name", list(CASES))
def test_loader_round_trip(name, tmp_path):
    t = tree(name)
    p = str(tmp_path / "voc.txt")
    save_text(p, *t.arrays())
    v = Vocabulary.load(p)
    info = v.info
    assert (info["k"], info["L"], info["scoring"], info["weighting"]) == (t.k, t.L, t.scoring, t.weighting)
    assert info["nodes"] == t.n and info["words"] == len(t.word_of) and info["max_depth"] == max(t.depth.values())
    parent, leaf, desc, weight, word = v.nodes()
    assert np.array_equal(parent, t.parent) and np.array_equal(leaf, t.is_leaf) and np.array_equal(desc, t.desc)
    want_word = np.full(t.n, -1, np.int32)
    for nid, w in t.word_of.items():
        want_word[nid - 1] = w
    assert np.array_equal(word, want_word)
    # weights: bit-equal to Python's float() of the text that is in the file
    text_w = np.array([float(line.split()[-1]) for line in open(p).read().splitlines()[1:]], np.float64)
    assert np.array_equal(weight.view(np.uint64), text_w.view(np.uint64)) and np.array_equal(text_w.view(np.uint64), t.weight.view(np.uint64))
    # the same tree from arrays
    v2 = Vocabulary.from_arrays(*t.arrays())
    assert v2.info == info
    assert all(np.array_equal(x, y) for x, y in zip(v2.nodes(), (parent, leaf, desc, weight, word)))


def test_loader_reads_awkward_numbers_like_python(tmp_path):
    texts = ["0.1", "1e-310", "3.141592653589793238462643383279", "1.7976931348623157e308", "0.30000000000000004", "2.2250738585072014e-308"]
    p = tmp_path / "w.txt"
    for a, b in zip(texts[0::2], texts[1::2]):
        p.write_text("2 1 0 0\n" + "".join("0 1 " + " ".join(["7"] * 32) + " " + w + "\n" for w in (a, b)) + "\n\n")   # (blank lines at the end are not nodes)
        got = Vocabulary.load(str(p)).nodes()[3]
        assert got.view(np.uint64).tolist() == np.array([float(a), float(b)]).view(np.uint64).tolist()


def _small_lines(tmp_path):
    t = V.make_tree(7, 3, 2)
    p = tmp_path / "small.txt"
    save_text(str(p), *t.arrays())
    return t, p.read_text().splitlines()


def _edit(lines, lineno, fn):
    out = list(lines)
    out[lineno - 1] = fn(out[lineno - 1])
    return out


MALFORMED = {
    # name: (edit of the lines of a valid k = 3, L = 2 file (12 nodes, 13 lines), 1-based line the message must name)
    "short_line": (lambda L: _edit(L, 6, lambda s: " ".join(s.split()[:20])), 6),
    "missing_weight": (lambda L: _edit(L, 9, lambda s: " ".join(s.split()[:-1])), 9),
    "empty_line_inside": (lambda L: _edit(L, 4, lambda s: ""), 4),
    "parent_is_itself": (lambda L: _edit(L, 5, lambda s: " ".join(["4"] + s.split()[1:])), 5),
    "parent_is_later": (lambda L: _edit(L, 5, lambda s: " ".join(["9"] + s.split()[1:])), 5),
    "negative_parent": (lambda L: _edit(L, 5, lambda s: " ".join(["-1"] + s.split()[1:])), 5),
    "byte_256": (lambda L: _edit(L, 7, lambda s: " ".join(s.split()[:5] + ["256"] + s.split()[6:])), 7),
    "byte_negative": (lambda L: _edit(L, 7, lambda s: " ".join(s.split()[:5] + ["-3"] + s.split()[6:])), 7),
    "byte_not_a_number": (lambda L: _edit(L, 7, lambda s: " ".join(s.split()[:5] + ["x1"] + s.split()[6:])), 7),
    "too_many_fields": (lambda L: _edit(L, 8, lambda s: s + " 1.0"), 8),
    "inner_node_without_children": (lambda L: L[:10], 10),   # node 9 (line 10) is the last inner node: its children are cut off
    "no_node_lines": (lambda L: L[:1], 2),
    "header_k_21": (lambda L: _edit(L, 1, lambda s: "21 2 0 0"), 1),
    "header_L_0": (lambda L: _edit(L, 1, lambda s: "3 0 0 0"), 1),
    "header_L_11": (lambda L: _edit(L, 1, lambda s: "3 11 0 0"), 1),
    "header_scoring_6": (lambda L: _edit(L, 1, lambda s: "3 2 6 0"), 1),
    "header_weighting_4": (lambda L: _edit(L, 1, lambda s: "3 2 0 4"), 1),
    "header_short": (lambda L: _edit(L, 1, lambda s: "3 2 0"), 1),
}


@pytest.mark.parametrize("name", list(MALFORMED))
def test_malformed_files_are_refused_with_the_line(name, tmp_path):
    t, lines = _small_lines(tmp_path)
    assert len(lines) == 13 and not t.is_leaf[8] and t.parent[9] == 9     # (node 9, line 10, is inner and has its children after it)
    edit, lineno = MALFORMED[name]
    p = tmp_path / "bad.txt"
    p.write_text("\n".join(edit(lines)) + "\n")
    with pytest.raises(OslamError) as ei:
        Vocabulary.load(str(p))
    assert ei.value.code == OSLAM_E_INVALID
    assert ("line %d" % lineno) in str(ei.value), str(ei.value)
    # the untouched file loads
    p.write_text("\n".join(lines) + "\n")
    assert Vocabulary.load(str(p)).info["nodes"] == 12


def test_missing_file_is_refused(tmp_path):
    with pytest.raises(OslamError) as ei:
        Vocabulary.load(str(tmp_path / "nope.txt"))
    assert ei.value.code == OSLAM_E_INVALID


@pytest.mark.parametrize("name", ["A", "B", "C20x2", "C3x10", "D0"])
def test_transform_host_matches_the_restatement(name, tmp_path):
    t = tree(name)
    v = load(t, tmp_path)
    feats, n_ties = V.make_descriptors(t, 2000, seed=5)
    assert n_ties >= 2
    levelsups = sorted({0, 2, 4, t.L, t.L + 1})
    want, paths = V.ref_transform_many(t, feats, levelsups)
    # the cases the descent must get right are in the set: a centre itself, a tie between siblings (constructed: the first of the two must win; twins
    # deeper in the tree), and — B — a leaf above nid_level
    ch = t.children[0]
    for f, p in zip(feats[-n_ties:], paths[-n_ties:]):
        d = V.hamming(t.desc[np.array(ch) - 1], f)
        assert (d == d.min()).sum() == 2 and p[0] == ch[int(np.flatnonzero(d == d.min())[0])]
    assert sum(int(V.hamming(t.desc[np.array(p) - 1], f).min() == 0) for f, p in zip(feats, paths)) >= 3      # (a descriptor that IS a centre on its path)
    if name == "B":
        assert any(len(p) < t.L for p in paths) and any(len(p) == t.L for p in paths)
    for lu in levelsups:
        word, node, weight = v.transform_host(feats, levelsup=lu)
        assert np.array_equal(word, want[lu][0]), lu
        assert np.array_equal(node, want[lu][1]), lu
        assert np.array_equal(weight.view(np.uint64), want[lu][2].view(np.uint64)), lu
    if name == "B":   # levelsup 0 on leaves above depth L: the leaf's own node id
        short = np.array([len(p) < t.L for p in paths])
        assert np.array_equal(v.transform_host(feats, 0)[1][short], np.array([p[-1] for p in paths], np.uint32)[short])


@pytest.mark.parametrize("scoring", [0, 1])
@pytest.mark.parametrize("weighting", [0, 1, 2, 3])
def test_vectors_and_score_match_the_restatement(weighting, scoring, tmp_path):
    t = V.tree_D(weighting, scoring)
    v = load(t, tmp_path)
    rng = np.random.default_rng(9)
    sets = []
    for s in range(2):
        feats = t.desc[rng.integers(0, t.n, 1500)].copy()     # near centres, so that words repeat within a set and between the two
        feats[:, rng.integers(0, 32)] ^= np.uint8(1 << s)
        word, node, weight = v.transform_host(feats, levelsup=2)
        assert (weight == 0).sum() > 10 and (np.bincount(word).max() > 1)
        bi, bv, fn, fs, fi = v.vectors(word, node, weight)
        bow, fv = V.ref_vectors(t, word, node, weight)
        assert bi.tolist() == sorted(bow)
        want = np.array([bow[int(i)] for i in bi])
        assert np.all(np.abs(bv - want) <= 1e-12 * np.abs(want))
        assert fn.tolist() == sorted(fv) and len(fs) == len(fn) + 1 and fs[0] == 0
        for r, nd in enumerate(fn):
            assert fi[fs[r]:fs[r + 1]].tolist() == fv[int(nd)]
        # zero-weight features are in neither vector
        zero = set(np.flatnonzero(weight == 0).tolist())
        assert not zero & set(fi.tolist()) and len(fi) == len(word) - len(zero)
        assert not (set(word[weight == 0].tolist()) - set(word[weight > 0].tolist())) & set(bi.tolist())
        sets.append(((bi, bv), bow))
    if scoring == 0:
        s = v.score(sets[0][0], sets[1][0])
        want = V.ref_score_l1(sets[0][1], sets[1][1])
        assert 0 < want < 1 and abs(s - want) <= 1e-12 * abs(want)
        assert abs(v.score(sets[0][0], sets[0][0]) - 1.0) <= 1e-12
    else:
        with pytest.raises(OslamError) as ei:
            v.score(sets[0][0], sets[1][0])
        assert ei.value.code == OSLAM_E_INVALID and "L1_NORM" in str(ei.value)


@pytest.mark.parametrize("scoring", [2, 3, 4, 5])
def test_other_scorings_divide_by_entries_and_refuse_to_score(scoring, tmp_path):
    for weighting in (0, 3):
        t = V.tree_D(weighting, scoring)
        v = load(t, tmp_path)
        feats = t.desc[np.random.default_rng(3).integers(0, t.n, 400)]
        word, node, weight = v.transform_host(feats, levelsup=2)
        bi, bv, _, _, _ = v.vectors(word, node, weight)
        bow, _ = V.ref_vectors(t, word, node, weight)
        want = np.array([bow[int(i)] for i in bi])
        assert bi.tolist() == sorted(bow) and np.all(np.abs(bv - want) <= 1e-12 * np.abs(want))
        with pytest.raises(OslamError) as ei:
            v.score((bi, bv), (bi, bv))
        assert ei.value.code == OSLAM_E_INVALID and "scoring %d" % scoring in str(ei.value)


def test_driver_over_the_oracle_table_uses_the_vocabulary(oracle, tmp_path):
    """30 frames of the synthetic RGB-D stream through the driver over the oracle's operator table (no device, no voc_nodes_keyed: the host descent) with
    vocabulary B: the FeatureVector nodes of its keyframes are nodes of B at depth L - 4 = 2, not the 11 .. 110 of the substitute."""
    from slam_common import H, W, make_streams, oracle_ops, run
    t = tree("B")
    v = load(t, tmp_path)
    n = 30
    streams = make_streams(1, n)
    cfg = slam.make_config(W, H, 1)
    sysm = slam.System(cfg, oracle_ops(cfg), vocabulary=v)
    _, states = run(sysm, streams, n)
    assert (states == slam.OK).all()
    st = sysm.stats(0)
    assert st["keyframes_created"] >= 3 and st["local_bas"] >= 2 and st["map_violations"] == 0, st
    level2 = {i for i in range(1, t.n + 1) if t.depth[i] == 2}
    assert max(level2) > 110
    seen, done = set(), 0
    for kf in range(st["keyframes_created"]):
        nodes = sysm.debug_bow_nodes(0, kf)
        if len(nodes):
            done += 1
            assert set(nodes.tolist()) <= level2
            seen |= set(nodes.tolist())
    assert done >= 2 and len(seen) > 20
    with pytest.raises(OslamError) as ei:
        sysm.set_vocabulary(v)
    assert ei.value.code == OSLAM_E_INVALID and "before the first frame" in str(ei.value)
    # a handle without a vocabulary keeps the substitute's ids
    sub = slam.System(cfg, oracle_ops(cfg))
    run(sub, streams, n)
    ids = np.concatenate([sub.debug_bow_nodes(0, kf) for kf in range(sub.stats(0)["keyframes_created"])])
    assert len(ids) and ids.min() >= 11 and ids.max() <= 110


def test_set_vocabulary_none_is_the_substitute_bit_for_bit(oracle):
    from slam_common import H, W, make_streams, oracle_ops, run
    n = 20
    streams = make_streams(1, n)
    cfg = slam.make_config(W, H, 1)
    a = slam.System(cfg, oracle_ops(cfg))
    b = slam.System(cfg, oracle_ops(cfg), vocabulary=None)
    b.set_vocabulary(None)
    pa, sa = run(a, streams, n)
    pb, sb = run(b, streams, n)
    assert np.array_equal(pa, pb) and np.array_equal(sa, sb) and a.stats(0) == b.stats(0)


def test_adapter_voc_program_compiles_and_refuses_a_bad_file(tmp_path):
    """tests/adapter_voc_program.cc is written against ORB_SLAM2::ORBVocabulary of include/orb_slam2_adapter.hpp; loadFromTextFile is host code."""
    import os
    import subprocess
    from object_slam_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "object_slam_amd")
    build.build_hip()
    prog = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "adapter_voc_program.cc"), "-o", prog,
                           "-L", libdir, "-loslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    bad = tmp_path / "bad.txt"
    bad.write_text("10 6 0 0\n0 0 1 2 3\n")
    r = subprocess.run([prog, str(tmp_path), str(bad)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("refused") and "line 2" in r.stdout, (r.stdout, r.stderr)
