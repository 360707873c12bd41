"""GPU: the KeyFrameDatabase operator (include/oslam_hip.h, "KeyFrameDatabase") against the literal restatement of tests/keyframe_db_common.py.  Candidate ids and
their order, counts and the diagnostics row: equal element for element, no case left out.  Scores (the connected ids' are the ones the operator outputs):
the sum of a score has at most n_common terms whose absolute values add up to at most 2 for L1-normalised vectors, so any two summation orders differ by
at most n_common * 2^-52 in fp64 — far below half a float ulp, hence at most 1 float ulp after the cast.  Accumulated scores: at most 11 float ulp (one per
score and one per each of the at most 10 additions).  tests/test_keyframe_db_cpu.py asserts the margin condition that makes the discrete results comparable."""
import os
import subprocess

import numpy as np
import pytest

import keyframe_db_common as kc
import voc_common as V
from object_slam_amd import OslamError, keyframe_db   # (at import: every test of this file needs the operator's module)
from object_slam_amd._lib import OSLAM_E_CAPACITY, OSLAM_E_INVALID
from object_slam_amd.vocabulary import Vocabulary, save_text

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "object_slam_amd")
TREE = V.make_tree(5, 4, 2)   # L1_NORM; the operator reads nothing of a vocabulary but its scoring type


@pytest.fixture(scope="module")
def voc():
    return Vocabulary.from_arrays(*TREE.arrays())


def ulps(a, b):
    """distance of two float32 arrays in units in the last place (both finite, same sign or zero)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def apply(db, op, recs, device=False, voc=None):
    """One operation of a script (keyframe_db_common) on the device; a query returns one dict per query in the restatement's form."""
    if op == "add":
        db.add(*keyframe_db.pack_add([r[0] for r in recs], [r[1] for r in recs], [(r[2], r[3]) for r in recs]))
    elif op == "erase":
        db.erase(keyframe_db.pack_keys([r[0] for r in recs], [r[1] for r in recs]))
    elif op == "clear":
        db.clear(recs)
    elif op == "covis":
        db.set_covisibility(keyframe_db.pack_covisibility([r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs]))
    elif op in ("reloc", "loop"):
        loop = op == "loop"
        rec, ids, vals, conn = keyframe_db.pack_queries([r[0] for r in recs], [(r[1], r[2]) for r in recs], min_scores=[r[3] for r in recs] if loop else None,
                                                        connected=[r[4] for r in recs] if loop else None)
        out = db.detect_loop_candidates(rec, ids, vals, conn, device=device, voc=voc) if loop else db.detect_relocalization_candidates(rec, ids, vals, device=device, voc=voc)
        res = []
        for q in range(len(recs)):
            n = int(out["n_cand"][q])
            assert 0 <= n <= db.max_keyframes, (q, n)
            assert (out["cand"][q, n:] == -1).all() and np.isnan(out["cand_acc"][q, n:]).all()   # nothing is written beyond the count
            r = dict(cand=out["cand"][q, :n].tolist(), acc=out["cand_acc"][q, :n].copy(), diag=out["diag"][q].tolist())
            if loop:
                r["conn_score"] = out["conn_score"][rec["conn_off"][q]:rec["conn_off"][q] + rec["n_conn"][q]].copy()
            res.append(r)
        return res
    else:
        raise ValueError(op)


def run(db, script, device=False):
    return [apply(db, op, recs, device) for op, recs in script]


def check_parity(script, expected, got):
    n_cand = n_conn = 0
    for (op, recs), exp, res in zip(script, expected, got):
        if exp is None:
            continue
        assert len(exp) == len(res)
        for q, (e, g) in enumerate(zip(exp, res)):
            where = (op, "query", q, "database", recs[q][0])
            assert g["cand"] == e["cand"], where
            assert g["diag"] == e["diag"], where
            print(where, "diag", g["diag"], "cand", g["cand"], "acc ulps", ulps(g["acc"], e["acc"]).tolist())
            assert (ulps(g["acc"], e["acc"]) <= 11).all(), where
            n_cand += len(e["cand"])
            if op == "loop":
                print("   conn_score ulps", ulps(g["conn_score"], e["conn_score"]).tolist())
                assert (ulps(g["conn_score"], e["conn_score"]) <= 1).all(), where
                assert [float(x) == -1.0 for x in g["conn_score"]] == [float(x) == -1.0 for x in e["conn_score"]], where
                n_conn += sum(float(x) != -1.0 for x in e["conn_score"])
    return n_cand, n_conn


def same(a, b):
    """two runs' outputs, bit for bit"""
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert (ra is None) == (rb is None)
        for x, y in zip(ra or [], rb or []):
            assert x["cand"] == y["cand"] and x["diag"] == y["diag"]
            assert np.array_equal(x["acc"].view(np.uint32), y["acc"].view(np.uint32))
            if "conn_score" in x:
                assert np.array_equal(x["conn_score"].view(np.uint32), y["conn_score"].view(np.uint32))
    return True


def test_parity_with_the_restatement(voc):
    """Databases of 0, 1, 15, 16, 17 and 65 keyframes, vectors of 0, 1, 15, 16, 17, 255, 256, 257 and 2400 words, an empty query, a query that shares no word,
    unused databases in between; reloc, loop, and reloc again over the scores the first batch left."""
    script, expected = kc.fixture()
    db = keyframe_db.KeyFrameDatabase(voc, kc.N_DATABASES, kc.MAX_KEYFRAMES, kc.MAX_WORDS)
    got = run(db, script)
    n_cand, n_conn = check_parity(script, expected, got)
    assert n_cand >= 12 and n_conn >= 8
    # the device entry point, on a second handle that goes through the same history: the same bits
    db2 = keyframe_db.KeyFrameDatabase(voc, kc.N_DATABASES, kc.MAX_KEYFRAMES, kc.MAX_WORDS)
    assert same(got, run(db2, script, device=True))
    db.close(); db2.close()


def test_state_sequences(voc):
    """add / erase / clear / set_covisibility interleaved with queries; reloc_score persists from call to call; ids come back with new vectors and serials."""
    script, expected = kc.state_fixture()
    stale = 0
    for (op, _), res in zip(script, expected):   # the fixture does meet the quirk: a neighbour that is reached, not scored, and holds a score from before
        for r in res or []:
            stale += op == "reloc" and r["diag"][3] < r["diag"][0]
    assert stale >= 4
    db = keyframe_db.KeyFrameDatabase(voc, 4, 32, 128)
    n_cand, _ = check_parity(script, expected, run(db, script))
    assert n_cand >= 20
    db.close()


def test_pool_is_recycled(voc):
    """12 chunks of 128 words; cycles of add and erase whose words exceed the pool many times over; then the capacity error where it is due."""
    rng = np.random.default_rng(4)
    db = keyframe_db.KeyFrameDatabase(voc, 2, 8, 300, pool_words=12 * 128)
    assert db.info == dict(free_chunks=12, chunks=12, present=0)
    ref = kc.RefDatabase()
    total = 0
    for it in range(30):
        vecs = [kc.l1_vector(rng, np.arange(400), int(n)) for n in (129, 256, 300, 1)]   # 2 + 2 + 3 + 1 chunks
        apply(db, "add", [(1, k, *v) for k, v in enumerate(vecs)])
        total += sum(len(v[0]) for v in vecs)
        assert db.info["free_chunks"] == 4 and db.info["present"] == 4
        if it % 10 == 0:
            for k, v in enumerate(vecs):
                ref.add(k, *v)
            q = kc.l1_vector(rng, np.arange(400), 200)
            g = apply(db, "reloc", [(1, *q)])[0]
            e = ref.detect_relocalization_candidates(*q)
            assert kc.margin_violations(ref.log) == []
            assert g["cand"] == e["cand"] and g["diag"] == e["diag"] and len(e["cand"]) >= 1
            ref.clear()
        if it % 2:
            apply(db, "erase", [(1, k) for k in range(4)])
        else:
            apply(db, "clear", [1])
        assert db.info == dict(free_chunks=12, chunks=12, present=0)
    assert total > 10 * 12 * 128
    apply(db, "add", [(0, k, *kc.l1_vector(rng, np.arange(400), 300)) for k in range(4)])   # 12 chunks: full
    with pytest.raises(OslamError) as ei:
        apply(db, "add", [(0, 5, *kc.l1_vector(rng, np.arange(400), 1))])
    assert ei.value.code == OSLAM_E_CAPACITY
    apply(db, "add", [(0, 5, *kc.l1_vector(rng, np.arange(400), 0))])   # no word, no chunk
    assert db.info == dict(free_chunks=0, chunks=12, present=5)
    db.close()


def test_refusals_change_nothing(voc):
    script, expected = kc.refusal_fixture()
    db = keyframe_db.KeyFrameDatabase(voc, 3, 16, 128, pool_words=16 * 128 + 256)
    rng = np.random.default_rng(1)
    vec = kc.l1_vector(rng, np.arange(300), 40)
    big = kc.l1_vector(rng, np.arange(300), 129)
    unsorted = (vec[0][::-1].copy(), vec[1])
    twice = (np.concatenate([vec[0][:1], vec[0][:1], vec[0][2:]]), vec[1])
    l2 = Vocabulary.from_arrays(*V.make_tree(5, 4, 2, scoring=1).arrays())
    qr, ql = script[2][1][0], script[3][1][0]
    refusals = [
        ("double add", OSLAM_E_INVALID, lambda: apply(db, "add", [(0, 0, *vec), (1, 3, *vec)])),                   # (the first record alone would be fine)
        ("slot overflow", OSLAM_E_CAPACITY, lambda: apply(db, "add", [(0, 1, *vec), (0, 16, *vec)])),
        ("pool overflow", OSLAM_E_CAPACITY, lambda: apply(db, "add", [(0, k, *vec) for k in range(4)])),           # 2 chunks are free
        ("too many words", OSLAM_E_CAPACITY, lambda: apply(db, "add", [(0, 2, *big)])),
        ("unsorted ids at add", OSLAM_E_INVALID, lambda: apply(db, "add", [(0, 2, *unsorted)])),
        ("a word twice at add", OSLAM_E_INVALID, lambda: apply(db, "add", [(0, 2, *twice)])),
        ("two queries on one database", OSLAM_E_INVALID, lambda: apply(db, "reloc", [qr, (0, *vec), qr])),
        ("a vocabulary that is not L1", OSLAM_E_INVALID, lambda: apply(db, "reloc", [qr], voc=l2)),
        ("unsorted query ids", OSLAM_E_INVALID, lambda: apply(db, "reloc", [(1, *unsorted)])),
        ("two loop queries on one database", OSLAM_E_INVALID, lambda: apply(db, "loop", [ql, ql])),
        ("a loop query over a vocabulary that is not L1", OSLAM_E_INVALID, lambda: apply(db, "loop", [ql], voc=l2)),
        ("covisibility of a keyframe that is not there", OSLAM_E_INVALID, lambda: apply(db, "covis", [(1, 2, [1]), (0, 9, [1])])),
    ]
    assert len(refusals) == kc.N_REFUSALS
    got = run(db, script[:4])
    info = db.info
    at = 4
    for i, (what, code, call) in enumerate(refusals):
        with pytest.raises(OslamError) as ei:
            call()
        assert ei.value.code == code, what
        assert db.info == info, what
        if at + 2 <= len(script):   # the queries that follow see the state the restatement has, stale reloc scores included
            got += run(db, script[at:at + 2])
            at += 2
    assert at == len(script)
    n_cand, n_conn = check_parity(script, expected, got)
    assert n_cand >= 2 * (kc.N_REFUSALS + 1) and n_conn >= kc.N_REFUSALS
    # the device entry point answers per query: -2 and nothing else of that query, the others as before
    rec, ids, vals, conn = keyframe_db.pack_queries([1, 0, 1], [qr[1:3], vec, qr[1:3]])
    out = db.detect_relocalization_candidates(rec, ids, vals, device=True)
    assert out["n_cand"].tolist() == [-2, 0, -2] and (out["diag"][[0, 2]] == -9).all() and (out["cand"] == -1).all() and out["diag"][1].tolist() == [0] * 5
    rec, ids, vals, conn = keyframe_db.pack_queries([1, 0], [unsorted, vec])
    assert db.detect_relocalization_candidates(rec, ids, vals, device=True)["n_cand"].tolist() == [-2, 0]
    rec["word_off"][0] = 10 ** 6
    assert db.detect_relocalization_candidates(rec, ids, vals, device=True)["n_cand"].tolist() == [-2, 0]
    rec, ids, vals, conn = keyframe_db.pack_queries([1], [qr[1:3]])
    assert same([apply(db, "reloc", [qr])], [[dict(cand=got[-2][0]["cand"], acc=got[-2][0]["acc"], diag=got[-2][0]["diag"])]])
    db.close()


def test_bit_identity_across_calls_and_batch_compositions(voc):
    script, expected = kc.identity_fixture()
    db = keyframe_db.KeyFrameDatabase(voc, 64, 16, 128)
    got = run(db, script)
    check_parity(script, expected, got)
    again = run(db, script[2:])                     # the same two batches of 64 once more (a reloc query rewrites the scores it wrote)
    assert same(got[2:], again)
    for q in (37, 0, 63):
        alone = [apply(db, "loop", [script[2][1][q]]), apply(db, "reloc", [script[3][1][q]])]
        assert same([[got[2][q]], [got[3][q]]], alone)
    dev = [apply(db, "loop", script[2][1], device=True), apply(db, "reloc", script[3][1], device=True)]
    assert same(got[2:], dev)
    # identical vectors, different slots, serials and databases: identical scores
    scores = expected[2][0]["scores"]
    best = max(scores, key=scores.get)                 # the keyframe of database 0 that scores highest against its loop query
    twin = [a[2:4] for a in script[0][1] if a[:2] == (0, best)][0]
    db.add(*keyframe_db.pack_add([5, 9, 9], [12, 13, 15], [twin] * 3))
    rec, ids, vals, conn = keyframe_db.pack_queries([5, 9, 0], [script[2][1][0][1:3]] * 3, min_scores=[0.0] * 3, connected=[[12], [15, 13], [best]])
    cs = db.detect_loop_candidates(rec, ids, vals, conn)["conn_score"]
    assert cs[0] > 0.05 and len(set(cs.view(np.uint32).tolist())) == 1
    db.close()


def _ops_text(script):
    lines, covis = [], {}
    for op, recs in script:
        if op == "covis":
            covis.update({(d, k): l for d, k, l in recs})
    for op, recs in script:
        for r in recs if op in ("add", "reloc", "loop") else []:
            bow = "%d %s" % (len(r[1 if op != "add" else 2]), " ".join("%d %r" % (int(w), float(x)) for w, x in zip(*(r[2:4] if op == "add" else r[1:3]))))
            if op == "add":
                l = covis.get((r[0], r[1]), [])
                lines.append("A %d %s %d %s" % (r[1], bow, len(l), " ".join(map(str, l))))
            elif op == "reloc":
                lines.append("R 0 %s" % bow)
            elif op == "loop":
                lines.append("L 0 %s %.9g %d %s" % (bow, np.float32(r[3]), len(r[4]), " ".join(map(str, r[4]))))
    return lines


def test_adapter_program_equals_the_python_view(tmp_path, voc):
    """tests/adapter_keyframe_db_program.cc, written against include/orb_slam2_adapter.hpp alone: one database, the operations of the refusal fixture plus an
    erase and a clear; its lines against the Python view's outputs."""
    from object_slam_amd import build
    build.build_hip()
    script = kc.refusal_fixture()[0][:6]
    lines = _ops_text(script) + ["E 3", "E 7"] + _ops_text(script[2:4]) + ["C"] + _ops_text(script[2:4])
    (tmp_path / "ops.txt").write_text("\n".join(lines) + "\n")
    save_text(str(tmp_path / "voc.txt"), *TREE.arrays())
    prog = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adapter_keyframe_db_program.cc"), "-o", prog,
                           "-L", LIBDIR, "-loslam_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    r = subprocess.run([prog, str(tmp_path), "16", "128"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    db = keyframe_db.KeyFrameDatabase(voc, 2, 16, 128)
    full = script + [("erase", [(1, 3), (1, 7)])] + script[2:4] + [("clear", [1])] + script[2:4]
    got = [q[0] for (op, _), q in zip(full, run(db, full)) if op in ("reloc", "loop")]
    out = [l for l in r.stdout.split("\n") if l]
    assert len(out) == len(got) == 8
    for line, g, op in zip(out, got, ["R", "L"] * 4):
        want = "%s %d" % (op, len(g["cand"])) + "".join(" %d %.9g" % (c, a) for c, a in zip(g["cand"], g["acc"])) + " | " + " ".join(map(str, g["diag"]))
        if op == "L":
            want += " |" + "".join(" %.9g" % s for s in g["conn_score"])
        assert line == want
    assert len(got[0]["cand"]) >= 1 and got[6]["cand"] == [] and got[4]["diag"] != got[0]["diag"]
    db.close()
