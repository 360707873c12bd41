"""CPU: pins the restatement of tests/keyframe_db_common.py (the yardstick of tests/test_keyframe_db_gpu.py) by facts that do not depend on it: the host
L1 score of the library, the (smallest common word, add serial) order claim of include/oslam_hip.h against the literal list replay, hand-built cases with
known answers, and the margin condition of the GPU fixtures.  Also: the module, the exports and the refusal without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import keyframe_db_common as kc
import voc_common as V
from object_slam_amd import OslamError, keyframe_db   # (at import: without the operator's module nothing here can pass)
from object_slam_amd.vocabulary import Vocabulary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _uniform(words):
    words = np.asarray(sorted(words), np.uint32)
    return words, np.full(len(words), 1.0 / len(words))


def test_header_section_is_exported():
    txt = open(os.path.join(ROOT, "include", "oslam_hip.h")).read()
    assert "KeyFrameDatabase" in txt
    names = sorted(set(re.findall(r"\b(oslam_kfdb_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))))
    assert len(names) >= 11, names
    from object_slam_amd import build
    L = C.CDLL(build.build_hip())
    for n in names:
        assert hasattr(L, n), "missing export %s" % n
    for n in ("oslam_kfdb_detect_loop_candidates", "oslam_kfdb_detect_relocalization_candidates"):
        assert n in names and n + "_device" in names


def test_record_mirrors_have_the_sizes_of_the_header(tmp_path):
    import subprocess
    pairs = [("oslam_kfdb_add_t", keyframe_db.ADD_DTYPE), ("oslam_kfdb_key_t", keyframe_db.KEY_DTYPE), ("oslam_kfdb_covis_t", keyframe_db.COVIS_DTYPE),
             ("oslam_kfdb_query_t", keyframe_db.QUERY_DTYPE)]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "oslam_hip.h"\nint main(void) {\n' + "".join('    printf("%%zu\\n", sizeof(%s));\n' % n for n, _ in pairs) +
                   '    printf("%d %d %d %d\\n", OSLAM_KFDB_COVIS, OSLAM_KFDB_CHUNK, OSLAM_KFDB_MAX_KEYFRAMES, OSLAM_KFDB_MAX_WORDS);\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    assert [int(x) for x in lines[:4]] == [dt.itemsize for _, dt in pairs]
    assert [int(x) for x in lines[4].split()] == [keyframe_db.COVIS, keyframe_db.CHUNK, keyframe_db.MAX_KEYFRAMES, keyframe_db.MAX_WORDS]


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    voc = Vocabulary.from_arrays(*V.make_tree(5, 4, 2).arrays())
    with pytest.raises(OslamError) as ei:
        keyframe_db.KeyFrameDatabase(voc, 2, 8, 64)
    assert "no CPU fallback" in str(ei.value)


def test_score_is_the_librarys_host_score():
    voc = Vocabulary.from_arrays(*V.make_tree(5, 4, 2).arrays())   # L1_NORM
    rng = np.random.default_rng(3)
    kfs, _, scenes = kc.make_database(rng, 30)
    for t in range(40):
        q = kc.scene_vector(rng, scenes[t % 3], 300)
        _, ki, kv = kfs[int(rng.integers(30))]
        assert kc.score_l1(q[0], q[1], ki, kv) == voc.score(q, (ki, kv))   # the same loop: the same bits
    ids, vals = kfs[0][1:]
    assert abs(kc.score_l1(ids, vals, ids, vals) - 1.0) < 1e-12


def _order_claim(db, ids, connected=()):
    """lKFsSharingWords by the claim: the present keyframes that share a word, ascending (smallest common word, add serial) — plain set arithmetic"""
    q = set(int(w) for w in ids)
    rows = []
    for kf in db.kfs.values():
        common = q & set(kf.ids.tolist())
        if common and kf.mnId not in connected:
            rows.append((min(common), kf.serial, kf.mnId, len(common)))
    rows.sort()
    return [r[2] for r in rows], {r[2]: r[3] for r in rows}


def test_order_is_smallest_common_word_then_add_serial():
    """Every query of both fixtures, which include erase, re-add under the same id, and clear."""
    n_checked = 0
    for script in (kc.fixture()[0], kc.state_fixture()[0]):
        dbs = {}
        for op in script:
            if op[0] in ("reloc", "loop"):
                for rec in op[1]:
                    db = dbs.setdefault(rec[0], kc.RefDatabase())
                    claim, words = _order_claim(db, rec[1], set(rec[4]) if op[0] == "loop" else ())
                    res, _ = kc.run_reference([(op[0], [rec])], dbs)
                    assert res[0][0]["sharing"] == claim
                    if claim:
                        assert res[0][0]["diag"][1] == max(words.values())
                    n_checked += len(claim) > 1
            else:
                kc.run_reference([op], dbs)
    assert n_checked > 30


def _db(vectors, covis=None):
    db = kc.RefDatabase()
    for k, (ids, vals) in enumerate(vectors):
        db.add(k, ids, vals)
    for k, l in (covis or {}).items():
        db.set_covisibility(k, l)
    return db


@pytest.mark.parametrize("max_common,min_common", [(5, 4), (10, 8)])
def test_truncation_of_min_common_words(max_common, min_common):
    """(int)(5 * 0.8f) = 4 and (int)(10 * 0.8f) = 8: 0.8f is a little above 0.8, the products round to 4 and 8 exactly.  A keyframe with exactly
    minCommonWords common words is not scored, one more is."""
    q = _uniform(range(20))
    vecs = [_uniform(list(range(max_common)) + [100]), _uniform(list(range(min_common)) + [101, 102]), _uniform(list(range(min_common + 1)) + [103])]
    r = _db(vecs).detect_relocalization_candidates(*q)
    assert r["diag"][:4] == [3, max_common, min_common, 2]
    assert sorted(r["scores"]) == [0, 2]
    r = _db(vecs).detect_loop_candidates(*q, 0.0, [])
    assert r["diag"][:4] == [3, max_common, min_common, 2] and sorted(r["scores"]) == [0, 2]


def test_connected_keyframe_that_would_have_been_best():
    q = _uniform(range(10))
    vecs = [q, _uniform(list(range(9)) + [50]), _uniform(list(range(8)) + [51, 52])]   # keyframe 0 is the query's twin: score 1
    covis = {1: [0], 2: [0]}
    r = _db(vecs, covis).detect_loop_candidates(*q, 0.1, [])
    assert r["cand"] == [0] and r["diag"][1] == 10          # 1 and 2 both name 0 as their best; dedup
    r = _db(vecs, covis).detect_loop_candidates(*q, 0.1, [0, 7])
    assert r["sharing"] == [1, 2] and r["diag"][1] == 9     # 0 never enters the list, nor the maximum, and is never "reached" as a neighbour
    assert r["cand"] == [1, 2] and r["acc"] == [r["scores"][1], r["scores"][2]]
    assert r["conn_score"][0] == F32(1.0) and r["conn_score"][1] == F32(-1)


def test_dedup_keeps_the_first_occurrence():
    q = _uniform(range(10))
    vecs = [_uniform(list(range(1, 10)) + [60]), q, _uniform(list(range(2, 10)) + [61, 62]), _uniform(list(range(9)) + [63])]
    # list order by smallest common word then serial: 1 (word 0), 3 (word 0), 0 (word 1), 2 (word 2); all of 0, 2, 3 name 1 as best
    r = _db(vecs, {0: [1], 2: [1], 3: [1]}).detect_relocalization_candidates(*q)
    assert r["sharing"] == [1, 3, 0, 2]
    # entry 1 itself (acc = 1, no neighbours) falls below 0.75f * bestAccScore; of the retained entries 3, 0 and 2, all with pBestKF = 1, the first one is output
    assert r["cand"] == [1] and r["acc"] == [F32(r["scores"][3] + r["scores"][1])]
    assert r["scores"][1] == F32(1.0)


def test_best_changes_on_strictly_greater_only():
    q = _uniform(range(10))
    twin = _uniform(list(range(9)) + [70])
    r = _db([twin, twin], {0: [1], 1: [0]}).detect_relocalization_candidates(*q)
    assert r["scores"][0] == r["scores"][1]
    assert r["cand"] == [0, 1]        # a neighbour with an equal score does not take over: each entry keeps itself
    assert r["acc"][0] == r["acc"][1] == F32(r["scores"][0] + r["scores"][1])


def test_stale_reloc_score_across_two_queries():
    a, b = _uniform(range(10)), _uniform(list(range(3)) + [80, 81, 82, 83])
    db = _db([a, b], {0: [1]})
    q1 = _uniform(list(range(3)) + [80, 81, 82, 83, 90])
    r1 = db.detect_relocalization_candidates(*q1)        # scores keyframe 1 (7 common words) and not keyframe 0 (3)
    assert sorted(r1["scores"]) == [1]
    s1 = r1["scores"][1]
    q2 = _uniform(range(12))
    r2 = db.detect_relocalization_candidates(*q2)        # scores keyframe 0 (10), reaches keyframe 1 (3 words) without scoring it
    assert sorted(r2["scores"]) == [0] and r2["sharing"] == [0, 1]
    assert r2["acc"] == [F32(r2["scores"][0] + s1)]       # ... and keyframe 1 contributes what query 1 left in it
    assert r2["cand"] == [1] if s1 > r2["scores"][0] else r2["cand"] == [0]
    db2 = _db([a, b], {0: [1]})
    assert db2.detect_relocalization_candidates(*q2)["acc"] == [r2["scores"][0]]   # without query 1: reloc_score is 0 at add


def test_margin_condition_of_the_gpu_fixtures():
    """A condition on the INPUTS of tests/test_keyframe_db_gpu.py: no comparison of scores whose sides are not equal by construction lies within 1e-5 relative
    (the 11-ulp float bound of an accumulated score is about 1.3e-6), so the restatement and the kernel decide every one of them alike."""
    n = 0
    for script, expected in (kc.fixture(), kc.state_fixture(), kc.identity_fixture(), kc.refusal_fixture()):
        for (op, _), res in zip(script, expected):
            for r in res or []:
                assert kc.margin_violations(r["log"]) == [], (op, r["diag"])
                n += len(r["log"])
    assert n > 500
    ties = sum(1 for _, res in zip(*kc.fixture()) for r in res or [] for k, a, b in r["log"] if k == "best" and a == b)
    assert ties > 0   # identical vectors are in the fixture and come out as ties


def test_fixture_covers_what_it_names():
    script, expected = kc.fixture()
    adds = script[0][1]
    assert sorted(set(len(a[2]) for a in adds if a[0] == 8) & set(kc.VEC_SIZES)) == sorted(kc.VEC_SIZES)
    counts = {}
    for a in adds:
        counts[a[0]] = counts.get(a[0], 0) + 1
    assert [counts.get(d, 0) for d in (0, 1, 3, 4, 6, 7)] == list(kc.KF_COUNTS) and not {2, 5, 11} & set(counts)
    for res in (expected[2], expected[3], expected[4]):
        by_db = {q[0]: r for q, r in zip(script[2][1], res)}
        assert by_db[9]["diag"][0] == 0 and by_db[10]["diag"][0] == 0 and by_db[0]["cand"] == []
        assert by_db[7]["diag"][3] < by_db[7]["diag"][0]          # the 0.8 filter drops some
        assert len(by_db[7]["cand"]) >= 1 and by_db[8]["diag"][0] >= 5
    assert any(r["diag"][4] < r["diag"][3] for r in expected[3])   # minScore drops some
