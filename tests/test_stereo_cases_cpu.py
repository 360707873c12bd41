"""Frame::ComputeStereoMatches without a GPU: the numpy restatement of tests/stereo_common.py against the C++ oracle on every case, the decisions
the case set takes (asserted, not hoped for), answers worked out by hand, and ground truth on noise-free shifts."""
import numpy as np
import pytest

import stereo_common as sc
from stereo_common import (ACCEPTED, ACCEPTED_CLAMP, CODES, CUT, DISPARITY, GUARD, MAXU_NEG, NO_CAND_DIST, NO_CAND_OCTAVE, NO_CAND_RANGE, RIGHT_WINDOW, ROW_OUTSIDE,
                           SHIFT_EDGE, f32)

KEPT = (ACCEPTED, ACCEPTED_CLAMP)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_case_names(oracle):
    assert tuple(c["name"] for c in sc.build_cases(oracle)) == sc.CASE_NAMES


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_restatement_equals_oracle(oracle, name):
    case = sc.case_by_name(oracle, name)
    ref = sc.run_restatement(oracle, case)
    oL, oR, _, _ = sc.pyramids(oracle, case)
    uR, dep, n = oracle.stereo_matches(oL, oR, case["kL"], case["dL"], case["kR"], case["dR"], case["bf"], case["b"], with_count=True)
    print(name, "N", len(case["kL"]), "Nr", len(case["kR"]), "before the cut", ref["n_before"], "kept", int(np.isin(ref["code"], KEPT).sum()))
    assert n == ref["n_before"]
    assert np.array_equal(bits(uR), bits(ref["uRight"]))
    assert np.array_equal(bits(dep), bits(ref["depth"]))
    assert np.array_equal(ref["uRight"] >= 0, np.isin(ref["code"], KEPT)) and (ref["code"] >= 0).all()


@pytest.fixture(scope="module")
def refs(oracle):
    return {c["name"]: (c, sc.run_restatement(oracle, c)) for c in sc.build_cases(oracle)}


def test_every_decision_is_taken(refs):
    count = np.zeros(len(CODES), np.int64)
    for name, (case, ref) in refs.items():
        count += np.bincount(ref["code"], minlength=len(CODES))
        d = ref["delta"][np.isin(ref["code"], (DISPARITY, ACCEPTED, ACCEPTED_CLAMP, CUT))]
        assert np.isfinite(d).all() and (np.abs(d) <= 0.5).all(), name          # the argument of stereo_common's docstring
    print({CODES[i]: int(count[i]) for i in range(len(CODES))})
    for code in range(len(CODES)):
        if code in sc.UNREACHABLE:
            assert count[code] == 0, CODES[code]
        else:
            assert count[code] >= 3, (CODES[code], count[code])


def test_edges_of_the_gates(refs):
    # uR == minU and the disparity test on both sides of maxD == 21
    case, ref = refs["maxd21"]
    m = ref["best_r"] >= 0
    at_min = case["kR"]["x"][ref["best_r"][m]] == case["kL"]["x"][m] - f32(21)
    assert at_min.sum() >= 3
    assert (ref["code"] == DISPARITY).sum() >= 3 and np.isin(ref["code"], KEPT).sum() >= 3
    case, ref = refs["maxd15"]
    assert (ref["code"] == NO_CAND_RANGE).sum() >= 3
    # uR == maxU: the clamped matches
    for name in ("clamp_single", "clamp_mixed", "median_zero_minority"):
        case, ref = refs[name]
        m = ref["code"] == ACCEPTED_CLAMP
        assert m.any() and (case["kR"]["x"][ref["best_r"][m]] == case["kL"]["x"][m]).all(), name
    assert (refs["clamp_mixed"][1]["code"] == ACCEPTED_CLAMP).sum() >= 5 and (refs["clamp_mixed"][1]["sad"][:5] == 0).all()
    # octave gate at exactly +-1 (searched) and +-2 (gated)
    for name, sign in (("octave_hi", 1), ("octave_lo", -1)):
        case, ref = refs[name]
        m = ref["best_r"] >= 0
        diff = case["kR"]["octave"][ref["best_r"][m]] - case["kL"]["octave"][m]
        assert (diff == sign).sum() >= 3 and (diff == 0).sum() >= 3 and (np.abs(diff) <= 1).all(), name
        gated = ref["code"] == NO_CAND_OCTAVE
        assert gated.sum() >= 3 and (case["kL"]["octave"][gated] == 2).all(), name
    # Hamming distance 74 searches, 75 does not
    case, ref = refs["hamming"]
    assert (ref["best_r"][case["d74"]] >= 0).all() and (ref["code"][case["d75"]] == NO_CAND_DIST).all() and len(case["d74"]) >= 3 and len(case["d75"]) >= 3
    # ties: two candidates at the winning distance, the lower index wins, and it is neither the leftmost nor the topmost of the two
    assert len(case["ties"]) >= 3
    for i, win, lose in case["ties"]:
        assert ref["n_at_best"][i] == 2 and ref["best_r"][i] == win and win < lose
        assert case["kR"]["x"][win] > case["kR"]["x"][lose] and case["kR"]["y"][win] > case["kR"]["y"][lose]
    # best shift at -L and at +L
    assert (refs["periodic5"][1]["bestinc"] == -5).all() and (refs["flat"][1]["bestinc"] == -5).all() and (refs["shifted5"][1]["bestinc"] == 5).all()
    assert (refs["flat"][1]["sad"] == 0).all() and (refs["flat"][1]["code"] == SHIFT_EDGE).all()
    # the borders: every early exit and the guard on every level used
    for name in ("borders", "borders_odd"):
        case, ref = refs[name]
        for code in (ROW_OUTSIDE, MAXU_NEG, RIGHT_WINDOW, GUARD):
            assert (ref["code"] == code).sum() >= 3, (name, CODES[code])
        for level in (0, 1, 3):
            assert ((ref["code"] == GUARD) & (ref["level"] == level)).sum() >= 3, (name, level)
        row0 = (case["kL"]["y"] > -1) & (case["kL"]["y"] < 0)
        assert row0.sum() >= 3 and (ref["code"][row0] != ROW_OUTSIDE).all()
        last = case["kL"]["y"] == case["left"].shape[0] - 1
        assert last.sum() >= 3 and (ref["code"][last] == GUARD).all()
    # the median of k_stereo_cut's third slice: matches and cuts among the keypoints from 2048 on
    case, ref = refs["size_2400_2400"]
    assert (ref["code"][2048:] == CUT).sum() >= 3 and np.isin(ref["code"][2048:], KEPT).sum() >= 3
    for name in ("size_1025_1025", "size_2049_2049"):
        assert refs[name][0]["max_kps"] == len(refs[name][0]["kL"]) and len(refs[name][0]["kL"]) % 2 == 1


def test_alignment_combinations(refs):
    for name in ("alignment", "alignment_odd"):
        case, ref = refs[name]
        kept = np.isin(ref["code"], KEPT)
        for level in (0, 1):
            seen = {(int(a), int(b)) for a, b in zip(ref["cxl"][kept & (ref["level"] == level)] % 4, ref["cxr"][kept & (ref["level"] == level)] % 4)}
            assert len(seen) == 16, (name, level, sorted(seen))


def test_corner_words(refs):
    """Matches that are kept and for which an aligned word of k_stereo_sad reaches outside its level (words_inside false): the kernel's byte-wise path.
    Level 0 as the device entry point sees it in the GPU tests — tightly packed, 4-byte aligned for the 320-wide images, and starting at 2 modulo 4 for
    every second 322 x 241 image of a batch — and level 1 in the extractor's pyramid.  No other case has such a match, which is why these exist."""
    n = {0: 0, 1: 0}
    for name, base in (("corners", 0), ("corners_odd", 2), ("corners_odd", 0)):
        case, ref = refs[name]
        reaches, inside = sc.words_inside(case, ref, base)
        out = reaches & ~inside & np.isin(ref["code"], KEPT)
        print(name, base, [(int(ref["level"][i]), int(ref["cy"][i]), int(ref["cxl"][i]), int(ref["cxr"][i])) for i in np.nonzero(out)[0]])
        for level in (0, 1):
            bottom = out & (ref["level"] == level) & (ref["cy"] + 5 == case["level_sizes"][level][1] - 1)
            assert bottom.sum() >= 2, (name, base, level)
            n[level] += int(bottom.sum())
        top = out & (ref["level"] == 0) & (ref["cy"] == 5)
        assert top.sum() >= (3 if base else 0) and (ref["sad"][out] > 0).all(), (name, base)
    assert n[0] >= 3 and n[1] >= 3
    for name, (case, ref) in refs.items():                      # the host entry point stages level 0 at a pitch of 64: the bottom-right corner again
        if name.startswith("corners"):
            reaches, inside = sc.words_inside(case, ref, 0, (case["left"].shape[1] + 63) // 64 * 64)
            assert (reaches & ~inside & np.isin(ref["code"], KEPT) & (ref["level"] == 0)).sum() >= 2, name


def test_row_table_fill(refs):
    """Overflow and near-full, computed from the row bands as k_stereo_scan does (items = rows of every band inside the image; capacity 24 per slot)."""
    for name, want in (("wide_table", "fits"), ("wide_overflow", "overflows"), ("wide_nearfull", "near")):
        case, ref = refs[name]
        scale, _ = sc.scales(case["cfg"])
        items, cap = sc.row_table_items(case["kR"], scale, case["left"].shape[0]), sc.ROW_ITEMS_PER_KP * case["max_kps"]
        print(name, items, cap)
        if want == "overflows":
            assert items > cap
        elif want == "near":
            assert cap - 1 <= items <= cap
        else:
            assert items < cap // 2
        assert np.isin(ref["code"], KEPT).sum() >= 3, name
    for name, (case, ref) in refs.items():
        if not name.startswith("wide_"):
            scale, _ = sc.scales(case["cfg"])
            assert sc.row_table_items(case["kR"], scale, case["left"].shape[0]) <= sc.ROW_ITEMS_PER_KP * case["max_kps"], name


# ---- answers worked out by hand ----

def test_hand_clamp(refs):
    """Left and right mirror-symmetric about column 160, one keypoint pair at (160, 100) on level 0.  SAD(-1) == SAD(+1) by symmetry, so deltaR = 0 and
    bestuR = 1 * (160 + 0 + 0) = 160 = uL: disparity 0, which is clamped: disparity = 0.01f, bestuR = (float)(160.0 - 0.01), depth = bf / 0.01f."""
    case, ref = refs["clamp_single"]
    assert ref["code"][0] == ACCEPTED_CLAMP and ref["bestinc"][0] == 0 and ref["sad"][0] > 0 and ref["delta"][0] == 0
    assert ref["uRight"][0] == f32(160.0 - 0.01) and ref["depth"][0] == f32(sc.BF) / f32(0.01)


def test_hand_parabola(refs):
    """marker_pair with (a, p, q, r) = (40, 10, 40, 20), left keypoint at x = 100, right keypoint at x = 92:
    SAD(0) = |40 - 40| + 10 + 20 = 30, SAD(-1) = |40 - 10| + 40 + 20 = 90, SAD(+1) = |40 - 20| + 10 + 40 = 70, SAD(+-2 .. +-4) = 110, SAD(-5) = 90,
    SAD(+5) = 100.  The minimum 30 is at shift 0; deltaR = (90 - 70) / (2 * (90 + 70 - 2 * 30)) = 20 / 200 = 0.1f;
    bestuR = 1 * ((92 + 0) + 0.1f), disparity = 100 - bestuR (about 7.9), depth = bf / disparity.  One match: the median is its own SAD, 30 < 63."""
    case, ref = refs["parabola_single"]
    assert ref["sad"][0] == 30 and ref["bestinc"][0] == 0 and ref["delta"][0] == f32(20) / f32(200) and ref["code"][0] == ACCEPTED
    u = f32(92) + f32(0.1)
    assert ref["uRight"][0] == u and abs(float(u) - 92.1) < 1e-5
    assert ref["depth"][0] == f32(sc.BF) / (f32(100) - u) and abs(float(ref["depth"][0]) - 47.9 / 7.9) < 1e-4


def test_hand_median(refs):
    """1.4f = 0x3FB33333 = 1.39999997615814208984375; times 1.5 = 2.099999964237213134765625, which rounds to the float 0x40066666 =
    2.099999904632568359375.  Times 10 = 20.99999904632568359375 = 21 - 2^-20: exactly halfway between the floats 21 - 2^-19 and 21, and the tie goes to
    the even mantissa, 21.0.  So with median 10 a SAD of 21 is NOT below thDist and is cut, while 20 stays.  SADs 5 10 10 21 20: the sorted list is
    5 10 10 20 21, its element 5 / 2 = 2 is 10."""
    assert f32(1.5) * f32(1.4) * f32(10) == f32(21.0)
    case, ref = refs["median_threshold"]
    assert list(ref["sad"]) == [5, 10, 10, 21, 20] and ref["n_before"] == 5
    assert list(ref["code"]) == [ACCEPTED, ACCEPTED, ACCEPTED, CUT, ACCEPTED]
    # the even SADs have p == r: deltaR = 0 and uRight = uL - 8 exactly
    assert (ref["uRight"][[1, 2, 4]] == case["kL"]["x"][[1, 2, 4]] - f32(8)).all() and ref["uRight"][3] == -1 and ref["depth"][3] == -1
    # M = 1, 2, 3: the median is element M / 2 of the sorted list
    assert list(refs["median_m1"][1]["code"]) == [ACCEPTED]                                  # 12 < 2.1 * 12
    assert list(refs["median_m1_zero"][1]["code"]) == [CUT]                                  # median 0: 0 < 0 fails
    assert list(refs["median_m2"][1]["code"]) == [ACCEPTED, ACCEPTED]                        # median 30 (element 1), not 10, which would cut the 30
    assert list(refs["median_m3"][1]["code"]) == [ACCEPTED, ACCEPTED, CUT]                   # median 10: 30 >= 21
    assert (refs["median_equal"][1]["code"] == ACCEPTED).all() and (refs["median_equal"][1]["sad"] == 14).all()
    assert (refs["median_zero_majority"][1]["code"] == CUT).all() and refs["median_zero_majority"][1]["n_before"] == 5
    assert list(refs["median_zero_minority"][1]["code"]) == [ACCEPTED_CLAMP, ACCEPTED_CLAMP, ACCEPTED, ACCEPTED, ACCEPTED]   # median 5, thDist 10.5
    for name in ("median_m1", "median_m2", "median_m3", "median_equal", "median_zero_majority", "median_zero_minority"):
        assert list(refs[name][1]["sad"]) == refs[name][0]["sads"], name


def test_hand_shift_edge(refs):
    """A texture of horizontal period 5, left == right, keypoints at the same place: the right windows at shifts -5, 0 and +5 all equal the left window, SAD 0;
    the first of them, -5 = -L, is kept as the minimum and the match is dropped.  right[x] == left[x - 5] on a random texture: only shift +5 = +L has SAD 0."""
    case, ref = refs["periodic5_single"]
    assert ref["code"][0] == SHIFT_EDGE and ref["bestinc"][0] == -5 and ref["sad"][0] == 0 and ref["uRight"][0] == -1 and ref["depth"][0] == -1 and ref["n_before"] == 0
    case, ref = refs["shifted5"]
    assert (ref["code"] == SHIFT_EDGE).all() and (ref["bestinc"] == 5).all() and (ref["sad"] == 0).all() and (ref["uRight"] == -1).all()


def test_ground_truth_on_integer_shifts(refs):
    """Noise-free integer shift d, a level-0 keypoint whose chosen right keypoint lies exactly at (x - d, y): the SAD at shift 0 is 0, so the minimum is there
    (or at an earlier all-zero shift, which never happens on these textures) and uRight = x - d + deltaR with |deltaR| <= 0.5."""
    total = 0
    for name in ("shift9", "shift7_odd"):
        case, ref = refs[name]
        d = case["shift"]
        kL, kR = case["kL"], case["kR"]
        m = np.isin(ref["code"], KEPT) & (ref["level"] == 0)
        j = ref["best_r"][m]
        exact = (kR["x"][j] == kL["x"][m] - f32(d)) & (kR["y"][j] == kL["y"][m])
        err = np.abs(kL["x"][m][exact].astype(np.float64) - ref["uRight"][m][exact] - d)
        print(name, int(exact.sum()), float(err.max()))
        assert (err <= 0.5).all(), name
        total += int(exact.sum())
    assert total >= 30
