"""GPU: the object association (include/oslam_hip.h, "Object association") against the numpy restatement of tests/object_match_common.py.  Histogram counts are
exact and hist is bitwise; every matcher output is exact: the ids, the counts, and the score arrays bit for bit with their NaN pattern.  No tolerance anywhere:
every score is a fixed sequence of IEEE operations that the restatement repeats (the library is built without contraction), so none had to be bounded."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import object_match_common as omc
from object_slam_amd import object_match as om
from object_slam_amd._lib import OSLAM_E_CAPACITY, OSLAM_E_INVALID, OslamError, check

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "object_slam_amd")
f32 = np.float32
BINS = omc.BINS
FILL, FFILL, GAP = -77, f32(-7.5), 2     # what output rows hold before a call; rows between the problems that no problem owns


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same_scores(a, b):
    """bit for bit where a number stands, NaN where NaN stands"""
    a, b = np.asarray(a, f32).reshape(-1), np.asarray(b, f32).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(_bits(a[~na]), _bits(b[~nb]))


# ------------------------------------------------------------------ histograms ------------------------------------------------------------------

def _reference(img, W, masks, frames):
    H = img.shape[1]
    counts, hist = np.zeros((len(masks), BINS), np.int32), np.zeros((len(masks), BINS), f32)
    for f, fr in enumerate(frames):
        o, n = int(fr["mask_off"]), int(fr["n_masks"])
        px = img[f][:, :3 * W].reshape(H, W, 3)
        counts[o:o + n], hist[o:o + n] = omc.hsv_histograms(px, masks[o:o + n, :, :W])
    return counts, hist


def _check_hist(m, img, W, masks, frames=None, device=False):
    frames = om.pack_frames([len(masks) // len(img)] * len(img)) if frames is None else frames
    nm = len(masks)
    got = m.hsv_histograms(img, masks, frames=frames, width=W, counts=np.full((nm, BINS), FILL, np.int32), hist=np.full((nm, BINS), FFILL, f32), device=device)
    counts, hist = _reference(img, W, masks, frames)
    owned = np.zeros(nm, bool)
    for fr in frames:
        owned[fr["mask_off"]:fr["mask_off"] + fr["n_masks"]] = True
    assert np.array_equal(got["counts"][owned], counts[owned]) and np.array_equal(_bits(got["hist"][owned]), _bits(hist[owned]))
    assert (got["counts"][~owned] == FILL).all() and (got["hist"][~owned] == FFILL).all()
    return got


@pytest.fixture(scope="module")
def hm():
    m = om.ObjectMatcher(8, 128, 64, 32, 4, 16, 16)
    yield m
    m.close()


def test_histograms_64x48_two_masks_and_repeat(hm):
    rng = np.random.default_rng(11)
    img, _ = omc.gen_image(rng, 64, 48)
    masks = omc.gen_masks(rng, 2, 64, 48)
    a = _check_hist(hm, img[None], 64, masks)
    b = _check_hist(hm, img[None], 64, masks)
    assert a["counts"].tobytes() == b["counts"].tobytes() and a["hist"].tobytes() == b["hist"].tobytes()
    c = _check_hist(hm, img[None], 64, masks, device=True)
    assert a["counts"].tobytes() == c["counts"].tobytes() and a["hist"].tobytes() == c["hist"].tobytes()
    assert a["counts"].sum() > 0


def test_histograms_unaligned_rows(hm):
    """67 x 13, stride 3 * 67 + 5, mask stride 71: every row starts at another byte of a dword, and no band size divides the height"""
    rng = np.random.default_rng(12)
    img, _ = omc.gen_image(rng, 67, 13, stride=3 * 67 + 5)
    masks = omc.gen_masks(rng, 3, 67, 13, mask_stride=71, values=(0, 1, 2, 128, 255))    # mask bytes other than 0 and 255
    _check_hist(hm, img[None], 67, masks)
    _check_hist(hm, img[None], 67, masks, device=True)


def test_histograms_one_pixel_empty_full_and_overlapping_masks(hm):
    rng = np.random.default_rng(13)
    img = np.array([[[200, 30, 90]]], np.uint8).reshape(1, 1, 3)
    got = _check_hist(hm, img, 1, np.array([5, 0], np.uint8).reshape(2, 1, 1))
    assert got["counts"][0].sum() == 3 and (got["counts"][1] == 0).all() and (got["hist"][1] == 0).all()
    img, _ = omc.gen_image(rng, 45, 37)
    masks = np.zeros((4, 37, 45), np.uint8)
    masks[1] = 255                     # full
    masks[2, 5:30, 3:40] = 9           # overlapping
    masks[3, 20:37, 10:45] = 200
    got = _check_hist(hm, img[None], 45, masks)
    assert (got["counts"][0] == 0).all() and (got["hist"][0] == 0).all() and got["counts"][1].sum() == 3 * 45 * 37


def test_histograms_8_and_max_detections_masks(hm):
    rng = np.random.default_rng(14)
    img, _ = omc.gen_image(rng, 50, 40)
    for n in (8, 32):
        _check_hist(hm, img[None], 50, omc.gen_masks(rng, n, 50, 40))


def test_histograms_batch_of_frames_with_different_counts(hm):
    rng = np.random.default_rng(15)
    W, H, ns = 70, 35, [3, 0, 8, 1, 2]
    img = np.stack([omc.gen_image(rng, W, H, stride=3 * W + 2)[0] for _ in ns])
    offs = np.cumsum([1] + [n + 1 for n in ns[:-1]])      # a row no frame owns before every frame's masks
    masks = omc.gen_masks(rng, int(offs[-1]) + ns[-1] + 1, W, H)
    frames = om.pack_frames(ns, offs)
    _check_hist(hm, img, W, masks, frames)
    _check_hist(hm, img, W, masks, frames, device=True)


def test_histograms_every_24_bit_colour():
    """4096 x 4096, every colour once: the conversion over its whole domain, 128 bands; the masks cut the image along a pattern unrelated to the colour order"""
    c = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([c & 255, (c >> 8) & 255, c >> 16], 1).astype(np.uint8).reshape(1, 4096, 3 * 4096)
    y, x = np.divmod(c, np.uint32(4096))
    key = ((x * np.uint32(2654435761) + y * np.uint32(40503)) >> np.uint32(9)) & np.uint32(15)
    masks = np.stack([((key == k) | (key == k + 8) | ((key == 15 - k) & (k < 3))) for k in range(8)]).astype(np.uint8).reshape(8, 4096, 4096) * np.uint8(3)
    h, s, v = omc.bgr2hsv(c & 255, (c >> 8) & 255, c >> 16)
    _, _, cols = omc.hsv_tables()
    # the masks are unions of the 16 classes of `key`: one histogram per class, summed per mask
    per_key = sum(np.bincount(key.astype(np.int64) * BINS + col, minlength=16 * BINS) for col in (cols["v"][v], cols["s"][s], cols["h"][h])).reshape(16, BINS)
    want = np.array([per_key[[j for j in range(16) if j == k or j == k + 8 or (j == 15 - k and k < 3)]].sum(0) for k in range(8)])
    assert all(want[k].sum() == 3 * np.count_nonzero(masks[k]) for k in range(8)) and min(cols["v"].min(), cols["s"].min(), cols["h"][:180].min()) >= 0 and h.max() < 180
    m = om.ObjectMatcher(1, 4096, 4096, 8, 1, 1, 1)
    try:
        got = m.hsv_histograms(img, masks, width=4096)
    finally:
        m.close()
    assert np.array_equal(got["counts"], want) and want.sum() > 3 * (1 << 24)
    assert np.array_equal(_bits(got["hist"]), _bits(np.array([omc.normalize_l1(w) for w in want])))


# ------------------------------------------------------------------ matchers ------------------------------------------------------------------

def _pack_two(problems):
    """records and rows of a batch; GAP rows that no problem owns before every problem's rows and scores"""
    pre = dict(obj3d=[], label=[], hist=[], box=[])
    cur = dict(obj3d=[], label=[], hist=[], box=[])
    recs = []
    pad = lambda d, n: [d[k].append(np.full((n,) + s, FILL, t)) for k, t, s in (("obj3d", np.int32, ()), ("label", np.int32, ()), ("hist", f32, (BINS,)), ("box", f32, (4,)))]
    po = co = so = 0
    for p in problems:
        pad(pre, GAP), pad(cur, GAP)
        po, co, so = po + GAP, co + GAP, so + GAP
        for k in pre:
            pre[k].append(np.asarray(p["pre"][k])), cur[k].append(np.asarray(p["cur"][k]))
        n_pre, n_cur = len(p["pre"]["label"]), len(p["cur"]["label"])
        recs.append((n_pre, po, n_cur, co, so))
        po, co, so = po + n_pre, co + n_cur, so + n_pre * n_cur
    cat = lambda d: dict(obj3d=np.concatenate(d["obj3d"]).astype(np.int32), label=np.concatenate(d["label"]).astype(np.int32), hist=np.concatenate(d["hist"]).astype(f32).reshape(-1, BINS),
                         box=np.concatenate(d["box"]).astype(f32).reshape(-1, 4))
    r = np.array(recs, np.int64).reshape(-1, 5)
    return om.pack_pair_problems(r[:, 0], r[:, 2], r[:, 1], r[:, 3], r[:, 4]), cat(pre), cat(cur), so


def _run_two(m, problems, device=False, params=None, recs=None):
    pr, pre, cur, ns = _pack_two(problems)
    pr = pr if recs is None else recs(pr)
    n = len(pr)
    raw = m.match_two_frame(pr, pre, cur, params=params, similarity=np.full(ns, FFILL, f32), iou=np.full(ns, FFILL, f32), n_assigned=np.full(n, FILL, np.int32),
                            status=np.full(n, FILL, np.int32), device=device)
    out = []
    for q in pr:
        s, k = slice(q["off_score"], q["off_score"] + q["n_pre"] * q["n_cur"]), slice(q["off_cur"], q["off_cur"] + q["n_cur"])
        out.append((raw["cur_obj3d"][k].copy(), raw["similarity"][s].copy(), raw["iou"][s].copy(), int(raw["n_assigned"][len(out)]), int(raw["status"][len(out)])))
    return out, raw, pr


def _ok_two(got, ref):
    return np.array_equal(got[0], ref[0]) and _same_scores(got[1], ref[1]) and _same_scores(got[2], ref[2]) and got[3] == ref[3] and got[4] == omc.DONE


def _pack_map(problems):
    cur = dict(obj3d=[], label=[], hist=[], kp_off=[], kp_n=[])
    obj = dict(obj3d_id=[], label=[], obs_off=[], obs_n=[])
    kps, ocen, ohist, recs = [np.full((GAP, 3), FFILL, f32)], [np.full((GAP, 3), FFILL, f32)], [np.full((GAP, BINS), FFILL, f32)], []
    nk = no = GAP
    co = oo = so = 0
    for p in problems:
        for d, keys in ((cur, cur), (obj, obj)):
            for k in keys:
                d[k].append(np.full(GAP, FILL, np.int32) if k != "hist" else np.full((GAP, BINS), FFILL, f32))
        co, oo, so = co + GAP, oo + GAP, so + GAP
        c, o = p["cur"], p["objs"]
        n_cur, n_obj = len(c["label"]), len(o["label"])
        cur["obj3d"].append(np.asarray(c["obj3d"], np.int32)), cur["label"].append(np.asarray(c["label"], np.int32)), cur["hist"].append(np.asarray(c["hist"], f32).reshape(-1, BINS))
        cur["kp_off"].append(np.array([nk + sum(len(q) for q in c["kps"][:j]) for j in range(n_cur)], np.int32)), cur["kp_n"].append(np.array([len(q) for q in c["kps"]], np.int32))
        kps += [np.asarray(q, f32).reshape(-1, 3) for q in c["kps"]]
        nk += sum(len(q) for q in c["kps"])
        obj["obj3d_id"].append(np.asarray(o["id"], np.int32)), obj["label"].append(np.asarray(o["label"], np.int32))
        obj["obs_off"].append(np.array([no + sum(len(q) for q in o["obs_center"][:i]) for i in range(n_obj)], np.int32)), obj["obs_n"].append(np.array([len(q) for q in o["obs_center"]], np.int32))
        ocen += [np.asarray(q, f32).reshape(-1, 3) for q in o["obs_center"]]
        ohist += [np.asarray(q, f32).reshape(-1, BINS) for q in o["obs_hist"]]
        no += sum(len(q) for q in o["obs_center"])
        recs.append((n_cur, co, n_obj, oo, so))
        co, oo, so = co + n_cur, oo + n_obj, so + n_obj * n_cur
    cur = {k: np.concatenate(v) for k, v in cur.items()}
    obj = {k: np.concatenate(v) for k, v in obj.items()}
    cur["kps"], obj["obs_center"], obj["obs_hist"] = np.concatenate(kps), np.concatenate(ocen), np.concatenate(ohist)
    r = np.array(recs, np.int64).reshape(-1, 5)
    pr = om.pack_map_problems(r[:, 0], r[:, 2], [p["Rwc"] for p in problems], [p["Ow"] for p in problems], [p["K"] for p in problems], r[:, 1], r[:, 3], r[:, 4])
    return pr, cur, obj, so


def _run_map(m, problems, device=False, params=None, edit=None):
    pr, cur, obj, ns = _pack_map(problems)
    if edit is not None:
        edit(pr, cur, obj)
    n = len(pr)
    raw = m.match_map_to_frame(pr, cur, obj, params=params, similarity=np.full(ns, FFILL, f32), mean_dist=np.full(ns, FFILL, f32), min_dist=np.full(ns, FFILL, f32),
                               n_by_similarity=np.full(n, FILL, np.int32), n_by_distance=np.full(n, FILL, np.int32), status=np.full(n, FILL, np.int32), device=device)
    out = []
    for q in pr:
        s, k = slice(q["off_score"], q["off_score"] + q["n_obj"] * q["n_cur"]), slice(q["off_cur"], q["off_cur"] + q["n_cur"])
        b = len(out)
        out.append((raw["cur_obj3d"][k].copy(), raw["similarity"][s].copy(), raw["mean_dist"][s].copy(), raw["min_dist"][s].copy(), int(raw["n_by_similarity"][b]),
                    int(raw["n_by_distance"][b]), int(raw["status"][b])))
    return out, raw, pr


def _ok_map(got, ref):
    return np.array_equal(got[0], ref[0]) and all(_same_scores(got[k], ref[k]) for k in (1, 2, 3)) and got[4:6] == tuple(ref[4:6]) and got[6] == omc.DONE


@pytest.fixture(scope="module")
def matcher():
    m = om.ObjectMatcher(256, 128, 64, 8, 16, 1 << 16, 1 << 16)
    yield m
    m.close()


@pytest.fixture(scope="module")
def two():
    hand = omc.hand_cases_two_frame()
    ps, ans = omc.generated_two_frame()
    names = sorted(hand)
    return dict(problems=[hand[k] for k in names] + list(ps), ref=[omc.match_two_frame(hand[k]) for k in names] + list(ans), names=names)


@pytest.fixture(scope="module")
def mapb():
    hand = omc.hand_cases_map()
    ps, ans = omc.generated_map()
    names = sorted(hand)
    return dict(problems=[hand[k] for k in names] + list(ps), ref=[omc.match_map_to_frame(hand[k]) for k in names] + list(ans), names=names)


@pytest.fixture(scope="module")
def two_first(matcher, two):
    return _run_two(matcher, two["problems"])


@pytest.fixture(scope="module")
def map_first(matcher, mapb):
    return _run_map(matcher, mapb["problems"])


def test_two_frame_parity_and_hand_answers(two, two_first):
    got = two_first[0]
    bad = [j for j, (g, r) in enumerate(zip(got, two["ref"])) if not _ok_two(g, r)]
    print("two-frame: %d problems, %d assign, differing: %s" % (len(got), sum(g[3] > 0 for g in got), bad))
    assert not bad
    for name, g in zip(two["names"], got):
        e = omc.hand_cases_two_frame()[name]["expect"]
        assert g[0].tolist() == e["cur"] and g[3] == e["n"], name


def test_map_parity_and_hand_answers(mapb, map_first):
    got = map_first[0]
    bad = [j for j, (g, r) in enumerate(zip(got, mapb["ref"])) if not _ok_map(g, r)]
    print("map: %d problems, by similarity in %d, by distance in %d, differing: %s" % (len(got), sum(g[4] > 0 for g in got), sum(g[5] > 0 for g in got), bad))
    assert not bad
    for name, g in zip(mapb["names"], got):
        e = omc.hand_cases_map()[name]["expect"]
        assert g[0].tolist() == e["cur"] and g[4:6] == (e["by_sim"], e["by_dist"]), name


def test_rows_no_problem_owns_keep_their_fill(two_first, map_first):
    for (_, raw, pr), n1, keys in ((two_first, "n_pre", ("similarity", "iou")), (map_first, "n_obj", ("similarity", "mean_dist", "min_dist"))):
        owned_s, owned_c = np.zeros(len(raw["similarity"]), bool), np.zeros(len(raw["cur_obj3d"]), bool)
        for q in pr:
            owned_s[q["off_score"]:q["off_score"] + q[n1] * q["n_cur"]] = True
            owned_c[q["off_cur"]:q["off_cur"] + q["n_cur"]] = True
        assert (~owned_c).sum() == GAP * len(pr) and (raw["cur_obj3d"][~owned_c] == FILL).all() and (raw["cur_obj3d"][owned_c] != FILL).all()
        for k in keys:
            assert (raw[k][~owned_s] == FFILL).all() and (raw[k][owned_s] != FFILL).all()


def test_problems_are_independent(matcher, two, mapb, two_first, map_first):
    order = np.random.default_rng(5).permutation(len(two["problems"]))
    got = _run_two(matcher, [two["problems"][j] for j in order])[0]
    assert all(_ok_two(g, two["ref"][j]) for g, j in zip(got, order))
    for j in range(0, len(two["problems"]), 37):
        assert _ok_two(_run_two(matcher, [two["problems"][j]])[0][0], two["ref"][j])
    order = np.random.default_rng(6).permutation(len(mapb["problems"]))
    got = _run_map(matcher, [mapb["problems"][j] for j in order])[0]
    assert all(_ok_map(g, mapb["ref"][j]) for g, j in zip(got, order))
    for j in range(0, len(mapb["problems"]), 37):
        assert _ok_map(_run_map(matcher, [mapb["problems"][j]])[0][0], mapb["ref"][j])


def test_host_and_device_entry_points_agree_and_calls_repeat(matcher, two, mapb, two_first, map_first):
    for device in (True, False):
        _, raw, _ = _run_two(matcher, two["problems"], device=device)
        assert all(raw[k].tobytes() == two_first[1][k].tobytes() for k in ("cur_obj3d", "similarity", "iou", "n_assigned", "status"))
        _, raw, _ = _run_map(matcher, mapb["problems"], device=device)
        assert all(raw[k].tobytes() == map_first[1][k].tobytes() for k in ("cur_obj3d", "similarity", "mean_dist", "min_dist", "n_by_similarity", "n_by_distance", "status"))


def test_thresholds_are_parameters(matcher, two, mapb):
    loose = dict(min_similarity=0.5, min_iou=0.2, max_mean_dist=5.0, max_min_dist=0.25)
    ps = two["problems"][-40:]
    got = _run_two(matcher, ps, params=om.make_params(**loose))[0]
    ref = [omc.match_two_frame(p, loose) for p in ps]
    assert all(_ok_two(g, r) for g, r in zip(got, ref)) and sum(r[3] for r in ref) > sum(r[3] for r in two["ref"][-40:])
    ps = mapb["problems"][-40:]
    got = _run_map(matcher, ps, params=om.make_params(**loose))[0]
    ref = [omc.match_map_to_frame(p, loose) for p in ps]
    assert all(_ok_map(g, r) for g, r in zip(got, ref)) and sum(r[4] + r[5] for r in ref) > sum(r[4] + r[5] for r in mapb["ref"][-40:])


def test_capacity_refusals_launch_nothing(matcher, two, mapb):
    small = om.ObjectMatcher(2, 64, 48, 8, 4, 64, 64)
    try:
        for device in (False, True):
            with pytest.raises(OslamError) as ei:          # three problems, two allowed
                _run_two(small, two["problems"][:3], device=device)
            assert ei.value.code == OSLAM_E_CAPACITY
            with pytest.raises(OslamError) as ei:          # an object of 129 observations, max_observations_total is 64
                _run_map(small, [mapb["problems"][len(mapb["names"]) + 7]], device=device)
            assert ei.value.code == OSLAM_E_CAPACITY
        # the host path writes its outputs only after the launch: a refused call leaves them as they were
        pr, pre, cur, ns = _pack_two(two["problems"][:3])
        outs = dict(similarity=np.full(ns, FFILL, f32), iou=np.full(ns, FFILL, f32), n_assigned=np.full(3, FILL, np.int32), status=np.full(3, FILL, np.int32))
        before = cur["obj3d"].copy()
        with pytest.raises(OslamError):
            small.match_two_frame(pr, pre, cur, **outs)
        assert np.array_equal(cur["obj3d"], before) and all((v == (FFILL if v.dtype == f32 else FILL)).all() for v in outs.values())
        img = np.zeros((1, 48, 3 * 65), np.uint8)
        with pytest.raises(OslamError) as ei:              # 65 columns, 64 allowed
            small.hsv_histograms(img, np.zeros((1, 48, 65), np.uint8), width=65)
        assert ei.value.code == OSLAM_E_CAPACITY
        with pytest.raises(OslamError) as ei:              # nine masks in a frame, eight allowed
            small.hsv_histograms(np.zeros((1, 8, 24), np.uint8), np.zeros((9, 8, 8), np.uint8), width=8)
        assert ei.value.code == OSLAM_E_CAPACITY
    finally:
        small.close()
    for bad in (7, 33):
        with pytest.raises(OslamError) as ei:
            om.ObjectMatcher(2, 64, 48, bad)
        assert ei.value.code == OSLAM_E_INVALID


def test_precondition_refusals_confine_themselves_to_their_problem(matcher, mapb, map_first):
    """an object without observations, a detection without keypoints and a range outside the flat arrays: the problem gets its status and nothing else of it is
    written; its neighbours in the batch are what they were"""
    idx = [j for j, p in enumerate(mapb["problems"]) if len(p["cur"]["label"]) >= 2 and len(p["objs"]["label"]) >= 2][:3]
    assert len(idx) == 3
    ps, ref = [mapb["problems"][j] for j in idx], [mapb["ref"][j] for j in idx]

    def no_obs(pr, cur, obj):
        obj["obs_n"][pr["off_obj"][1] + 1] = 0

    def no_kps(pr, cur, obj):
        cur["kp_n"][pr["off_cur"][1]] = 0

    def obs_outside(pr, cur, obj):
        obj["obs_off"][pr["off_obj"][1]] = len(obj["obs_center"]) - obj["obs_n"][pr["off_obj"][1]] + 1

    def kps_outside(pr, cur, obj):
        cur["kp_off"][pr["off_cur"][1] + 1] = -1

    def too_many_objects(pr, cur, obj):
        pr["n_obj"][1] = 17

    for device in (False, True):
        for edit, status in ((no_obs, omc.REFUSED_NO_OBSERVATION), (no_kps, omc.REFUSED_NO_KEYPOINT), (obs_outside, omc.REFUSED_RECORD), (kps_outside, omc.REFUSED_RECORD),
                             (too_many_objects, omc.REFUSED_RECORD)):
            got, raw, pr = _run_map(matcher, ps, device=device, edit=edit)
            assert _ok_map(got[0], ref[0]) and _ok_map(got[2], ref[2]), edit.__name__
            q = pr[1]
            k = slice(q["off_cur"], q["off_cur"] + q["n_cur"])
            assert got[1][6] == status and got[1][4] == FILL and got[1][5] == FILL and np.array_equal(raw["cur_obj3d"][k], ps[1]["cur"]["obj3d"]), edit.__name__
            n_scores = len(ps[1]["objs"]["label"]) * q["n_cur"]
            assert all((raw[key][q["off_score"]:q["off_score"] + n_scores] == FFILL).all() for key in ("similarity", "mean_dist", "min_dist")), edit.__name__
    # MatchTwoFrame: a record outside the rows
    from_two = omc.generated_two_frame()
    sel = [j for j, p in enumerate(from_two[0]) if len(p["cur"]["label"]) >= 1 and len(p["pre"]["label"]) >= 1][:3]
    ps2, ref2 = [from_two[0][j] for j in sel], [from_two[1][j] for j in sel]

    def outside(pr):
        pr = pr.copy()
        pr["off_pre"][1] = 1 << 20
        return pr
    got, raw, pr = _run_two(matcher, ps2, recs=outside)
    assert _ok_two(got[0], ref2[0]) and _ok_two(got[2], ref2[2]) and got[1][4] == omc.REFUSED_RECORD and got[1][3] == FILL and (got[1][1] == FFILL).all()
    assert np.array_equal(got[1][0], ps2[1]["cur"]["obj3d"])


def test_histograms_chain_into_match_two_frame_on_one_stream(matcher):
    """the histograms of two frames stay on the device and are the pre and cur rows of oslam_objmatch_match_two_frame_device on the same stream: the outcome is
    that of the host path fed the downloaded histograms"""
    import torch
    from object_slam_amd._lib import upload
    frames = omc.fixture_frames()
    A, B = frames[0], frames[1]
    W, H = omc.FIXTURE_W, omc.FIXTURE_H
    img = np.stack([A["image"], B["image"]])
    masks = np.array([d["mask"] for d in A["dets"]] + [d["mask"] for d in B["dets"]], np.uint8)
    nA, nB = len(A["dets"]), len(B["dets"])
    fr = om.pack_frames([nA, nB])
    host = matcher.hsv_histograms(img, masks, frames=fr, width=W)
    boxes = np.array([d["box"] for d in A["dets"]] + [d["box"] for d in B["dets"]], f32)
    labels = np.array([d["label"] for d in A["dets"]] + [d["label"] for d in B["dets"]], np.int32)
    pre_ids, cur_ids = np.arange(nA, dtype=np.int32) + 40, np.full(nB, -1, np.int32)
    pr = om.pack_pair_problems([nA], [nB])
    want = matcher.match_two_frame(pr, dict(obj3d=pre_ids, label=labels[:nA], hist=host["hist"][:nA], box=boxes[:nA]),
                                   dict(obj3d=cur_ids.copy(), label=labels[nA:], hist=host["hist"][nA:], box=boxes[nA:]))
    assert want["n_assigned"][0] == 3 and want["status"][0] == 0
    ins = dict(img=img, masks=masks, fr=fr, counts=np.zeros((nA + nB, BINS), np.int32), hist=np.zeros((nA + nB, BINS), f32), boxes=boxes, labels=labels, pre_ids=pre_ids, cur_ids=cur_ids, pr=pr,
               sim=np.full(nA * nB, FFILL, f32), iou=np.full(nA * nB, FFILL, f32), nas=np.full(1, FILL, np.int32), st=np.full(1, FILL, np.int32))
    t = {k: upload(v) for k, v in ins.items()}
    a = lambda k, off=0: t[k].data_ptr() + off
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    stream = C.c_void_p(side.cuda_stream)
    rp = om.DetRows(nA, a("labels"), a("hist"), a("boxes"), a("pre_ids"), None, None, 0, None)
    rc = om.DetRows(nB, a("labels", 4 * nA), a("hist", 4 * BINS * nA), a("boxes", 16 * nA), a("cur_ids"), None, None, 0, None)
    prm = om.make_params()
    with torch.cuda.stream(side):
        check(matcher.L.oslam_objmatch_hsv_histograms_device(matcher.h, 2, W, H, 3 * W, W, a("img"), a("fr"), nA + nB, a("masks"), a("counts"), a("hist"), stream))
        check(matcher.L.oslam_objmatch_match_two_frame_device(matcher.h, 1, a("pr"), C.byref(rp), C.byref(rc), C.byref(prm), nA * nB, a("sim"), a("iou"), a("nas"), a("st"), stream))
    side.synchronize()
    back = lambda k: t[k].cpu().numpy()[:ins[k].nbytes].view(ins[k].dtype).reshape(ins[k].shape)
    assert np.array_equal(_bits(back("hist")), _bits(host["hist"])) and np.array_equal(back("cur_ids"), want["cur_obj3d"])
    assert _same_scores(back("sim"), want["similarity"]) and _same_scores(back("iou"), want["iou"]) and back("nas")[0] == 3 and back("st")[0] == 0


def test_timing_gives_kernel_milliseconds(hm):
    rng = np.random.default_rng(16)
    img, _ = omc.gen_image(rng, 64, 48)
    hm.set_timing(True)
    try:
        hm.hsv_histograms(img[None], omc.gen_masks(rng, 2, 64, 48), width=64)
        ms = hm.last_kernel_ms()
        assert ms[0] > 0 and ms[1] > 0
    finally:
        hm.set_timing(False)


def test_adapter_program_matches_the_restatement(tmp_path):
    from object_slam_amd import build
    build.build_hip()
    prog = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adapter_object_program.cc"), "-o", prog,
                           "-L", LIBDIR, "-loslam_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    frames = omc.fixture_frames()
    want, claims = omc.track_fixture(frames)
    d = str(tmp_path / "fixture")
    os.makedirs(d)
    hx = lambda v: " ".join(float(x).hex() for x in np.asarray(v, f32).reshape(-1))
    K = omc.FIXTURE_K
    with open(os.path.join(d, "meta.txt"), "w") as f:
        for k, v in dict(n_frames=len(frames), width=omc.FIXTURE_W, height=omc.FIXTURE_H, fx=K[0], fy=K[1], cx=K[2], cy=K[3]).items():
            f.write("%s %r\n" % (k, float(v)))
    for j, F in enumerate(frames):
        F["image"].tofile(os.path.join(d, "image_%d.bin" % j))
        np.array([x["mask"] for x in F["dets"]], np.uint8).tofile(os.path.join(d, "masks_%d.bin" % j))
        with open(os.path.join(d, "frame_%d.txt" % j), "w") as f:
            f.write("Rwc %s\nOw %s\nn_det %d\n" % (hx(F["Rwc"]), hx(F["Ow"]), len(F["dets"])))
            for x in F["dets"]:
                f.write("det %d %s %d\nkps %s\ncenter %s\n" % (x["label"], hx(x["box"]), len(x["kps"]), hx(x["kps"]), hx(x["center"])))
    r = subprocess.run([prog, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [[int(v) for v in l.split()[3:]] for l in r.stdout.split("\n") if l.startswith("frame ")]
    print(got, claims)
    assert got == want and want == [[x["truth"] for x in F["dets"]] for F in frames]
