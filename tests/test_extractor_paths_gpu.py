"""GPU parity of every ORB extractor kernel variant: the geometry, the scale factor, the batch size and the alignment of the caller's device buffer
decide which kernels launch_batch() runs (three resize kernels, word / byte loads of level 0, 1 / 4 / 16 keypoints per wavefront, halves, the two
FAST kernels, three quad-tree storages, two blur roundings).  Every case compares all stages bit-exact with the CPU oracle, asserts FROM THE PLAN
RECORD of the handle (ORBextractor.debug_plan: written where the library takes the decision) that the variant it is meant to pin really ran, and
asserts a non-trivial keypoint count.  Shapes are the smallest that select the variant; the oracle needs about 5 ms per 160 x 120 image."""
import numpy as np
import pytest

from extractor_common import Layout, oracle_ref, run_stages
from object_slam_amd import ORBextractor, OslamError, synth
from object_slam_amd._lib import OSLAM_E_INVALID
from object_slam_amd.extractor import RESIZE_LDS, RESIZE_NONE, RESIZE_PLAIN, RESIZE_WORDS

pytestmark = pytest.mark.gpu

MIN_KPS = 50   # a non-trivial result: the oracle finds 59 and 78 keypoints in the two poorest images below (131 x 97, structured) and 130 to 304 in the others


def _cfg(nfeatures, scale, nlevels):
    return dict(nfeatures=nfeatures, scaleFactor=scale, nlevels=nlevels, iniThFAST=20, minThFAST=7)


def _structured(w, h, seed=5):
    return synth.make_stream(1, w, h, seed=seed)[0][0]


def _noise(w, h, seed=11):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w)).astype(np.uint8)


def _both(w, h):
    return (("structured", _structured(w, h)), ("noise", _noise(w, h)))


# ---- a. resize variants (host entry: the staged level 0 is 64-byte aligned, so the tables of the level decide alone) ----

# (width, height, levels, scale factor, resize kernel per level)
RESIZE_CASES = [
    # tap distance 7 inside a quad: no quad tables.  Level 1 is 128 x 96
    (320, 240, 2, 2.5, [RESIZE_NONE, RESIZE_PLAIN]),
    # quad tables fit, 16 destination rows need 33 source rows (LDS tile: 24)
    (320, 240, 2, 2.0, [RESIZE_NONE, RESIZE_WORDS]),
    # 16 destination rows need 24 or 25 source rows depending on the phase: level 1 (320 -> 213) fits the LDS tile in every tile, level 2 (213 -> 142) does not
    (320, 240, 3, 1.5, [RESIZE_NONE, RESIZE_LDS, RESIZE_WORDS]),
    # one partial tile in x and a partial last tile in y on every level (136 x 101, 113 x 84, 94 x 70); widths 163, 113 and 94 are no multiple of 4
    (163, 121, 4, 1.2, [RESIZE_NONE, RESIZE_LDS, RESIZE_LDS, RESIZE_LDS]),
    # level 1 is 427 x 83: a full and a partial 256-pixel tile in x, five full and one partial 16-row tile in y
    (512, 100, 2, 1.2, [RESIZE_NONE, RESIZE_LDS]),
]


@pytest.mark.parametrize("w,h,nlevels,scale,resize", RESIZE_CASES, ids=lambda v: None if isinstance(v, list) else str(v))
def test_resize_variants(oracle, w, h, nlevels, scale, resize):
    cfg = _cfg(300, scale, nlevels)
    for name, img in _both(w, h):
        counts, plan, _ = run_stages(oracle, cfg, img)
        assert len(plan["halves"]) == 1 and plan["halves"][0]["resize"] == resize, (name, plan)
        assert plan["halves"][0]["src_aligned4"] and plan["halves"][0]["src_aligned16"]
        assert counts[0] >= MIN_KPS, (name, counts)
    if (w, h) == (163, 121):   # a partial last quad of pixels on levels 0, 2 and 3 (level 1 is 136 wide)
        assert [lv["size"][0] % 4 for lv in oracle_ref(oracle, cfg, img)["levels"]] == [3, 0, 1, 2]


# ---- b. unaligned and padded level-0 sources ----

# Level 0 of 163 x 121 (4 levels) has 33 x 45 cells and goes to k_fast_cells; level 0 of 131 x 97 (3 levels) has 33 x 33 cells and goes to
# k_fast_cells_wave, whose loads (unlike k_fast_cells') depend on the alignment.  (width, height, levels, level 0 is a big-cell level, resize of levels >= 2)
GEOMETRIES = {"163x121": (163, 121, 4, True, [RESIZE_LDS, RESIZE_LDS]), "131x97": (131, 97, 3, False, [RESIZE_LDS])}

# name -> (base offset, row stride - aligned width, gap between images, level-0 rows 4-byte aligned, 16-byte aligned, level-1 resize kernel), with
# aligned width = the width rounded up to 4 (164 and 132).  Unaligned rows: k_resize at level 1 and the byte paths of k_fast_cells_wave,
# k_blur_strip (every strip is a border strip) and k_orient_describe, which test the same pitch and pointer bits as launch_batch()
LAYOUTS = {
    "tight": (0, None, 0, False, False, RESIZE_PLAIN),           # stride = width: nothing is aligned
    "base_plus_1": (1, 0, 0, False, False, RESIZE_PLAIN),
    "base_plus_3": (3, 0, 0, False, False, RESIZE_PLAIN),
    "images_4_aligned": (0, 0, 4, True, False, RESIZE_WORDS),    # 4-aligned rows and images, but no 16-byte alignment: word paths
    "stride_192": (0, 192, 0, True, True, RESIZE_LDS),           # padded rows, 16-byte aligned
}


def _images0(w, h):
    return np.stack([_structured(w, h, 5), _structured(w, h, 9), _noise(w, h)])


@pytest.mark.parametrize("fill", [0, 255])
@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_level0_layouts(oracle, geometry, name, fill):
    """Batch 3, so that the image stride matters; all three elements with full stage parity.  The bytes outside the image rows are 0 in one run
    and 255 in the other and both equal the oracle: no padding byte reaches a result (the word paths do load them)."""
    w, h, nlevels, big0, resize_up = GEOMETRIES[geometry]
    base, stride, gap, al4, al16, resize1 = LAYOUTS[name]
    stride = w if stride is None else (stride or (w + 3) // 4 * 4)
    layout = Layout(base, stride, stride * h + gap)
    counts, plan, _ = run_stages(oracle, _cfg(300, 1.2, nlevels), _images0(w, h), layout=layout, fill=fill)
    half, = plan["halves"]
    assert (half["src_aligned4"], half["src_aligned16"]) == (al4, al16), plan
    assert half["resize"] == [RESIZE_NONE, resize1] + resize_up, plan
    assert plan["big_cell"][0] == big0 and half["nb"] == 3 and half["kpw"] == 1, plan
    assert min(counts) >= MIN_KPS, counts


# ---- c. keypoints per wavefront of k_orient_describe ----

CFG_B = _cfg(300, 1.2, 4)
EMPTY, NOISE = 2, 5   # batch elements replaced by a constant image (no keypoint) and by noise (quota reached)


def _batch_images(n):
    imgs = synth.make_stream(n, 160, 120, seed=3)[0].copy()
    imgs[EMPTY] = 128
    imgs[NOISE] = _noise(160, 120)
    return imgs


def _check_batch_counts(counts):
    assert counts[EMPTY] == 0 and counts[NOISE] >= 290, counts
    rest = [c for i, c in enumerate(counts) if i not in (EMPTY, NOISE)]
    assert min(rest) >= MIN_KPS, counts


@pytest.mark.parametrize("batch,kpw", [(7, 1), (8, 4), (31, 4), (32, 16), (33, 16)])
def test_orient_describe_batch_sizes(oracle, batch, kpw):
    imgs = _batch_images(33)[:batch]
    named = (0, EMPTY, NOISE, batch - 1)
    counts, plan, out = run_stages(oracle, CFG_B, imgs, layout=Layout(0, 160, 160 * 120), full=named)
    half, = plan["halves"]
    assert (half["nb"], half["kpw"]) == (batch, kpw), plan
    _check_batch_counts(counts)
    if batch >= 32:   # the slots of a wavefront are filled at every residue of the count
        assert len(set(c % 16 for c in counts)) >= 8, counts
    # a result does not depend on its batch: the same bytes from a handle with batch 1
    for b in (0, EMPTY, batch - 1):
        _, plan1, one = run_stages(oracle, CFG_B, imgs[b:b + 1], layout=Layout(0, 160, 160 * 120), full=())
        assert plan1["halves"][0]["kpw"] == 1
        assert one[0][0].tobytes() == out[b][0].tobytes() and one[0][1].tobytes() == out[b][1].tobytes(), b


# ---- d. batches cut in two halves ----

@pytest.mark.parametrize("batch,halves", [(7, [(3, 1), (4, 1)]), (17, [(8, 4), (9, 4)]), (65, [(32, 16), (33, 16)])])
def test_unequal_halves(oracle, monkeypatch, batch, halves):
    imgs = _batch_images(batch)
    layout = Layout(0, 160, 160 * 120)
    named = (0, EMPTY, NOISE, halves[0][0] - 1, halves[0][0], batch - 1)   # both sides of the cut
    counts, plan, ref = run_stages(oracle, CFG_B, imgs, layout=layout, full=())
    assert [(x["nb"], x["kpw"]) for x in plan["halves"]] == [(batch, halves[1][1])], plan
    monkeypatch.setenv("OSLAM_ORB_SPLIT_MIN", "2")
    counts, plan, got = run_stages(oracle, CFG_B, imgs, layout=layout, full=named)
    monkeypatch.delenv("OSLAM_ORB_SPLIT_MIN")
    assert [(x["nb"], x["kpw"]) for x in plan["halves"]] == halves, plan
    assert plan["halves"][0]["resize"] == plan["halves"][1]["resize"] == [RESIZE_NONE, RESIZE_LDS, RESIZE_LDS, RESIZE_LDS]
    _check_batch_counts(counts)
    for b in range(batch):
        assert ref[b][0].tobytes() == got[b][0].tobytes() and ref[b][1].tobytes() == got[b][1].tobytes(), b


# ---- e. FAST cell shapes ----

# (width, height, levels, big-cell flag per level (k_fast_cells; the others k_fast_cells_wave), quad-tree roots are in the comments)
CELL_CASES = [
    (160, 120, 4, [True, False, True, False]),   # cell heights 44, 34, 51, 37
    (131, 97, 3, [False, True, True]),           # level 1: cells 39 x 49, level 2: a single cell 59 wide
    (400, 100, 2, [False, True]),                # 5 and 6 quad-tree roots; level 1: cells 31 x 51
]


@pytest.mark.parametrize("w,h,nlevels,big", CELL_CASES, ids=lambda v: None if isinstance(v, list) else str(v))
def test_fast_cell_shapes(oracle, w, h, nlevels, big):
    for name, img in _both(w, h):
        counts, plan, _ = run_stages(oracle, _cfg(300, 1.2, nlevels), img)
        assert plan["big_cell"] == big and plan["halves"][0]["big_cell_kernel"], (name, plan)
        assert plan["skipped_cells"] == [0] * nlevels
        assert counts[0] >= MIN_KPS, (name, counts)
        ref = oracle_ref(oracle, _cfg(300, 1.2, nlevels), img)
        assert all(len(lv["cand"]) > 0 for lv in ref["levels"]), name   # both kernels found candidates


def test_fast_skipped_cells(oracle):
    """813 x 96: 26 columns of 31-pixel cells over a 781-pixel region, the last column starts 6 pixels before the region's end and is skipped
    (reference src/ORBextractor.cc:799: iniX >= maxBorderX - 6).  A column is skipped when nCols * wCell - region_w >= wCell - 6, which needs
    more than 24 columns: 813 is the smallest such width; a skipped row would need more than 27 rows."""
    for name, img in _both(813, 96):
        counts, plan, _ = run_stages(oracle, _cfg(300, 1.2, 1), img)
        assert plan["skipped_cells"] == [2] and plan["big_cell"] == [False], (name, plan)
        assert not plan["halves"][0]["big_cell_kernel"]
        assert counts[0] >= MIN_KPS, (name, counts)


# ---- f. quad-tree storage ----

def test_quadtree_spill_and_lds_in_one_call(oracle):
    """Noise at 320 x 240: level 0 has more than kCandCap = 4096 candidates (k_octree_spill takes it, k_octree leaves it), levels 1 and 2 have fewer
    (k_octree takes them, k_octree_spill leaves them)."""
    cfg = _cfg(1000, 1.2, 3)
    img = _noise(320, 240)
    counts, plan, _ = run_stages(oracle, cfg, img)
    n = [len(lv["cand"]) for lv in oracle_ref(oracle, cfg, img)["levels"]]
    assert n[0] > 4096 and 0 < n[2] < n[1] < 4096, n
    assert not plan["halves"][0]["oct_nodes_hbm"] and plan["big_cell"] == [False] * 3
    assert counts[0] >= 950, counts


def test_quadtree_node_tables_hbm_threshold(oracle):
    """One level of 256 x 256: the node tables (88 B per node, quota + 12 nodes) and the 24 KB candidate list fit the 160 KB - 512 B of LDS up to
    1562 features; 1563 is the smallest count whose tables go to HBM (k_octree_hbm).  Both sides of the threshold, same image."""
    img = _noise(256, 256)
    for nf, hbm in ((1562, False), (1563, True)):
        counts, plan, _ = run_stages(oracle, _cfg(nf, 1.2, 1), img)
        assert plan["halves"][0]["oct_nodes_hbm"] == hbm, (nf, plan)
        assert counts[0] >= 1500, (nf, counts)


# ---- g. plain blur rounding ----

def _tie_image(w, h):
    """The two roundings differ only where the 16 fraction bits of the column pass are exactly one half.  A band of 8-pixel stripes of 136 and 122 puts
    that case on two columns of every stripe edge: with the taps (18, 34, 49, 55, 49, 34, 18) / 257, 101 * 136 + 156 * 122 = 156 * 122 + 101 * 136 =
    32768, so 128.5 is stored as 128 by half-to-even and as 129 by half-up."""
    img = _structured(w, h).copy()
    img[h // 3:h // 3 + 24, :] = np.where((np.arange(w) // 8) % 2 == 0, 136, 122).astype(np.uint8)
    return img


@pytest.mark.parametrize("w,h,nlevels", [(163, 121, 4), (320, 240, 3)])
def test_plain_blur_rounding(oracle, w, h, nlevels):
    """oslam_orb_set_blur_rounding(0) against the oracle's scalar rounding, through the host entry (word path of the blur) and through a tight
    device buffer (odd width 163: byte path; 320: word path from the caller's buffer)."""
    cfg = _cfg(300, 1.2, nlevels)
    img = _tie_image(w, h)
    sse2, plain = oracle_ref(oracle, cfg, img, True), oracle_ref(oracle, cfg, img, False)
    # else the case proves nothing: hundreds of blurred pixels of level 0 and some descriptor bits depend on the rounding
    assert (sse2["levels"][0]["blurred"] != plain["levels"][0]["blurred"]).sum() >= 300
    assert sse2["kps"].tobytes() == plain["kps"].tobytes() and (sse2["desc"] != plain["desc"]).any()
    counts, plan, _ = run_stages(oracle, cfg, img, blur_sse2=False)
    assert plan["halves"][0]["src_aligned16"] and counts[0] >= MIN_KPS
    counts, plan, _ = run_stages(oracle, cfg, np.stack([img, _noise(w, h)]), layout=Layout(0, w, w * h), blur_sse2=False)
    assert plan["halves"][0]["src_aligned4"] == (w % 4 == 0), plan
    assert min(counts) >= MIN_KPS, counts


# ---- h. refusals ----

@pytest.mark.parametrize("w,h,nlevels,why", [
    (100, 100, 4, "FAST cell grid"),    # level 3 is 58 x 58
    (100, 300, 1, "0 quad-tree roots"),   # round(68 / 268)
    (2000, 62, 1, "66 quad-tree roots"),  # round(1968 / 30)
])
def test_create_refuses_geometry(w, h, nlevels, why):
    with pytest.raises(OslamError) as ei:
        ORBextractor(300, 1.2, nlevels, 20, 7, w, h)
    assert ei.value.code == OSLAM_E_INVALID and why in str(ei.value), ei.value


def test_batch_entry_refuses_bad_arguments():
    import torch
    ex = ORBextractor(300, 1.2, 4, 20, 7, 160, 120, max_batch=2)
    buf = torch.zeros(3 * 160 * 128, dtype=torch.uint8, device="cuda")
    try:
        for batch, stride, image_stride in ((1, 159, 160 * 120), (0, 160, 160 * 120), (3, 160, 160 * 120), (2, 160, 160 * 120 - 1)):
            with pytest.raises(OslamError) as ei:
                ex.extract_batch_device(buf.data_ptr(), batch, stride, image_stride, torch.cuda.current_stream().cuda_stream)
            assert ei.value.code == OSLAM_E_INVALID, ei.value
            plan = ex.debug_plan()
            assert plan["halves"] == [] and plan["batch"] == 0, plan   # nothing was launched
        ex.extract_batch_device(buf.data_ptr(), 2, 160, 160 * 120, torch.cuda.current_stream().cuda_stream)
        assert len(ex.fetch(1)[0]) == 0 and ex.debug_plan()["halves"][0]["nb"] == 2
    finally:
        ex.close()
