"""CPU: the numpy restatement of the object association (tests/object_match_common.py) against answers worked out by hand from the formulas of include/oslam_hip.h,
"Object association"; the generators; the header, the library's exports and the ctypes mirrors.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import object_match_common as omc
from object_slam_amd import object_match

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
TWO, MAP = omc.hand_cases_two_frame(), omc.hand_cases_map()


def _hsv(b, g, r):
    return tuple(int(x) for x in omc.bgr2hsv(b, g, r))


def test_hsv_of_the_primaries():
    # sdiv[255] = 4096 and hdiv[255] = round(737280 / 1530) = 482: s = (255 * 4096 + 2048) >> 12 = 255; blue: h = (1020 * 482 + 2048) >> 12 = 120; green: (510 * 482 + 2048) >> 12 = 60
    assert _hsv(255, 0, 0) == (120, 255, 255)
    assert _hsv(0, 255, 0) == (60, 255, 255)
    assert _hsv(0, 0, 255) == (0, 255, 255)


def test_hsv_of_a_grey_and_of_a_negative_hue():
    assert _hsv(128, 128, 128) == (0, 0, 128)
    # magenta: v == r, h = g - b = -255; (-255 * 482 + 2048) >> 12 = floor(-29.5) = -30; + 180
    assert _hsv(255, 0, 255) == (150, 255, 255)
    # b = 10, g = 0, r = 200: diff = 200, hdiv[200] = round(737280 / 1200) = 614; (-10 * 614 + 2048) >> 12 = floor(-0.999) = -1 -> 179; s = (200 * sdiv[200] + 2048) >> 12 with
    # sdiv[200] = round(5222.4) = 5222: 1046448 >> 12 = 255
    assert _hsv(10, 0, 200) == (179, 255, 200)


def test_hsv_of_the_256_greys():
    g = np.arange(256)
    h, s, v = omc.bgr2hsv(g, g, g)
    assert (h == 0).all() and (s == 0).all() and np.array_equal(v, g)


def test_hue_stays_below_180_over_the_whole_cube():
    g = np.arange(0, 256, 5)
    b, gg, r = np.meshgrid(g, g, g, indexing="ij")
    h, s, v = omc.bgr2hsv(b, gg, r)
    assert h.min() >= 0 and h.max() <= 179 and s.max() <= 255 and np.array_equal(v, np.maximum(b, np.maximum(gg, r)))


def test_histogram_bin_edges_and_column_order():
    _, _, cols = omc.hsv_tables()
    assert (cols["h"][5], cols["h"][6], cols["h"][179]) == (64 + 0, 64 + 1, 64 + 29) and (cols["h"][180:] == -1).all()
    assert (cols["s"][7], cols["s"][8], cols["s"][255]) == (32 + 0, 32 + 1, 32 + 31)
    assert (cols["v"][7], cols["v"][8], cols["v"][255]) == (0, 1, 31)
    # one pixel of pure blue, (H, S, V) = (120, 255, 255): V bin 31 in column 31, S bin 31 in column 63, H bin 20 in column 84
    img = np.array([[[255, 0, 0]]], np.uint8)
    counts, hist = omc.hsv_histograms(img, np.array([[[9]]], np.uint8))
    assert np.flatnonzero(counts[0]).tolist() == [31, 63, 84] and counts[0].sum() == 3
    assert hist[0, 31] == f32(1.0) * f32(1.0 / 3.0)


def test_hist_sums_to_one_and_an_empty_mask_gives_zeros():
    rng = np.random.default_rng(1)
    _, px = omc.gen_image(rng, 37, 23)
    masks = omc.gen_masks(rng, 4, 37, 23, values=(0, 1, 7, 255))
    masks[3] = 0
    counts, hist = omc.hsv_histograms(px, masks)
    for k in range(3):
        n = int((masks[k] != 0).sum())
        assert n > 0 and counts[k].sum() == 3 * n and counts[k, :32].sum() == n and counts[k, 32:64].sum() == n and counts[k, 64:].sum() == n
        assert abs(float(hist[k].astype(np.float64).sum()) - 1.0) <= 94 * float(np.finfo(f32).eps)
    assert (counts[3] == 0).all() and (hist[3] == 0).all()


def test_cosine_of_hand_histograms():
    s = omc.cosine([omc.E0, omc.E0, omc.E0, omc.E0], [omc.E0, omc.E1, omc.NEAR0, omc.HALF])[0]
    assert s[0] == 1.0 and s[1] == 0.0 and abs(float(s[2]) - 0.9 / np.sqrt(0.82)) < 1e-6 and abs(float(s[3]) - np.sqrt(0.5)) < 1e-6
    assert np.isnan(omc.cosine([np.zeros(94)], [omc.E0])[0, 0])     # a histogram of zeros: 0 / 0


def test_box_iou_of_hand_boxes():
    assert omc.box_iou(omc.BOX, omc.BOX) == 1.0 and omc.box_iou(omc.BOX, omc.BOX_FAR) == 0.0
    assert abs(float(omc.box_iou(omc.BOX, omc.BOX_SHIFT)) - 0.6) < 1e-6 and abs(float(omc.box_iou(omc.BOX, omc.BOX_HALF)) - 1.0 / 3.0) < 1e-6
    assert omc.box_iou(omc.BOX, (30.0, 10.0, 20.0, 20.0)) == 0.0        # touching edges: x1 >= x2


@pytest.mark.parametrize("name", sorted(TWO))
def test_two_frame_hand_case(name):
    c = TWO[name]
    e = c["expect"]
    cur, sim, iou, n = omc.match_two_frame(c)
    assert cur.tolist() == e["cur"] and n == e["n"]
    assert np.array_equal(np.isnan(sim), np.isnan(iou))
    if "sim_nan" in e:
        assert np.isnan(sim).tolist() == e["sim_nan"]
    if "iou" in e:
        assert np.allclose(iou, np.array(e["iou"], f32), atol=1e-6)


@pytest.mark.parametrize("name", sorted(MAP))
def test_map_hand_case(name):
    c = MAP[name]
    e = c["expect"]
    assert omc.map_precondition(c) == omc.DONE
    cur, sim, mean, mind, by_sim, by_dist = omc.match_map_to_frame(c)
    assert cur.tolist() == e["cur"] and (by_sim, by_dist) == (e["by_sim"], e["by_dist"])
    assert np.array_equal(np.isnan(sim), np.isnan(mean)) and np.array_equal(np.isnan(sim), np.isnan(mind))


def test_hand_cases_are_what_their_names_say():
    assert len(TWO) + len(MAP) >= 12
    _, sim, mean, mind, _, _ = omc.match_map_to_frame(MAP["both_rules_fire_onto_two_detections"])
    assert sim[0, 0] == 1.0 and 0.99 < sim[0, 1] < 1.0 and abs(float(mean[0, 0]) - 0.2) < 1e-6 and abs(float(mind[0, 1]) - 0.05) < 1e-6
    _, sim, _, mind, _, _ = omc.match_map_to_frame(MAP["distance_tie_smallest_index"])
    assert mind[0, 0] == mind[0, 1] and sim[0, 0] == 0.0
    _, sim, _, _, _, _ = omc.match_map_to_frame(MAP["claim_hides_detection"])
    assert not np.isnan(sim[0, 0]) and np.isnan(sim[1, 0])
    _, sim, mean, mind, _, _ = omc.match_map_to_frame(MAP["mean_too_far_min_near"])
    assert sim[0, 0] == 1.0 and mean[0, 0] > 0.3 and mind[0, 0] < 0.1
    _, sim, iou, _ = omc.match_two_frame(TWO["winner_fails_iou_runner_up_ignored"])
    assert sim[0, 0] > sim[0, 1] > 0.8 and iou[0, 0] < 0.5 < iou[0, 1]
    assert omc.map_precondition(dict(MAP["empty_map"], objs=dict(obs_center=[np.zeros((0, 3))]))) == omc.REFUSED_NO_OBSERVATION


def test_generated_problems_straddle_every_threshold():
    """the generators' own assertions (each rule fires in a fifth of the problems and stays silent in a fifth), and scores on both sides of the four thresholds"""
    ps, ans = omc.generated_two_frame()
    sims = np.concatenate([a[1].reshape(-1) for a in ans])
    ious = np.concatenate([a[2].reshape(-1) for a in ans])
    sims, ious = sims[~np.isnan(sims)], ious[~np.isnan(ious)]
    print("two-frame: %d scores, similarity > 0.8: %d, IoU > 0.5: %d, problems that assign: %d" % (len(sims), (sims > 0.8).sum(), (ious > 0.5).sum(), sum(a[3] > 0 for a in ans)))
    assert min((sims > 0.8).sum(), (sims <= 0.8).sum(), (ious > 0.5).sum(), (ious <= 0.5).sum()) >= 40
    assert {len(p["pre"]["label"]) for p in ps} == set(range(9)) and {len(p["cur"]["label"]) for p in ps} == set(range(9))
    ps, ans = omc.generated_map()
    sims, means, mins = (np.concatenate([a[k].reshape(-1) for a in ans]) for k in (1, 2, 3))
    sims, means, mins = sims[~np.isnan(sims)], means[~np.isnan(means)], mins[~np.isnan(mins)]
    print("map: %d scores, similarity > 0.8: %d, mean < 0.3: %d, min < 0.1: %d, by similarity in %d problems, by distance in %d" % (
        len(sims), (sims > 0.8).sum(), (means < 0.3).sum(), (mins < 0.1).sum(), sum(a[4] > 0 for a in ans), sum(a[5] > 0 for a in ans)))
    assert min((sims > 0.8).sum(), (sims <= 0.8).sum(), (means < 0.3).sum(), (means >= 0.3).sum(), (mins < 0.1).sum(), (mins >= 0.1).sum()) >= 40
    assert {len(p["objs"]["label"]) for p in ps} == set(range(13)) and {len(p["cur"]["label"]) for p in ps} == set(range(9))
    assert any(a[4] > 0 and a[5] > 0 for a in ans)


def test_fixture_of_the_caller_program():
    """three objects keep their ids over six frames; the one that left is recovered by MatchMapToFrame; the swap of detection order does not swap ids"""
    frames = omc.fixture_frames()
    ids, claims = omc.track_fixture(frames)
    truth = [[d["truth"] for d in F["dets"]] for F in frames]
    print(ids, claims)
    assert ids == truth and truth[2] == truth[3][::-1] and 1 not in truth[2] + truth[3] and 1 in truth[4]
    assert claims[0] == (0, 0, 0) and claims[1][0] == 3 and claims[4][0] == 2 and claims[4][1] + claims[4][2] >= 1


def test_header_declares_and_library_exports_the_entry_points():
    from object_slam_amd import build
    from object_slam_amd._lib import lib
    build.build_hip()
    header = open(os.path.join(ROOT, "include", "oslam_hip.h")).read()
    declared = set(re.findall(r"\b(oslam_objmatch_\w+)\s*\(", header))
    want = {"oslam_objmatch_create", "oslam_objmatch_destroy", "oslam_objmatch_hsv_histograms", "oslam_objmatch_hsv_histograms_device", "oslam_objmatch_match_two_frame",
            "oslam_objmatch_match_two_frame_device", "oslam_objmatch_match_map_to_frame", "oslam_objmatch_match_map_to_frame_device", "oslam_objmatch_set_timing",
            "oslam_objmatch_last_kernel_ms"}
    assert want <= declared, want - declared
    L = lib()
    for name in sorted(declared):
        assert hasattr(L, name), name
    assert "object_match.hip" in build.SOURCES


def test_struct_mirrors_have_the_sizes_of_the_header(tmp_path):
    import ctypes as C
    pairs = [("oslam_objmatch_params_t", C.sizeof(object_match.Params)), ("oslam_objmatch_det_rows_t", C.sizeof(object_match.DetRows)),
             ("oslam_objmatch_obj_rows_t", C.sizeof(object_match.ObjRows)), ("oslam_objmatch_frame_t", object_match.FRAME_DTYPE.itemsize),
             ("oslam_objmatch_pair_problem_t", object_match.PAIR_DTYPE.itemsize), ("oslam_objmatch_map_problem_t", object_match.MAP_DTYPE.itemsize)]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "oslam_hip.h"\nint main(void) {\n' + "".join('    printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n, _ in pairs)
                   + "    return 0;\n}\n")
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    for name, size in pairs:
        assert int(got[name]) == size, name
    assert object_match.BINS == omc.BINS == 94


def test_no_device_is_an_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from object_slam_amd._lib import OSLAM_E_HIP, OslamError
    with pytest.raises(OslamError) as ei:
        object_match.ObjectMatcher(1, 64, 48)
    assert ei.value.code == OSLAM_E_HIP


def test_adapter_and_caller_program_compile():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adapter_object_program.cc")])
