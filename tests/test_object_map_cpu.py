"""CPU: the numpy restatement of the object map maintenance (tests/object_map_common.py) against answers worked out by hand from the formulas of
include/oslam_hip.h, "Object map maintenance"; the generators; the header, the library's exports and the ctypes mirrors.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import object_map_common as omc
from object_slam_amd import object_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
HAND, MERGE = omc.hand_cases(), omc.merge_hand_cases()


@pytest.fixture(scope="module")
def answers():
    return {k: omc.reject_outliers(c["pos"], c["cnt"], c["total"], c["mode"]) for k, c in HAND.items()}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name, answers):
    c, r = HAND[name], answers[name]
    assert np.array_equal(r["keep"], c["keep"]), (r["keep"].tolist(), c["keep"].tolist())
    assert r["n_kept"] == int(c["keep"].sum())
    for k, v in c["expect"].items():
        if k == "negative_variance":
            assert r["variance"] < 0 and np.isnan(r["std_dev"])
        elif k == "outliers":
            d = omc.norm3(c["pos"] - r["candidates_center"][None, :]).astype(f32)
            assert r["std_dev"] > 0 and np.nonzero(d > f32(3) * r["std_dev"])[0].tolist() == list(v)
        elif k == "cluster":
            assert r["cluster"].tolist() == list(v)
        else:
            assert r[k] == v, (k, r[k], v)


def test_hand_cases_cover_the_paths_and_the_sizes_the_kernel_branches_on():
    assert len(HAND) >= 22
    assert {c["expect"].get("path", -1) for c in HAND.values()} >= {omc.PATH_TEST5, omc.PATH_TEST7, omc.PATH_SHORTCUT}
    assert {len(c["pos"]) for c in HAND.values()} >= {0, 1, 2, 70, 300, 3000, 3001}


def test_the_threshold_floats_are_what_the_cases_say():
    assert f32(0.1) * f32(0.1) > omc.TOL2 and f32(0.0999) * f32(0.0999) < omc.TOL2
    assert not np.float64(f32(2.0 / 20.0)) < 0.1 and np.float64(f32(2.0 / 21.0)) < 0.1
    assert omc.label_bad([1, 2, 0, 3], [2, 4, 0, 7]).tolist() == [False, False, True, True]   # 0.5 is not < 0.5; an empty map is probability 0


def test_components_of_a_shuffled_line_and_of_its_halves():
    p = omc._line(40)
    perm = np.random.default_rng(0).permutation(40)
    assert (omc.components(p[perm]) == 0).all()
    q = np.delete(p, 20, axis=0)   # the line cut in two
    comp = omc.components(q)
    assert sorted(set(comp.tolist())) == [0, 20] and (comp[:20] == 0).all() and (comp[20:] == 20).all()


def test_center_and_size_by_hand():
    center, bbox = omc.center_and_size([[1, 2, 3], [3, 2, -1], [2, 5, 1]])
    assert center.tolist() == [2.0, 3.0, 1.0] and bbox.tolist() == [3.0, 5.0, 3.0, 1.0, 2.0, -1.0]
    assert omc.center_and_size(np.zeros((0, 3))) == (None, None)
    center, bbox = omc.center_and_size([[np.nan, 0, 0], [1, 0, 0]])
    assert np.isnan(center[0]) and bbox[0] == 1.0 and bbox[3] == 1.0
    # the sum runs in list order in float32: 1e8 + 1 + 1 ... loses every 1, the reverse order does not
    big = np.array([[1e8, 0, 0]] + [[1, 0, 0]] * 8, f32)
    assert omc.center_and_size(big)[0][0] == f32(1e8) / f32(9) and omc.center_and_size(big[::-1])[0][0] == f32(1e8 + 8) / f32(9)


@pytest.mark.parametrize("name", sorted(MERGE))
def test_merge_hand_case(name):
    c = MERGE[name]
    ratio, sets = omc.merge_sets(c["label"], c["track_id"], c["bbox"])
    assert sets == c["sets"], sets


def test_overlap_ratio_by_hand():
    box = omc._unit_box
    assert omc.overlap_ratio(box(0.0), box(0.5)) == f32(0.5) and omc.overlap_ratio(box(0.0), box(1.0)) == 0 and omc.overlap_ratio(box(0.0), box(0.0)) == 1
    assert omc.overlap_ratio(box(0.0), box(0.25, sx=0.5)) == 1.0     # the smaller box lies inside: the larger of the two quotients
    assert omc.overlap_ratio(box(0.0), [1.5, 1.0, 0.5, 0.5, 0.0, 0.5]) == 0


def test_generated_problems_reach_every_rule():
    """the generators give all three paths' decisions: small clusters dropped, 3-sigma outliers dropped, negative variances, bad rows, several clusters"""
    seen = dict(small=0, sigma=0, negvar=0, bad=0, multi=0, shortcut=0, empty=0)
    for mode in (omc.MODE_UPDATE, omc.MODE_NEW_OBJECT):
        for p in omc.generated(mode, count=60):
            r = omc.reject_outliers(p["pos"], p["cnt"], p["total"], mode)
            seen["negvar"] += r["variance"] < 0
            seen["bad"] += r["n_candidates"] < len(p["pos"])
            seen["multi"] += r["n_clusters"] > 1
            seen["shortcut"] += r["path"] == omc.PATH_SHORTCUT
            seen["empty"] += len(p["pos"]) == 0
            cand = r["n_candidates"]
            if r["path"] == omc.PATH_TEST7 and cand > 15:
                cl = r["cluster"][r["cluster"] >= 0]
                roots, sizes = np.unique(cl, return_counts=True)
                small = roots[sizes < 0.1 * cand - 1e-3]
                seen["small"] += len(small) > 0
                big_dropped = [(r["keep"][k] == 0 and r["cluster"][k] >= 0 and r["cluster"][k] not in small) for k in range(len(p["pos"]))]
                seen["sigma"] += any(big_dropped)
    assert all(v > 0 for v in seen.values()), seen
    maps = omc.generated_maps(count=60)
    n_sets = [len(omc.merge_sets(*m)[1]) for m in maps]
    assert max(n_sets) >= 2 and min(n_sets) == 0


def test_header_declares_and_library_exports_the_entry_points():
    from object_slam_amd import build
    from object_slam_amd._lib import lib
    build.build_hip()
    header = open(os.path.join(ROOT, "include", "oslam_hip.h")).read()
    declared = set(re.findall(r"\b(oslam_objmap_\w+)\s*\(", header))
    want = {"oslam_objmap_create", "oslam_objmap_destroy", "oslam_objmap_reject_outliers", "oslam_objmap_reject_outliers_device", "oslam_objmap_center_and_size",
            "oslam_objmap_center_and_size_device", "oslam_objmap_merge_sets", "oslam_objmap_merge_sets_device", "oslam_objmap_set_timing", "oslam_objmap_last_kernel_ms"}
    assert want <= declared, want - declared
    L = lib()
    for name in sorted(declared):
        assert hasattr(L, name), name
    assert "object_map.hip" in build.SOURCES
    import object_slam_amd
    assert object_slam_amd.ObjectMap is object_map.ObjectMap and object_slam_amd.object_map is object_map


def test_struct_mirrors_have_the_sizes_of_the_header(tmp_path):
    pairs = [("oslam_objmap_problem_t", object_map.PROBLEM_DTYPE.itemsize), ("oslam_objmap_result_t", object_map.RESULT_DTYPE.itemsize),
             ("oslam_objmap_merge_problem_t", object_map.MERGE_DTYPE.itemsize)]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "oslam_hip.h"\nint main(void) {\n' + "".join('    printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n, _ in pairs)
                   + '    printf("bbox %zu\\n", offsetof(oslam_objmap_result_t, bbox));\n    return 0;\n}\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    for name, size in pairs:
        assert int(got[name]) == size, name
    assert int(got["bbox"]) == object_map.RESULT_BBOX_OFFSET
    assert (object_map.MODE_UPDATE, object_map.MODE_NEW_OBJECT, object_map.PATH_TEST5, object_map.PATH_TEST7, object_map.PATH_SHORTCUT) == \
        (omc.MODE_UPDATE, omc.MODE_NEW_OBJECT, omc.PATH_TEST5, omc.PATH_TEST7, omc.PATH_SHORTCUT)


def test_no_device_is_an_error():
    import torch
    if torch.cuda.is_available():
        return   # (the GPU suite creates handles)
    from object_slam_amd._lib import OSLAM_E_HIP, OslamError
    with pytest.raises(OslamError) as ei:
        object_map.ObjectMap(1)
    assert ei.value.code == OSLAM_E_HIP


def test_adapter_and_caller_program_compile():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adapter_object_map_program.cc")])


def test_fixture_of_the_caller_program():
    """two objects out of the new-object path (one through the rules, one through the shortcut), a third later; updates drop a bad point and far points; the two
    overlapping objects of one label merge into the one of larger track id, whose merged list is cleaned again"""
    points, frames = omc.fixture_scene()
    lines = omc.run_fixture(points, frames)
    assert lines[:4] == ["frame 0: 0:40 1:30", "frame 1: 0:64 1:30 2:55", "frame 2: 0:64 1:30 2:59", "erased 1 left 2"]
    assert lines[4].startswith("object 0 label 1 updates 2 valid 1 replaced 2 obs 3 n 64 ") and lines[5].startswith("object 1 label 2 updates 0 valid 1 replaced -1 obs 1 n 30 ")
    assert lines[6].startswith("object 2 label 1 updates 2 valid 1 replaced -1 obs 5 n 123 ")
