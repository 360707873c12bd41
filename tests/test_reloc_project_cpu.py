"""CPU: the restatement of ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) in tests/reloc_project_common.py against hand-built known
answers and against the truth of generated problems, so that the GPU tests may compare the kernel with it; what the generated parity batch exercises; the ctypes
mirrors of include/oslam_hip.h, "Relocalisation projection"."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reloc_project_common as rpc
import sim3_match_common as smc
from object_slam_amd import reloc_project   # (at import: every test of this file belongs to the operator, also those that pin the restatement it is compared with)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in rpc.hand_cases()}
f32 = np.float32


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_gives_the_known_answer(name):
    c = CASES[name]
    d = {}
    matched, n, removed = rpc.run_problem(c, d)
    e = c["expect"]
    print(name, matched.tolist(), n, removed)
    assert matched.tolist() == list(e["matched"]) and n == e["n"] and removed == e["removed"]
    if n >= 0:
        assert n == sum(1 for v in e["matched"] if v >= 0)
        # the claims of the pass structure the operator uses are the sequential ones (what the histogram removed was claimed too)
        passes, claims = rpc.replay_passes(c["frame"]["has_mp"], d["cands"])
        assert (claims >= 0).sum() == n + removed and np.array_equal(claims[matched >= 0], matched[matched >= 0]) and passes <= len(c["skip"]) + 1


def _uv(c):
    T = c["Tcw"]
    _, u, v, level = rpc._gates(c["pts"], c["skip"], T[:3, :3], T[:3, 3], rpc.camera_centre(T[:3, :3], T[:3, 3]), rpc.CAM, rpc.BOUNDS, rpc.LOG_SF, rpc.NLEVELS)
    return u, v, level


def test_hand_cases_are_what_their_comments_say():
    pop = lambda a, b: int(smc._POP[np.bitwise_xor(a, b)].sum())
    c = CASES["chain"]
    d = [[pop(c["pts"]["desc"][i], c["frame"]["desc"][k]) for k in range(5)] for i in range(5)]
    assert d[0][0] == 0 and all(d[j][j - 1] == 6 and d[j][j] == 14 and min(d[j][k] for k in range(5) if k not in (j - 1, j)) == 26 for j in range(1, 5))
    det = {}
    rpc.run_problem(c, det)
    assert rpc.replay_passes(c["frame"]["has_mp"], det["cands"])[0] >= 5
    c = CASES["big_window"]
    n = rpc.CACHE_CASE_CANDIDATES
    assert n > 7 and all(pop(c["pts"]["desc"][i], c["frame"]["desc"][k]) == k + 1 for i in range(n) for k in range(n))
    det = {}
    rpc.run_problem(c, det)
    assert all(len(cl) == n for cl in det["cands"]) and rpc.replay_passes(c["frame"]["has_mp"], det["cands"])[0] >= n
    for m in (7, 8):   # the cache boundary: every slot has exactly m candidates (7: the last count cached, 8: the first that overflows) and the replay takes m + 1 passes
        c = CASES["window_%d" % m]
        det = {}
        rpc.run_problem(c, det)
        assert len(det["cands"]) == m and all(len(cl) == m for cl in det["cands"]) and rpc.replay_passes(c["frame"]["has_mp"], det["cands"])[0] == m + 1
    c = CASES["removed_match_still_blocks"]
    assert pop(c["pts"]["desc"][1], c["frame"]["desc"][0]) == 3 and rpc.rot_bin(90.0, 0.0) == 3
    c = CASES["tie"]
    assert [pop(c["pts"]["desc"][0], c["frame"]["desc"][k]) for k in range(2)] == [10, 10]
    px, py = smc._grid_cells(c["frame"]["keysUn"], rpc.BOUNDS, f32(0.1), f32(0.1))
    assert (px.tolist(), py.tolist()) == ([11, 9], [9, 11])   # the column-first traversal reaches keypoint 1 first; row-first, or index order, would reach keypoint 0
    # the bounds: the projections are exactly on the bounds, and exactly one producible step beyond
    u, v, _ = _uv(CASES["bounds_inclusive"])
    assert (u[0], u[1], v[2], v[3]) == (0.0, 640.0, 0.0, 480.0)
    assert u[4] == -2.0 ** -15 and u[5] == np.nextafter(f32(640), f32(1000)) and v[6] == -2.0 ** -16 and v[7] == np.nextafter(f32(480), f32(1000))
    assert f32(-320.0) - f32(2.0 ** -15) == np.nextafter(f32(-320), f32(-1000)) and f32(-240.0) - f32(2.0 ** -16) == np.nextafter(f32(-240), f32(-1000))
    # depth: behind the camera and on the keypoint; infinite; NaN; NaN
    u, v, _ = _uv(CASES["depth"])
    assert (u[0], v[0]) == (100.0, 100.0) and CASES["depth"]["pts"]["Xw"][0, 2] == -2.0 and np.isinf(u[1]) and np.isnan(u[2]) and np.isnan(v[2]) and np.isnan(u[3])
    for level in (0, 3, 7):
        assert (_uv(CASES["level_%d" % level])[2] == level).all()
    c = CASES["distance"]
    assert c["pts"]["Xw"][0, 2] == f32(1.2) * f32(3.0) and c["pts"]["Xw"][2, 2] == f32(0.8) * f32(5.0) == f32(4.0)
    for od in (100, 64):
        c = CASES["orbdist_%d" % od]
        assert [pop(c["pts"]["desc"][k], c["frame"]["desc"][k]) for k in range(2)] == [od, od + 1] and c["orb_dist"] == od and c["th"] == (10.0 if od == 100 else 3.0)
    c = CASES["window_edge"]
    K = c["frame"]["keysUn"]
    assert K["x"][0] - f32(100) == 10.0 and 0 < f32(10) - (K["x"][1] - f32(300)) < 1e-4 and K["y"][2] - f32(300) == 10.0 and 0 < f32(10) - (f32(300) - K["y"][3]) < 1e-4
    # the histogram: the bins the comments name
    factor = f32(1.0) / f32(30)
    assert f32(15.0) * factor == f32(0.5) and rpc.rot_bin(15.0, 0.0) == 1 and rpc.rot_bin(10.0, 350.0) == 1 and rpc.rot_bin(0.0, 0.0) == 0
    assert (rpc.rot_bin(165.0, 0.0), rpc.rot_bin(285.0, 0.0)) == (6, 10) and rpc.rot_bin(np.nan, 0.0) is None and rpc.rot_bin(360.0, 0.0) == 12
    assert f32(0.1) * f32(10.0) == f32(1.0) and f32(1.0) < f32(0.1) * f32(11.0)
    assert rpc.three_maxima([0, 0, 2, 0, 2, 0, 2, 0, 2] + [0] * 21) == (2, 4, 6)
    assert rpc.three_maxima([11, 0, 0, 1, 0, 0, 1] + [0] * 23) == (0, -1, -1) and rpc.three_maxima([11, 0, 0, 2, 0, 0, 1] + [0] * 23) == (0, 3, -1)
    assert rpc.three_maxima([0] * 30) == (-1, -1, -1)


def test_generator():
    p = rpc.make_problem(7, 300, 333, rpc.FINE)
    assert len(p["frame"]["has_mp"]) == 300 and len(p["skip"]) == 333 == len(p["truth"]) and 333 % 64 != 0
    assert all(p["frame"][k].dtype == rpc.empty_frame()[k].dtype for k in rpc.FRAME_KEYS) and all(p["pts"][k].dtype == rpc.empty_pts()[k].dtype for k in rpc.PT_KEYS)
    want = np.nonzero(p["truth"] >= 0)[0]
    assert len(want) >= 100 and not p["skip"][want].any() and not p["frame"]["has_mp"][p["truth"][want]].any()
    assert p["frame"]["has_mp"].sum() >= 10 and p["skip"].sum() >= 10 and (p["truth"] == rpc.DONT_CARE).sum() >= 5
    # a findable slot projects, through the searched pose, within the window of its keypoint and is 14 bits at most from it; some lie behind the camera
    T = p["Tcw"]
    Pc = p["pts"]["Xw"][want].astype(np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3]
    uv = smc._project(Pc)
    k = p["truth"][want]
    assert np.maximum(np.abs(uv[:, 0] - p["frame"]["keysUn"]["x"][k]), np.abs(uv[:, 1] - p["frame"]["keysUn"]["y"][k])).max() < 3.0
    assert smc._POP[np.bitwise_xor(p["pts"]["desc"][want], p["frame"]["desc"][k])].sum(1).max() <= 14 and (Pc[:, 2] < 0).sum() >= 4
    assert len(set(k.tolist())) == len(k)
    q = rpc.make_problem(7, 300, 333, rpc.FINE)
    assert all(np.array_equal(p["pts"][key], q["pts"][key]) for key in rpc.PT_KEYS) and np.array_equal(p["truth"], q["truth"])


def test_restatement_recovers_the_truth_and_the_parity_batch_exercises_the_kernel():
    """In every generated problem of the GPU parity batch the restatement sends at least 90 % of the findable slots to their keypoint and at most 2 anywhere they
    must not go (a random descriptor is within 100 bits of another with probability 3e-4 per candidate); and the restatement alone shows that the batch needs
    three passes, loses matches to the histogram, matches through level + 1 and matches slots behind the camera, so that the GPU parity test cannot pass vacuously."""
    problems = rpc.batch_problems()[:rpc.N_GENERATED]
    modes = set()
    for p, (r, det) in zip(problems, rpc.reference_of(problems, "generated")):
        want, got, false = rpc.truth_score(p, r)
        passes, claims = rpc.replay_passes(p["frame"]["has_mp"], det["cands"])
        print("%s: %d of %d findable slots, %d others, count %d, removed %d, passes %d, through level + 1: %d" % (p["name"], got, want, false, r[1], r[2], passes, len(det["plus1"])))
        assert want >= 100 and got * 10 >= want * 9 and false <= 2
        assert r[1] >= 20 and passes >= 3 and r[2] > 0 and len(det["plus1"]) > 0
        assert len(p["skip"]) % 64 != 0 and len(p["skip"]) % 1024 != 0
        assert (claims >= 0).sum() == r[1] + r[2] and np.array_equal(claims[r[0] >= 0], r[0][r[0] >= 0])
        T = p["Tcw"]
        z = p["pts"]["Xw"].astype(np.float64) @ T[2, :3].astype(np.float64) + T[2, 3]
        assert (z[r[0][r[0] >= 0]] < 0).sum() >= 4   # matched behind the camera
        modes.add((float(p["th"]), p["orb_dist"]))
    assert modes == {rpc.COARSE, rpc.FINE}
    assert len(problems[-1]["frame"]["has_mp"]) == reloc_project.MAX_KEYPOINTS == 2400
    names = [p["name"] for p in rpc.batch_problems()]
    assert {"n_pts_zero", "n_kp_zero", "both_zero"} <= set(names) and len(set(names)) == len(names)


@pytest.mark.parametrize("name", sorted(rpc.SCENARIOS))
def test_scenarios_of_the_caller_program(name):
    """with the true pose in place of the optimised ones, the searches of src/Tracking.cc:1717 and :1731 find what the scenario was built for"""
    (n_good, n_wrong, n_coarse, n_offset), _, _ = rpc.SCENARIOS[name]
    s = rpc.make_scenario(17, n_good, n_wrong, n_coarse, n_offset)
    g = s["groups"]
    n_kp = len(s["mp"])
    held = np.full(n_kp, -1, np.int64)
    held[g["good"]] = g["good"]                                   # PoseOptimization dropped the wrong ones
    sFound = set(s["mp"][s["mp"] >= 0].tolist())
    assert len(sFound) == n_good + n_wrong
    skip = s["bad"].copy()
    skip[list(sFound)] = 1
    m, n, removed = rpc.search_by_projection(dict(s["frame"], has_mp=(held >= 0).astype(np.uint8)), s["pts"], skip, s["Ttrue"], *rpc.COARSE)
    assert n == n_coarse + n_offset and removed == 0 and set(m[m >= 0].tolist()) == set(g["coarse"].tolist()) | set(g["offset"].tolist())
    held = np.where(m >= 0, m, held)
    skip = s["bad"].copy()
    skip[held[held >= 0]] = 1
    m, n, removed = rpc.search_by_projection(dict(s["frame"], has_mp=(held >= 0).astype(np.uint8)), s["pts"], skip, s["Ttrue"], *rpc.FINE)
    assert n == n_wrong and removed == 0 and np.array_equal(np.nonzero(m >= 0)[0], g["wrong"]) and np.array_equal(m[g["wrong"]], g["wrong"])


def test_struct_mirrors_have_the_sizes_of_the_header(tmp_path):
    pairs = [("oslam_reloc_proj_problem_t", reloc_project.Problem), ("oslam_reloc_proj_frame_rows_t", reloc_project.FrameRows), ("oslam_reloc_proj_pt_rows_t", reloc_project.PtRows)]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "oslam_hip.h"\nint main(void) {\n' + "".join('    printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n, _ in pairs)
                   + '    printf("ORBdist_at %zu\\nkf_angle_at %zu\\n", offsetof(oslam_reloc_proj_problem_t, ORBdist), offsetof(oslam_reloc_proj_pt_rows_t, kf_angle));\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    c_vals = dict((l.split()[0], int(l.split()[1])) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, cls in pairs:
        assert C.sizeof(cls) == c_vals[name], (name, C.sizeof(cls), c_vals[name])
    assert reloc_project.PROBLEM_DTYPE.itemsize == c_vals["oslam_reloc_proj_problem_t"] == 96
    assert reloc_project.Problem.ORBdist.offset == c_vals["ORBdist_at"] == reloc_project.PROBLEM_DTYPE.fields["ORBdist"][1] == 92
    assert reloc_project.PtRows.kf_angle.offset == c_vals["kf_angle_at"]
    pr = reloc_project.pack_problems([3, 0, 5], [0, 3, 3], [7, 2, 0], [0, 7, 9], np.tile(np.eye(4), (3, 1, 1)), [10.0, 3.0, 3.0], [100, 64, 64])
    assert pr["kp_out_off"].tolist() == [0, 3, 3] and pr["pt_out_off"].tolist() == [0, 7, 9] and pr["th"].tolist() == [10.0, 3.0, 3.0] and pr["ORBdist"].tolist() == [100, 64, 64]
    one = reloc_project.Problem.from_buffer_copy(pr[2].tobytes())
    assert (one.n_kp, one.kp_off, one.n_pts, one.pt_off, one.kp_out_off, one.pt_out_off, one.th, one.ORBdist, one.Tcw[15], one.Tcw[1]) == (5, 3, 0, 9, 3, 9, 3.0, 64, 1.0, 0.0)
    assert (reloc_project.COARSE, reloc_project.FINE) == (rpc.COARSE, rpc.FINE) == ((10.0, 100), (3.0, 64))


def test_library_exports_the_symbols():
    from object_slam_amd import build
    from object_slam_amd._lib import lib
    build.build_hip()
    L = lib()
    for name in ("oslam_reloc_proj_create", "oslam_reloc_proj_destroy", "oslam_match_search_by_projection_reloc_batch", "oslam_match_search_by_projection_reloc_batch_device"):
        assert hasattr(L, name), name


def test_no_device_is_an_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from object_slam_amd._lib import OSLAM_E_HIP, OslamError
    with pytest.raises(OslamError) as ei:
        reloc_project.RelocProjector(4, 400, 1000)
    assert ei.value.code == OSLAM_E_HIP and "no CPU fallback" in str(ei.value)
