"""CPU: the restatement of ORBmatcher::SearchByProjection(pKF, Scw, ...) and ORBmatcher::Fuse(pKF, Scw, ...) in tests/sim3_project_common.py against hand-built
known answers and against the truth of generated problems, so that the GPU tests may compare the kernel with it; the ctypes mirrors of include/oslam_hip.h,
"Sim3 projection"."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sim3_match_common as smc
import sim3_project_common as spc
from object_slam_amd import sim3_project   # (at import: every test of this file belongs to the operator, also those that pin the restatement it is compared with)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in spc.hand_cases()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_gives_the_known_answer(name):
    c = CASES[name]
    r = spc.run_problem(c)
    e = c["expect"]
    print(name, [x.tolist() if hasattr(x, "tolist") else x for x in r])
    if c["mode"] == "search":
        assert r[0].tolist() == list(e["matched"]) and r[1] == e["n"] == sum(1 for v in e["matched"] if v >= 0)
    else:
        assert r[0].tolist() == list(e["fused_kp"]) and r[1].tolist() == list(e["replace"]) and r[2] == e["n"] == sum(1 for v in e["fused_kp"] if v >= 0)


def test_hand_cases_are_what_their_comments_say():
    pop = lambda a, b: int(smc._POP[np.bitwise_xor(a, b)].sum())
    c = CASES["chain"]
    d = [[pop(c["pts"]["desc"][i], c["kf"]["desc"][k]) for k in range(4)] for i in range(4)]
    assert d[0][0] == 0 and all(d[j][j - 1] == 6 and d[j][j] == 14 and min(d[j][k] for k in range(4) if k not in (j - 1, j)) > 14 for j in range(1, 4))
    c = CASES["chain_fallback_51"]
    assert [pop(c["pts"]["desc"][1], c["kf"]["desc"][k]) for k in range(2)] == [6, 51]
    for name, cells in (("tie", ([11, 9], [9, 11])), ("tie_fuse", ([11, 10], [10, 11]))):
        c = CASES[name]
        assert [pop(c["pts"]["desc"][0], c["kf"]["desc"][k]) for k in range(2)] == [10, 10]
        px, py = smc._grid_cells(c["kf"]["keysUn"], spc.BOUNDS, np.float32(0.1), np.float32(0.1))
        assert (px.tolist(), py.tolist()) == cells   # the column-first traversal reaches keypoint 1 first; row-first, or index order, would reach keypoint 0
    c = CASES["big_window"]
    n = spc.CACHE_CASE_CANDIDATES
    assert n > 7 and all(pop(c["pts"]["desc"][i], c["kf"]["desc"][k]) == k + 1 for i in range(n) for k in range(n))
    for m in (7, 8):   # the cache boundary: n keypoints against n points, every one a candidate (within TH_LOW, octave 6 or 7) of every point
        c = CASES["window_%d" % m]
        assert len(c["kf"]["state"]) == len(c["skip"]) == m and not c["kf"]["state"].any() and set(c["kf"]["keysUn"]["octave"].tolist()) == {6, 7}
        assert max(np.abs(c["kf"]["keysUn"]["x"] - 300).max(), np.abs(c["kf"]["keysUn"]["y"] - 300).max()) < 35.0   # inside the window of radius 35.8
        assert all(pop(c["pts"]["desc"][i], c["kf"]["desc"][k]) == k + 1 <= 50 for i in range(m) for k in range(m))
    assert np.float32(10.0) * spc.SF[7] > 35.0 and len(set(zip(*[v.tolist() for v in smc._grid_cells(c["kf"]["keysUn"], spc.BOUNDS, np.float32(0.1), np.float32(0.1))]))) > 4
    c = CASES["distance"]
    assert c["pts"]["Xw"][0, 2] == np.float32(1.2) * np.float32(3.0) and c["pts"]["Xw"][2, 2] == np.float32(0.8) * np.float32(5.0) == np.float32(4.0)
    c = CASES["angle"]
    assert float(c["pts"]["normal"][0, 2]) * 2.0 == 1.0 and float(c["pts"]["normal"][1, 2]) * 2.0 < 1.0


def test_decompose():
    t = np.array([0.25, -0.5, 1.0], np.float32)
    for s in (1.0, 0.5, 2.0):
        scw, Rcw, tcw, Ow = spc.decompose(spc.scaled_pose(s, t=t))
        assert scw == np.float32(s) and np.array_equal(Rcw, np.eye(3, dtype=np.float32)) and np.array_equal(tcw, t) and np.array_equal(Ow, -t)
        assert all(a.dtype == np.float32 for a in (Rcw, tcw, Ow)) and isinstance(scw, np.float32)
    R = smc.rodrigues(np.array([0.1, -0.2, 0.3])).astype(np.float32)
    S = spc.scaled_pose(1.3, R, t)
    scw, Rcw, tcw, Ow = spc.decompose(S)
    s0 = S[0, :3].astype(np.float64)
    assert scw == np.float32(np.sqrt((s0[0] * s0[0] + s0[1] * s0[1]) + s0[2] * s0[2])) and abs(float(scw) - 1.3) < 1e-6
    assert np.array_equal(Rcw, (S[:3, :3].astype(np.float64) * (1.0 / np.float64(scw))).astype(np.float32)) and np.abs(Rcw - R).max() < 1e-6
    assert np.abs(Rcw.astype(np.float64) @ Ow + tcw).max() < 1e-6   # the camera centre maps to the origin


def test_generator():
    for mode in ("search", "fuse"):
        p = spc.make_problem(7, 300, 517, 1.1, mode)
        assert len(p["kf"]["state"]) == 300 and len(p["skip"]) == 517 == len(p["truth"]) and 517 % 64 != 0
        assert all(p["kf"][k].dtype == spc.empty_kf()[k].dtype for k in spc.KF_KEYS) and all(p["pts"][k].dtype == spc.empty_pts()[k].dtype for k in spc.PT_KEYS)
        want = np.nonzero(p["truth"] >= 0)[0]
        assert len(want) >= 100 and not p["skip"][want].any()
        # a findable point projects, through Scw, within the noise of its keypoint, is 12 bits at most from it, in range and front-facing
        scw, Rcw, tcw, Ow = spc.decompose(p["Scw"])
        assert abs(float(scw) - 1.1) < 1e-6
        Pc = p["pts"]["Xw"][want].astype(np.float64) @ Rcw.astype(np.float64).T + tcw
        uv = smc._project(Pc)
        k = p["truth"][want]
        assert (Pc[:, 2] > 0).all() and np.hypot(uv[:, 0] - p["kf"]["keysUn"]["x"][k], uv[:, 1] - p["kf"]["keysUn"]["y"][k]).max() < 6.0
        assert smc._POP[np.bitwise_xor(p["pts"]["desc"][want], p["kf"]["desc"][k])].sum(1).max() <= 4 + 3
        # the gated kinds are there: behind, out of range, back-facing, each at least a tenth of the list
        ok, _, _, _ = spc._gates(p["pts"], np.zeros(517, np.uint8), Rcw, tcw, Ow, spc.CAM, spc.BOUNDS, spc.LOG_SF, spc.NLEVELS)
        Pall = p["pts"]["Xw"].astype(np.float64) @ Rcw.astype(np.float64).T + tcw
        PO = p["pts"]["Xw"].astype(np.float64) - Ow
        assert (Pall[:, 2] < 0).mean() > 0.1 and ((PO * p["pts"]["normal"]).sum(1) < 0).mean() > 0.1
        assert (np.linalg.norm(PO, axis=1) > 1.2 * p["pts"]["maxDistance"]).mean() > 0.1 and 0.3 < ok.mean() < 0.7
        if mode == "fuse":
            assert set(np.unique(p["kf"]["state"][k])) == {0, 1, 2} and len(set(k.tolist())) < len(k)   # duplicates go to the same keypoint
        else:
            assert len(set(k.tolist())) == len(k) and (p["kf"]["state"] == 1).sum() == int(0.45 * 300) // 10 and p["skip"].sum() > (p["kf"]["state"] == 1).sum()
        q = spc.make_problem(7, 300, 517, 1.1, mode)
        assert all(np.array_equal(p["pts"][key], q["pts"][key]) for key in spc.PT_KEYS) and np.array_equal(p["truth"], q["truth"])


def test_restatement_recovers_the_truth_of_generated_problems():
    """at least 90 % of the findable points, none of the others, and a count equal to the number found, in every problem of the GPU parity batch; every search
    problem has at least 100 findable points"""
    problems = spc.parity_problems() + spc.full_problems()
    for p, r in zip(problems, spc.reference_of(problems, "parity_and_full")):
        want, got, false = spc.truth_score(p, r)
        print("%s: %d of %d findable points, %d others, count %d" % (p["name"], got, want, false, spc.count_of(r)))
        assert want >= 100 and got * 10 >= want * 9 and false == 0 and spc.count_of(r) == got
        assert len(p["skip"]) % 64 != 0 and len(p["skip"]) % 1024 != 0


def test_struct_mirrors_have_the_sizes_of_the_header(tmp_path):
    pairs = [("oslam_sim3_proj_problem_t", sim3_project.Problem), ("oslam_sim3_proj_kf_rows_t", sim3_project.KfRows), ("oslam_sim3_proj_pt_rows_t", sim3_project.PtRows)]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "oslam_hip.h"\nint main(void) {\n' + "".join('    printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n, _ in pairs)
                   + '    printf("OSLAM_FUSE_OCCUPANT %d\\nOSLAM_FUSE_ADDED %d\\n", OSLAM_FUSE_OCCUPANT, OSLAM_FUSE_ADDED);\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    c_vals = dict((l.split()[0], int(l.split()[1])) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, cls in pairs:
        assert C.sizeof(cls) == c_vals[name], (name, C.sizeof(cls), c_vals[name])
    assert sim3_project.PROBLEM_DTYPE.itemsize == c_vals["oslam_sim3_proj_problem_t"] == 92
    assert (sim3_project.FUSE_OCCUPANT, sim3_project.FUSE_ADDED) == (c_vals["OSLAM_FUSE_OCCUPANT"], c_vals["OSLAM_FUSE_ADDED"]) == (spc.FUSE_OCCUPANT, spc.FUSE_ADDED) == (-2, -3)
    pr = sim3_project.pack_problems([3, 0, 5], [0, 3, 3], [7, 2, 0], [0, 0, 7], np.tile(np.eye(4), (3, 1, 1)), [10.0, 4.0, 4.0])
    assert pr["kp_out_off"].tolist() == [0, 3, 3] and pr["pt_out_off"].tolist() == [0, 7, 9] and pr["th"].tolist() == [10.0, 4.0, 4.0]
    one = sim3_project.Problem.from_buffer_copy(pr[2].tobytes())
    assert (one.n_kp, one.kp_off, one.n_pts, one.pt_off, one.kp_out_off, one.pt_out_off, one.th, one.Scw[15], one.Scw[1]) == (5, 3, 0, 7, 3, 9, 4.0, 1.0, 0.0)


def test_no_device_is_an_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from object_slam_amd._lib import OSLAM_E_HIP, OslamError
    with pytest.raises(OslamError) as ei:
        sim3_project.Sim3Projector(4, 400, 1000)
    assert ei.value.code == OSLAM_E_HIP and "no CPU fallback" in str(ei.value)
