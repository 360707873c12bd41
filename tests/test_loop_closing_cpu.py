"""No GPU: pins the restatements of tests/loop_closing_common.py by facts that do not depend on them.  The KeyFrame-pair SearchByBoW in two independent
forms and on hand cases that carry their answers; CorrectLoop's propagation and the map update after global BA against a known world transform G (the
project's bar: 1e-4 relative to max(1, |.|), no exclusions, poses far from the origin included); the header, build.SOURCES and the ctypes mirrors; and the
`parent` validation of the host entry point as a stand-alone program under AddressSanitizer and UBSan."""
import os
import re
import subprocess

import numpy as np
import pytest

import loop_closing_common as lcc
import sim3_opt_common as soc

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
BAR = 1e-4
FAR = (3000.0, -1500.0, 4000.0)   # a world whose origin is kilometres away: float32 poses there carry ~2.4e-4 absolute in t


def close(a, b):
    """the project's bar: |a - b| <= 1e-4 max(1, |b|) with |b| the magnitude of the quantity (its norm over the last axis)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.maximum(1.0, np.linalg.norm(b.reshape(b.shape[0], -1), axis=1)) if b.ndim > 1 else np.maximum(1.0, np.abs(b))
    err = np.linalg.norm((a - b).reshape(b.shape[0], -1), axis=1) if b.ndim > 1 else np.abs(a - b)
    return bool((err <= BAR * scale).all()), float((err / scale).max()) if err.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_bow_kf_hand_cases():
    for c in lcc.bow_kf_hand_cases():
        kw = {k: c[k] for k in ("keys1", "desc1", "valid1", "node1", "keys2", "desc2", "valid2", "node2", "nnratio", "checkOri")}
        for fn in (lcc.search_by_bow_kf, lcc.search_by_bow_kf_literal):
            nm, m = fn(**kw)
            np.testing.assert_array_equal(m, c["expect"], err_msg=c["name"])
            assert nm == c["nmatches"], c["name"]


def test_bow_kf_two_forms_agree_on_200_pairs():
    rng = np.random.default_rng(5)
    total = removed = 0
    for i in range(200):
        N1, N2 = int(rng.integers(0, 90)), int(rng.integers(0, 90))
        p = lcc.bow_kf_pair(rng, N1, N2, int(rng.integers(1, 12)))
        ori = bool(i % 2)
        a = lcc.search_by_bow_kf(**p, nnratio=(0.75, 0.9)[i % 3 == 0], checkOri=ori)
        b = lcc.search_by_bow_kf_literal(**p, nnratio=(0.75, 0.9)[i % 3 == 0], checkOri=ori)
        assert a[0] == b[0], i
        np.testing.assert_array_equal(a[1], b[1], err_msg=str(i))
        assert a[0] == int((a[1] >= 0).sum())
        m = a[1][a[1] >= 0]
        assert len(set(m.tolist())) == len(m) and all(p["valid2"][k] for k in m)   # a side-2 keypoint is given away once, and only with a map point
        total, removed = total + a[0], removed + int((a[1] == -2).sum())
    assert total > 1000 and removed >= 10, (total, removed)   # the generator exercises both the claims and the rotation check


# ---------------------------------------------------------------------------------------------------------------------------------------------
def _check_propagation_truth(p):
    r = lcc.propagate(p)
    n = len(p["Tiw"])
    assert r["status"].tolist()[:2] == [0, n]
    G = p["G"]
    s, RG, tG = G
    got = r["corrected_ref"] >= 0
    ok, worst = close(r["P"][got], lcc.apply_G(G, p["P"][got].astype(np.float64)))
    assert ok, ("points", worst)
    assert r["status"][2] == got.sum()
    for i in range(n):
        T0, T1 = p["Tiw"][i].astype(np.float64), r["Tiw"][i].astype(np.float64)
        Ow0, Ow1 = -T0[:3, :3].T @ T0[:3, 3], -T1[:3, :3].T @ T1[:3, 3]
        ok, worst = close(Ow1[None], lcc.apply_G(G, Ow0)[None])
        assert ok, ("centre", i, worst)
        assert np.abs(T1[:3, :3] - T0[:3, :3] @ RG.T).max() <= BAR, ("rotation", i)
        assert T1[3].tolist() == [0, 0, 0, 1]
        # Scorr[i] = Siw_old o G^-1: rotation R_i R_G^T, scale 1 / s, translation t_i - R_i R_G^T t_G / s
        rec = r["Scorr"][i]
        Ri = T0[:3, :3] @ RG.T
        assert np.abs(rec[:9].reshape(3, 3) - Ri).max() <= BAR and abs(rec[12] - 1.0 / s) <= BAR * max(1.0, 1.0 / s)
        ok, worst = close(rec[9:12][None], (T0[:3, 3] - Ri @ tG / s)[None])
        assert ok, ("Scorr t", i, worst)
        assert np.abs(r["Snc"][i][:9].reshape(3, 3) - T0[:3, :3]).max() <= BAR and r["Snc"][i][12] == 1.0
        np.testing.assert_array_equal(r["Snc"][i][9:12], T0[:3, 3])
    return r


@pytest.mark.parametrize("centre", [(0.0, 0.0, 0.0), FAR])
@pytest.mark.parametrize("s_G", [0.5, 2.0, None])
def test_propagation_against_truth(centre, s_G):
    for seed, (n_kf, per_kf, n_points) in enumerate([(1, 20, 30), (2, 15, 25), (12, 40, 150)]):
        p = lcc.make_prop_problem(100 + seed, n_kf, per_kf, n_points, centre=centre, s_G=s_G, empty_kf=(3 if n_kf > 3 else None))
        r = _check_propagation_truth(p)
        if n_kf > 3:
            assert (r["corrected_ref"] >= 0).sum() > 50 and (p["bad"] != 0).any()
            assert not (r["corrected_ref"][p["bad"] != 0] >= 0).any()


def test_propagation_stamps_the_smallest_index_and_refuses():
    p = lcc.make_prop_problem(7, 6, 10, 40)
    p["entries"] = [np.array([], np.int32), np.array([5, -1, 7], np.int32), np.array([7, 9], np.int32), np.array([9, 7, 5, 11], np.int32), np.array([7], np.int32),
                    np.array([], np.int32)]
    p["bad"][:] = 0
    p["bad"][11] = 1
    r = lcc.propagate(p)
    assert r["corrected_ref"][[5, 7, 9, 11]].tolist() == [1, 1, 2, -1]           # 7 is held by keyframes 1, 2, 3 and 4; 11 is bad
    assert (np.delete(r["corrected_ref"], [5, 7, 9]) == -1).all()
    assert r["status"].tolist() == [0, 6, 3, 9]
    # the point of keyframe 1 and the point of keyframe 2 move by different Sim3 only through rounding: both are G(P)
    assert close(r["P"][[5, 7, 9]], lcc.apply_G(p["G"], p["P"][[5, 7, 9]].astype(np.float64)))[0]
    fill = dict(P=np.full((40, 3), 7.5), corrected_ref=np.full(40, -9))
    for bad in (dict(cur=6), dict(cur=-1), dict(Scw=np.concatenate([p["Scw"][:12], [0.0]])), dict(Scw=np.concatenate([[np.nan], p["Scw"][1:]])),
                dict(entries=p["entries"][:5] + [np.array([40], np.int32)]), dict(entries=p["entries"][:5] + [np.array([-2], np.int32)])):
        r = lcc.propagate(dict(p, **bad), fill)
        assert r["status"].tolist() == [-1, 6, 0, 0] and (r["P"] == 7.5).all() and (r["corrected_ref"] == -9).all()
    T = p["Tiw"].copy()
    T[2, 1, 3] = np.inf
    assert lcc.propagate(dict(p, Tiw=T))["status"][0] == -1


def test_compose_scw_is_the_matrix_product():
    rng = np.random.default_rng(3)
    for centre in ((0, 0, 0), FAR):
        Tmw = lcc.rand_poses(rng, 1, centre)[0]
        R, t, s = lcc.rand_rot(rng), rng.normal(0, 2, 3), float(rng.uniform(0.5, 2))
        rec, M = lcc.compose_scw(np.concatenate([R.reshape(9), t, [s]]), Tmw)
        want = lcc.pose44(s * R, t) @ Tmw.astype(np.float64)     # [sR | t] [Rmw | tmw]
        assert close(M[:3].astype(np.float64), want[:3])[0] and M[3].tolist() == [0, 0, 0, 1]
        assert close(rec[9:12][None], want[:3, 3][None])[0] and abs(rec[12] - s) < 1e-12
        assert np.abs(rec[:9].reshape(3, 3) - R @ Tmw[:3, :3].astype(np.float64)).max() <= BAR


# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("centre", [(0.0, 0.0, 0.0), FAR])
def test_gba_update_against_truth(centre):
    for seed, (name, parent, in_ba, status0, rounds, unreached) in enumerate(lcc.gba_trees()):
        p = lcc.make_gba_problem(40 + seed, parent, in_ba, 200, centre=centre)
        r = lcc.update_after_gba(p, dict(Tcw=np.full((len(parent), 4, 4), 3.25), P=np.full((200, 3), -1.5)))
        if status0 != 0:
            assert r["status"].tolist() == [-1, 0, 0, 0], name
            assert (r["Tcw"] == 3.25).all() and (r["P"] == -1.5).all(), name
            continue
        n_prop = int((np.asarray(in_ba) == 0).sum())
        assert r["status"].tolist()[:2] == [0, n_prop] and r["status"][3] == rounds, (name, r["status"])
        assert r["reached"].all(), name
        want = np.stack([p["Tcw"][k].astype(np.float64) @ p["Ginv"] for k in range(len(parent))])
        for k in range(len(parent)):
            ok, worst = close(r["Tcw"][k][:3, 3][None], want[k][:3, 3][None])
            assert ok and np.abs(r["Tcw"][k][:3, :3] - want[k][:3, :3]).max() <= BAR, (name, k, worst)
            if in_ba[k]:
                np.testing.assert_array_equal(r["Tcw"][k], p["TcwGBA"][k])
        good = p["bad"] == 0
        sel = good & (p["pt_in_ba"] == 0)
        ok, worst = close(r["P"][sel], lcc.apply_G(p["G"], p["P"][sel].astype(np.float64)))
        assert ok, (name, worst)
        np.testing.assert_array_equal(r["P"][good & (p["pt_in_ba"] != 0)], p["PosGBA"][good & (p["pt_in_ba"] != 0)])
        assert (r["P"][~good] == -1.5).all() and r["status"][2] == good.sum()


def test_gba_chain_of_five_rounds_in_the_written_parenthesisation():
    """(Tcw[c] * Twc[p]) * TcwGBA[p], not Tcw[c] * (Twc[p] * TcwGBA[p]): the two differ in the last bits and the restatement takes the first"""
    name, parent, in_ba, *_ = lcc.gba_trees()[0]
    p = lcc.make_gba_problem(1, parent, in_ba, 0)
    r = lcc.update_after_gba(p)
    T = r["Tcw"]
    differ = 0
    for c in range(5, 10):
        Twc = lcc.set_pose_twc(p["Tcw"][c - 1])
        np.testing.assert_array_equal(T[c], lcc.mat4_mul(lcc.mat4_mul(p["Tcw"][c], Twc), T[c - 1]))
        differ += int((T[c] != lcc.mat4_mul(p["Tcw"][c], lcc.mat4_mul(Twc, T[c - 1]))).any())
    assert differ > 0
    assert lcc.parent_check([-1, 0, 1]) == 0 and lcc.parent_check([1, 0]) == 2 and lcc.parent_check([0]) == 2 and lcc.parent_check([-1, 2]) == 1


# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_header_sources_and_mirrors(tmp_path):
    from object_slam_amd import build, loop_correct, matcher
    from object_slam_amd._lib import lib
    build.build_hip()
    header = open(os.path.join(ROOT, "include", "oslam_hip.h")).read()
    declared = set(re.findall(r"\b(oslam_loop_\w+)\s*\(", header))
    want = {"oslam_loop_correct_create", "oslam_loop_correct_destroy", "oslam_loop_compose_scw", "oslam_loop_compose_scw_device", "oslam_loop_propagate",
            "oslam_loop_propagate_device", "oslam_loop_update_after_gba", "oslam_loop_update_after_gba_device"}
    assert want <= declared, want - declared
    assert re.search(r"\boslam_match_search_by_bow_kf\s*\(", header)
    L = lib()
    for name in sorted(declared | {"oslam_match_search_by_bow_kf"}):
        assert hasattr(L, name), name
    assert "loop_correct.hip" in build.SOURCES and "bow_matcher.hip" in build.SOURCES
    import object_slam_amd
    assert object_slam_amd.LoopCorrector is loop_correct.LoopCorrector and object_slam_amd.loop_correct is loop_correct
    import ctypes as C
    pairs = [("oslam_loop_correct_problem_t", loop_correct.PROBLEM_DTYPE.itemsize, C.sizeof(loop_correct.Problem)),
             ("oslam_loop_gba_problem_t", loop_correct.GBA_PROBLEM_DTYPE.itemsize, C.sizeof(loop_correct.GbaProblem)),
             # the BoW structs keep the sizes they had before the KeyFrame-pair mode
             ("oslam_bow_job_t", 208, C.sizeof(matcher.BowJob)), ("oslam_bow_side1_t", 64, C.sizeof(matcher.BowSide1)), ("oslam_bow_side2_t", 72, C.sizeof(matcher.BowSide2))]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "oslam_hip.h"\nint main(void) {\n' + "".join('    printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n, _, _ in pairs)
                   + '    printf("refuse %zu\\n", offsetof(oslam_loop_gba_problem_t, refuse));\n    return 0;\n}\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    for name, a, b in pairs:
        assert int(got[name]) == a == b, (name, got[name], a, b)
    assert int(got["refuse"]) == loop_correct.GBA_PROBLEM_DTYPE.fields["refuse"][1] == 16


def test_parent_check_under_sanitizers(tmp_path):
    """tests/loop_parent_check.cc under AddressSanitizer and UBSan: valid trees, a cycle, a self-parent and indices out of range, every array in an exactly
    sized heap block"""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "loop_parent_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(here, "loop_parent_check.cc"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def test_no_device_is_an_error():
    import torch
    if torch.cuda.is_available():
        return   # (the GPU suite creates handles)
    from object_slam_amd import LoopCorrector
    from object_slam_amd._lib import OSLAM_E_HIP, OslamError
    with pytest.raises(OslamError) as ei:
        LoopCorrector(1, 1, 1, 1)
    assert ei.value.code == OSLAM_E_HIP


def test_adapter_program_compiles():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adapter_loop_correct_program.cc")])
