"""CPU: the restatement of ORBmatcher::SearchBySim3 in tests/sim3_match_common.py against hand-built known answers and against the truth of generated
keyframe pairs, so that the GPU tests may compare the kernel with it; the ctypes mirrors of include/oslam_hip.h, "SearchBySim3"."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sim3_match_common as smc
from object_slam_amd import sim3_match   # (at import: every test of this file belongs to the operator, also those that pin the restatement it is compared with)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in smc.hand_cases()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_gives_the_known_answer(name):
    c = CASES[name]
    match12, n_found, det = smc.run_pair(c, detail=True)
    e = c["expect"]
    rows = e.get("rows", list(range(len(match12))))
    print(name, match12.tolist(), n_found, {k: v.tolist() for k, v in det.items()})
    assert match12[rows].tolist() == list(e["match12"])
    assert n_found == int((match12 >= 0).sum())
    if "rows" not in e:
        assert n_found == sum(1 for v in e["match12"] if v >= 0)
    for k in ("vnMatch1", "vnMatch2"):
        if k in e:
            assert det[k].tolist() == list(e[k]), k
    if "level1" in e:
        assert det["level1"][rows].tolist() == list(e["level1"])


def test_tie_case_is_a_tie_in_two_cells_against_index_order():
    c = CASES["tie"]
    q = c["kf1"]["mp_desc"][0]
    d = [int(smc._POP[np.bitwise_xor(c["kf2"]["desc"][k], q)].sum()) for k in range(2)]
    assert d == [10, 10]
    px, py = smc._grid_cells(c["kf2"]["keysUn"], smc.BOUNDS, np.float32(0.1), np.float32(0.1))
    assert (px.tolist(), py.tolist()) == ([11, 9], [9, 11])   # ix outer reaches keypoint 1 first; iy outer, or index order, would reach keypoint 0


def test_transforms_and_scale_tables():
    sf, log_sf = smc.scale_factors()
    assert sf.dtype == np.float32 and sf[1] == np.float32(1.2) and sf[2] == np.float32(1.2) * np.float32(1.2) and log_sf == np.float32(np.log(np.float64(np.float32(1.2))))
    sR12, sR21, t21 = smc.sim3_transforms(1.0, np.eye(3), [0.25, -0.5, 1.0])
    assert np.array_equal(sR12, np.eye(3, dtype=np.float32)) and np.array_equal(sR21, np.eye(3, dtype=np.float32)) and t21.tolist() == [-0.25, 0.5, -1.0]
    R = smc.rodrigues(np.array([0.1, -0.2, 0.3])).astype(np.float32)
    sR12, sR21, t21 = smc.sim3_transforms(1.3, R, [0.25, -0.5, 1.0])
    s = np.float64(np.float32(1.3))
    assert np.array_equal(sR12, (s * R.astype(np.float64)).astype(np.float32)) and np.array_equal(sR21, ((1.0 / s) * R.T.astype(np.float64)).astype(np.float32))
    assert all(a.dtype == np.float32 for a in (sR12, sR21, t21))
    assert np.abs(sR21.astype(np.float64) @ (sR12.astype(np.float64) @ [1, 2, 3] + [0.25, -0.5, 1.0]) + t21 - [1, 2, 3]).max() < 1e-6


def test_generator():
    p = smc.make_pair(5, 300, 400, scale=1.1)
    n1, n2 = 300, 400
    assert len(p["kf1"]["has_mp"]) == n1 and len(p["kf2"]["has_mp"]) == n2 and p["s12"] == np.float32(1.1)
    assert all(p["kf1"][k].dtype == smc.empty_kf()[k].dtype for k in smc.ROW_KEYS)
    assert 0.55 <= p["kf1"]["has_mp"].mean() <= 0.65 and int((p["partner"] >= 0).sum()) == int(0.45 * 300)
    assert (p["matched_in"] != -1).sum() == 15 and ((p["matched_in"] >= 0) & (p["matched_in"] < n2)).any() and (p["matched_in"] == -2).any() and (p["matched_in"] >= n2).any()
    assert not (p["truth"][p["matched_in"] != -1] >= 0).any()
    # a true pair is one world point: both map points, through their own poses and the Sim3, land within the noise of each other's keypoint
    i1 = np.nonzero(p["partner"] >= 0)[0]
    i2 = p["partner"][i1]
    cam = lambda T, X: X.astype(np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3]
    P1, P2 = cam(p["T1w"], p["kf1"]["Xw"][i1]), cam(p["T2w"], p["kf2"]["Xw"][i2])
    assert np.abs(1.1 * P2 @ p["R12"].astype(np.float64).T + p["t12"] - P1).max() < 1e-4
    uv = smc._project(P1)
    assert np.hypot(uv[:, 0] - p["kf1"]["keysUn"]["x"][i1], uv[:, 1] - p["kf1"]["keysUn"]["y"][i1]).max() < 6.0
    d = smc._POP[np.bitwise_xor(p["kf1"]["mp_desc"][i1], p["kf2"]["desc"][i2])].sum(1)
    assert d.max() <= 4 + 2 * 8 and d.min() > 0
    assert np.array_equal(p["kf1"]["maxDistance"][i1] / smc.SF[-1], p["kf1"]["minDistance"][i1])
    q = smc.make_pair(5, 300, 400, scale=1.1)
    assert all(np.array_equal(p["kf2"][k], q["kf2"][k]) for k in smc.ROW_KEYS) and np.array_equal(p["truth"], q["truth"])


def test_restatement_recovers_the_truth_of_generated_pairs():
    """at least 90 % of the pairs SearchBySim3 may find, and no false pair, in every pair of the parity batch"""
    pairs = smc.parity_pairs()
    ref = smc.reference_of(pairs, "parity")
    for p, (match12, n_found) in zip(pairs, ref):
        want, got, false = smc.truth_score(p, match12)
        print("%s s12 = %.2f: %d of %d true pairs, %d false, nFound %d" % (p["name"], p["s12"], got, want, false, n_found))
        assert want >= 100 and got * 10 >= want * 9 and false == 0 and n_found == got


def test_struct_mirrors_have_the_sizes_of_the_header(tmp_path):
    pairs = [("oslam_sim3_pair_t", sim3_match.Pair), ("oslam_sim3_match_rows_t", sim3_match.Rows)]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "oslam_hip.h"\nint main(void) {\n' + "".join('    printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n, _ in pairs)
                   + "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    c_sizes = dict((l.split()[0], int(l.split()[1])) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, cls in pairs:
        assert C.sizeof(cls) == c_sizes[name], (name, C.sizeof(cls), c_sizes[name])
    assert sim3_match.PAIR_DTYPE.itemsize == c_sizes["oslam_sim3_pair_t"] == 204
    pr = sim3_match.pack_pairs([3, 0, 5], [0, 3, 3], [2, 4, 0], [8, 10, 14], [1.0, 1.1, 0.9], np.tile(np.eye(3), (3, 1, 1)), np.zeros((3, 3)), np.tile(np.eye(4), (3, 1, 1)),
                               np.tile(np.eye(4), (3, 1, 1)))
    assert pr["out_off"].tolist() == [0, 3, 3] and pr["th"].tolist() == [7.5] * 3 and pr["s12"][1] == np.float32(1.1)
    one = Pair = sim3_match.Pair.from_buffer_copy(pr[2].tobytes())
    assert (one.n1, one.off1, one.n2, one.off2, one.out_off, one.th, one.T2w[15], one.R12[4]) == (5, 3, 0, 14, 3, 7.5, 1.0, 1.0) and Pair is one


def test_no_device_is_an_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from object_slam_amd._lib import OSLAM_E_HIP, OslamError
    with pytest.raises(OslamError) as ei:
        sim3_match.Sim3Matcher(4, 400)
    assert ei.value.code == OSLAM_E_HIP and "no CPU fallback" in str(ei.value)
