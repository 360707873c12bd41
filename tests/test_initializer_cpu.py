"""CPU: the host side of the Initializer (include/oslam_hip.h, "Initializer") — the draw rule, the struct mirrors, the exported symbols — and the
restatement of tests/initializer_common.py pinned against the truth of generated scenes, so that the GPU tests may compare with it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import initializer_common as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("oslam_init_create", "oslam_init_destroy", "oslam_init_draw", "oslam_init_initialize_batch", "oslam_init_initialize_batch_device", "oslam_init_set_timing",
           "oslam_init_last_kernel_ms")


def _angle(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.astype(np.float64).T @ Rb) - 1) / 2, -1, 1))))


def test_restatement_initialises_general_scenes_with_F_and_planar_scenes_with_H():
    """the long parity scenes against the truth, with the bounds derived in initializer_common.py"""
    for kind, N, sd in ic.LONG_SCENES:
        s = ic.parity_scene(kind, N, sd)
        r = ic.initialize(s["keys1"], s["keys2"], s["matches12"], s["K"], s["sigma"], 100 + sd)
        rec = r["rec"]
        assert r["returned"] == 1 and r["model"] == (2 if kind == "general" else 1) and r["N"] == N, (kind, r["returned"], r["model"])
        dR = _angle(rec["R"], s["R"])
        dt = float(np.degrees(np.arccos(np.clip(rec["t"].astype(np.float64) @ s["t"], -1, 1))))
        m = rec["triangulated"].astype(bool)
        assert not (m & ~(s["matches12"] >= 0)).any()
        tm = m & s["truth"]
        dP = float((np.linalg.norm(rec["P3D"][tm] * s["scale"] - s["X1"][tm], axis=1) / s["X1"][tm][:, 2]).max())
        print("%s %d: model %d, nGood %d, rotation %.3g deg, translation %.3g deg, points %.3g of depth" % (kind, N, r["model"], rec["nGood"], dR, dt, dP))
        assert dR < ic.TRUTH_ROT_DEG and dt < ic.TRUTH_TRANS_DEG and dP < ic.TRUTH_DEPTH and tm.sum() >= 0.9 * s["truth"].sum()


def test_restatement_does_not_initialise_from_a_pure_rotation():
    for sd in (1, 2, 3):
        s = ic.make_scene(sd, 200, "rotation")
        r = ic.initialize(s["keys1"], s["keys2"], s["matches12"], s["K"], s["sigma"], sd)
        assert r["returned"] == 0 and r["model"] == 1, (sd, r["returned"], r["model"])


def test_parity_scenes_leave_no_problem_out():
    """What tests/test_initializer_gpu.py relies on: with the restatement alone no CheckRT test of any motion of any parity problem lies within its margin
    of the threshold, the long general and planar scenes initialise, and the planar scenes of 51 and 52 matches count 51 and 52 points (the two sides of
    min(50, size - 1))."""
    for which, its, seeds in (("long", ic.LONG_ITS, ic.LONG_SEEDS), ("short", ic.SHORT_ITS, ic.SHORT_SEEDS)):
        for s, seed, (kind, N, _) in zip(ic.parity_scenes(which), seeds, ic.LONG_SCENES if which == "long" else ic.SHORT_SCENES):
            assert len(s["keys1"]) <= 512 and len(s["keys2"]) <= 512 and int((s["matches12"] >= 0).sum()) == N
            r = ic.initialize(s["keys1"], s["keys2"], s["matches12"], s["K"], s["sigma"], seed, dict(ic.REF, max_iterations=its))
            if N < 8:
                assert r["rec"] is None and r["model"] == 0
                continue
            assert r["rec"] is not None and not r["rec"]["near"], (kind, N)
            if which == "long":
                assert r["returned"] == 1 and r["model"] == (2 if kind == "general" else 1)
            if kind == "planar" and N in (51, 52):
                assert r["rec"]["nGood"] == N and r["returned"] == 1


def test_restatement_pieces():
    s = ic.parity_scene("general", 120, 14)
    i1, i2 = ic.compact(s["matches12"])
    assert len(i1) == 120 and (np.diff(i1) > 0).all() and np.array_equal(s["matches12"][i1], i2)
    p, T = ic.normalize(s["keys1"])
    assert p.dtype == np.float32 and abs(p.mean(0)).max() < 1e-5 and np.abs(np.abs(p).mean(0) - 1).max() < 1e-5
    q = (T.astype(np.float64) @ np.hstack([s["keys1"], np.ones((len(p), 1))]).T).T
    assert np.abs(q[:, :2] - p).max() < 1e-4
    M = np.array([[2, 0, 1], [0.5, 3, -1], [0, 0.25, 1]], np.float32)
    assert np.abs(ic.inv33(M).astype(np.float64) @ M - np.eye(3)).max() < 1e-6
    # without noise the true F takes every true match (an outlier near its epipolar line is one too), the true motion is among DecomposeE's four and counts them
    s = ic.make_scene(14, 120, "general", noise=0.0)
    i1, i2 = ic.compact(s["matches12"])
    K, R, t = ic.K_of(s["K"]).astype(np.float64), s["R"], s["t"]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F = (np.linalg.inv(K).T @ tx @ R @ np.linalg.inv(K)).astype(np.float32)
    pts = np.hstack([s["keys1"][i1], s["keys2"][i2]])
    score, bits = ic.check_fundamental(F, pts, 1.0)
    assert bits[s["truth"][i1]].all() and bits.sum() <= s["truth"].sum() + 6 and score > 0
    hits = [(np.abs(Rm - R).max() < 1e-5 and np.abs(tm - t).max() < 1e-5, ic.check_rt(Rm, tm, pts, bits, s["K"], 1.0)["nGood"]) for Rm, tm in ic.decompose_E(F, s["K"])]
    assert sum(h for h, _ in hits) == 1 and max(n for _, n in hits) == [n for h, n in hits if h][0] >= 0.8 * bits.sum()


def test_draw_rule():
    from object_slam_amd import initializer as ini
    from object_slam_amd._lib import OslamError
    for seed in (0, 1, 12345, 0xffffffff):
        for N in (8, 9, 51, 300, 100000):
            for it in (0, 1, 15, 199):
                d = ic.draw(seed, it, N)
                assert len(set(d)) == 8 and all(0 <= i < N for i in d)
                assert ini.draw(seed, it, N).tolist() == d
    assert sorted(ic.draw(5, 3, 8)) == list(range(8))
    assert len({tuple(ic.draw(7, it, 1000)) for it in range(50)}) == 50
    with pytest.raises(OslamError):
        ini.draw(1, 0, 7)


def test_struct_mirrors_have_the_sizes_of_the_header(tmp_path):
    from object_slam_amd import initializer as ini
    pairs = [("oslam_init_params_t", ini.Params), ("oslam_init_problem_t", ini.Problem)]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "oslam_hip.h"\nint main(void) {\n' + "".join('    printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n, _ in pairs)
                   + "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    c_sizes = dict((l.split()[0], int(l.split()[1])) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, cls in pairs:
        assert C.sizeof(cls) == c_sizes[name], (name, C.sizeof(cls), c_sizes[name])
    assert ini.PROBLEM_DTYPE.itemsize == c_sizes["oslam_init_problem_t"] and ini.PARAMS_DTYPE.itemsize == c_sizes["oslam_init_params_t"]


def test_adapter_class_compiles_and_links(tmp_path):
    """tests/adapter_initializer_compile_check.cc and the caller tests/adapter_initializer_program.cc, built as tests/test_adapter_gpu.py builds its own"""
    from object_slam_amd import build
    build.build_hip()
    libdir = os.path.join(ROOT, "object_slam_amd")
    for src, exe in (("adapter_initializer_compile_check.cc", "check"), ("adapter_initializer_program.cc", "prog")):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", src), "-o", str(tmp_path / exe),
                               "-L", libdir, "-loslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    assert subprocess.call([str(tmp_path / "check")]) == 0


def test_symbols_are_exported():
    from object_slam_amd._lib import lib
    L = lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name


def test_no_device_is_an_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from object_slam_amd import initializer as ini
    from object_slam_amd._lib import OSLAM_E_HIP, OslamError
    with pytest.raises(OslamError) as ei:
        ini.Initializer(4, 100, 200)
    assert ei.value.code == OSLAM_E_HIP and "no CPU fallback" in str(ei.value)
