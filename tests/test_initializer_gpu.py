"""GPU: the Initializer (include/oslam_hip.h, "Initializer") against the numpy restatement of tests/initializer_common.py — every score and count on the
dumped matrices, every determined hypothesis, the decision and the reconstruction from the kernel's winning matrix — against the truth of the generated
scenes, and the edges, batch independence and determinism of the operator."""
import os
import subprocess

import numpy as np
import pytest

import initializer_common as ic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "object_slam_amd")
TOL = 1e-4   # the project's bar (TOL of test_sim3_gpu.py): absolute on unit-norm hypotheses, on R and on the unit t, relative to the depth on points
KEYS = ("R21", "t21", "P3D", "triangulated", "status", "scores", "iter_scores", "hypotheses", "iter_inliers", "match_inliers")
PER_PROBLEM = ("R21", "t21", "status", "scores", "iter_scores", "hypotheses", "iter_inliers")
PER_KEY = ("P3D", "triangulated", "match_inliers")
f32 = np.float32


def _pack(scenes, seeds):
    from object_slam_amd import initializer as ini
    pr = ini.pack_problems([len(s["keys1"]) for s in scenes], [len(s["keys2"]) for s in scenes], [s["K"] for s in scenes], [s["sigma"] for s in scenes], seeds)
    cat = lambda k, w, dt: np.concatenate([np.asarray(s[k], dt).reshape(-1, w) for s in scenes]) if scenes else np.zeros((0, w), dt)
    return pr, (cat("keys1", 2, f32), cat("matches12", 1, np.int32).reshape(-1), cat("keys2", 2, f32))


def _run(handle, pr, arrays, its, **kw):
    """One call with the outputs pre-filled with a pattern.  Returns copies."""
    from object_slam_amd import initializer as ini
    n, M1 = len(pr), len(arrays[0])
    out = handle.initialize_batch(pr, *arrays, ini.make_params(max_iterations=its), dumps=True, R21=np.full((n, 3, 3), 7.0, f32), t21=np.full((n, 3), 7.0, f32),
                                  P3D=np.full((M1, 3), 7.0, f32), triangulated=np.full(M1, 0xAB, np.uint8), **kw)
    return {k: v.copy() for k, v in out.items()}


def _same(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in KEYS)


def _slice(out, pr, b):
    """the bytes of problem b in the outputs of a call"""
    o, n = int(pr["off1"][b]), int(pr["n1"][b])
    return [out[k][b].tobytes() for k in PER_PROBLEM] + [out[k][o:o + n].tobytes() for k in PER_KEY]


def _untouched(out, pr, b):
    o, n = int(pr["off1"][b]), int(pr["n1"][b])
    return (out["R21"][b] == 7.0).all() and (out["t21"][b] == 7.0).all() and (out["P3D"][o:o + n] == 7.0).all() and (out["triangulated"][o:o + n] == 0xAB).all()


@pytest.fixture(scope="module")
def handle():
    from object_slam_amd import initializer as ini
    h = ini.Initializer(16, 4096, 200)
    yield h
    h.close()


@pytest.fixture(scope="module")
def batches(handle):
    """the two calls of the module: name -> dict(scenes, seeds, its, pr, arrays, out)"""
    res = {}
    for which, its, seeds in (("long", ic.LONG_ITS, ic.LONG_SEEDS), ("short", ic.SHORT_ITS, ic.SHORT_SEEDS)):
        scenes = ic.parity_scenes(which)
        pr, arrays = _pack(scenes, seeds)
        res[which] = dict(scenes=scenes, seeds=seeds, its=its, pr=pr, arrays=arrays, out=_run(handle, pr, arrays, its), kinds=[s[0] for s in (ic.LONG_SCENES if which == "long" else ic.SHORT_SCENES)])
    return res


@pytest.fixture(scope="module")
def reference(batches):
    """the restatement's hypotheses of every problem, computed once: name -> list of initializer_common.hypotheses(...)"""
    return {w: [ic.hypotheses(s["keys1"], s["keys2"], s["matches12"], s["sigma"], seed, B["its"]) for s, seed in zip(B["scenes"], B["seeds"])] for w, B in batches.items()}


def _problems(batches, reference):
    for w, B in batches.items():
        for b, (s, hy) in enumerate(zip(B["scenes"], reference[w])):
            yield w, B, b, s, hy


def _ulps(a, b):
    a, b = f32(a), f32(b)
    if np.isnan(a) or np.isnan(b):
        return 0 if np.isnan(a) and np.isnan(b) else 1 << 30
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))   # (scores are >= 0)


def test_scoring_parity_on_the_dumped_matrices(batches, reference):
    """Every hypothesis the kernel dumped: the restatement's CheckHomography / CheckFundamental on THE DUMPED MATRIX give the same inlier count and the same
    score within one float32 ulp (both are an fp64 sum of at most 600 float terms rounded once; the restatement's sum is exact).  The inlier bits themselves
    are dumped for the best iterations: they must be equal."""
    total, worst = 0, 0
    for w, B, b, s, hy in _problems(batches, reference):
        out, o, n1 = B["out"], int(B["pr"]["off1"][b]), int(B["pr"]["n1"][b])
        if hy["N"] < 8:
            assert (out["iter_inliers"][b] == -1).all() and np.isnan(out["iter_scores"][b]).all() and np.isnan(out["hypotheses"][b]).all()
            continue
        for it in range(B["its"]):
            for model in (0, 1):
                M = out["hypotheses"][b, it, model]
                assert np.isfinite(M).all()
                sc, bits = ic.check_homography(M, ic.inv33(M), hy["pts"], s["sigma"]) if model == 0 else ic.check_fundamental(M, hy["pts"], s["sigma"])
                assert int(bits.sum()) == out["iter_inliers"][b, it, model], (w, b, it, model)
                u = _ulps(sc, out["iter_scores"][b, it, model])
                worst, total = max(worst, u), total + 1
                assert u <= 1, (w, b, it, model, float(sc), float(out["iter_scores"][b, it, model]))
        for model, best in ((0, out["status"][b, 5]), (1, out["status"][b, 6])):
            flags = np.zeros(n1, np.uint8)
            if best >= 0:
                M = out["hypotheses"][b, best, model]
                flags[hy["idx1"]] = (ic.check_homography(M, ic.inv33(M), hy["pts"], s["sigma"]) if model == 0 else ic.check_fundamental(M, hy["pts"], s["sigma"]))[1]
            assert np.array_equal(out["match_inliers"][o:o + n1, model], flags), (w, b, model)
    print("scores of %d hypotheses: worst difference %d ulp" % (total, worst))


def test_hypothesis_parity_with_the_restatement(batches, reference):
    """The dumped H21i / F21i back in normalised coordinates, unit Frobenius norm, sign rule, against the restatement's Hn / Fn.  Left out: a hypothesis whose
    relative singular-value gap is below GAP (undetermined), at most 1 in 20; and the F side of the noise-free planar scene, whose all-inlier samples are
    rank-deficient.  Where the two components of largest magnitude differ by less than TOL the sign rule itself is undetermined: both signs are tried."""
    total = left_out = 0
    worst = 0.0
    for w, B, b, s, hy in _problems(batches, reference):
        if hy["N"] < 8:
            continue
        for it in range(B["its"]):
            for model, key, gap in ((1, "Hn", "gapH"), (2, "Fn", "gapF")):
                if B["kinds"][b] == "planar0" and model == 2:
                    continue
                total += 1
                if hy[gap][it] < ic.GAP:
                    left_out += 1
                    continue
                got = ic.to_normalised(B["out"]["hypotheses"][b, it, model - 1], model, hy["T1"], hy["T2"])
                ref = hy[key][it].astype(np.float64).reshape(9)
                ref = ic.sign_rule(ref / np.linalg.norm(ref))
                d = np.abs(got - ref).max()
                mags = np.sort(np.abs(ref))
                if mags[-1] - mags[-2] < TOL:
                    d = min(d, np.abs(got + ref).max())
                worst = max(worst, d)
                assert d <= TOL, (w, b, it, model, d, hy[gap][it])
    print("worst difference of a unit-norm hypothesis %.3g; left out %d of %d" % (worst, left_out, total))
    assert total > 0 and left_out * 20 <= total


def _angle(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)) - 1) / 2, -1, 1))))


def test_decision_and_reconstruction(batches, reference):
    """status, scores, triangulated, R21, t21 and P3D against the restatement run from the KERNEL's winning matrix, and against the truth for the long scenes."""
    from object_slam_amd import initializer as ini
    total = left_out = 0
    worst = dict(R=0.0, t=0.0, P=0.0, par=0.0)
    for w, B, b, s, hy in _problems(batches, reference):
        out, o, n1 = B["out"], int(B["pr"]["off1"][b]), int(B["pr"]["n1"][b])
        st, sc = out["status"][b], out["scores"][b]
        if hy["N"] < 8:
            continue
        prm = dict(ic.REF, max_iterations=B["its"])
        bH, SH = ic.best_iteration(out["iter_scores"][b, :, 0])
        bF, SF = ic.best_iteration(out["iter_scores"][b, :, 1])
        RH, model = ic.choose_model(SH, SF)
        assert (st[5], st[6], st[1], st[2]) == (bH, bF, model, hy["N"]) and sc[0] == SH and sc[1] == SF and (sc[2] == RH or (np.isnan(sc[2]) and np.isnan(RH)))
        assert model == (2 if B["kinds"][b] == "general" else 1) or w == "short"
        best = bH if model == 1 else bF
        assert best >= 0
        M = out["hypotheses"][b, best, model - 1]
        inl = out["match_inliers"][o:o + n1, model - 1][hy["idx1"]].astype(bool)
        rec = ic.reconstruct(model, M, hy["pts"], hy["idx1"], n1, inl, s["K"], s["sigma"], prm)
        total += 1
        print("%s %d (%s, N %d): status %s, parallax %.4f; restatement: returned %d nGood %d motion %d aux %d near %s" % (
            w, b, B["kinds"][b], hy["N"], st.tolist(), sc[3], rec["returned"], rec["nGood"], rec["motion"], rec["aux"], rec["near"]))
        if rec["near"]:
            left_out += 1
            continue
        assert (st[0], st[3], st[4], st[7]) == (rec["returned"], rec["nGood"], rec["motion"], rec["aux"]), (w, b)
        # the parallax: cosParallax agrees to TOL
        dpar = abs(np.cos(np.radians(float(sc[3]))) - np.cos(np.radians(float(rec["parallax"]))))
        worst["par"] = max(worst["par"], dpar)
        assert dpar <= TOL
        if not rec["returned"]:
            assert _untouched(out, B["pr"], b)
            continue
        assert np.array_equal(out["triangulated"][o:o + n1], rec["triangulated"])
        dR, dt = np.abs(out["R21"][b] - rec["R"]).max(), np.abs(out["t21"][b] - rec["t"]).max()
        counted = np.abs(rec["P3D"]).sum(1) > 0
        assert np.array_equal(np.abs(out["P3D"][o:o + n1]).sum(1) > 0, counted)
        dP = (np.abs(out["P3D"][o:o + n1] - rec["P3D"]).max(1)[counted] / np.abs(rec["P3D"][counted, 2])).max()
        worst.update(R=max(worst["R"], dR), t=max(worst["t"], dt), P=max(worst["P"], dP))
        assert dR <= TOL and dt <= TOL and dP <= TOL, (w, b, dR, dt, dP)
        assert abs(np.linalg.norm(out["t21"][b]) - 1) <= 1e-6
        if w == "long":   # the truth, with the bounds derived in initializer_common.py (the noise-free planar scene included)
            m = out["triangulated"][o:o + n1].astype(bool) & s["truth"]
            aR = _angle(out["R21"][b], s["R"])
            at = float(np.degrees(np.arccos(np.clip(out["t21"][b].astype(np.float64) @ s["t"], -1, 1))))
            aP = float((np.linalg.norm(out["P3D"][o:o + n1][m] * s["scale"] - s["X1"][m], axis=1) / s["X1"][m][:, 2]).max())
            print("    truth: rotation %.3g deg, translation %.3g deg, points %.3g of depth, %d triangulated" % (aR, at, aP, m.sum()))
            assert st[0] == 1 and aR < ic.TRUTH_ROT_DEG and at < ic.TRUTH_TRANS_DEG and aP < ic.TRUTH_DEPTH and m.sum() >= 0.9 * s["truth"].sum()
    print("worst |dR| %.3g, |dt| %.3g, |dP| / depth %.3g, |d cosParallax| %.3g; left out %d of %d problems" % (worst["R"], worst["t"], worst["P"], worst["par"], left_out, total))
    assert left_out * 20 <= total
    assert ini.MODEL_H == 1 and ini.MODEL_F == 2


def test_selection_straddles_the_51st_value(batches):
    """the planar scenes of 51 and 52 matches count every match: sorted cosParallax[min(50, size - 1)] is the last of 51 and the last but one of 52"""
    B = batches["short"]
    for b, (kind, N, _) in enumerate(ic.SHORT_SCENES):
        if kind == "planar" and N in (51, 52):
            assert B["out"]["status"][b, 0] == 1 and B["out"]["status"][b, 3] == N


def test_too_few_matches_run_nothing_and_leave_the_outputs(batches):
    B = batches["short"]
    for b, (kind, N, _) in enumerate(ic.SHORT_SCENES):
        if N >= 8:
            continue
        assert B["out"]["status"][b].tolist() == [0, 0, N, 0, -1, -1, -1, 0]
        assert _untouched(B["out"], B["pr"], b) and (B["out"]["iter_inliers"][b] == -1).all()
    for w in batches:   # and every problem that does not return keeps the caller's bytes
        for b in range(len(batches[w]["pr"])):
            if batches[w]["out"]["status"][b, 0] != 1:
                assert _untouched(batches[w]["out"], batches[w]["pr"], b)


def test_eight_matches_draw_the_same_set_every_iteration(batches):
    from object_slam_amd import initializer as ini
    B = batches["short"]
    b = [i for i, s in enumerate(ic.SHORT_SCENES) if s[1] == 8][0]
    for it in range(B["its"]):
        assert sorted(ini.draw(B["seeds"][b], it, 8).tolist()) == list(range(8))
    for model in (0, 1):
        H = B["out"]["hypotheses"][b, :, model].reshape(B["its"], 9).astype(np.float64)
        H /= np.linalg.norm(H, axis=1)[:, None]
        assert np.abs(H - H[0]).max() <= TOL and len(set(B["out"]["iter_inliers"][b, :, model].tolist())) == 1


def test_samples_nan_ratio_and_input_validation(handle, batches):
    B = batches["short"]
    b = [i for i, s in enumerate(ic.SHORT_SCENES) if s[:2] == ("planar", 52)][0]
    s, seed, its = B["scenes"][b], B["seeds"][b], B["its"]
    good = np.array([ic.draw(seed, it, 52) for it in range(its)], np.int32)
    one_bad = good.copy()
    one_bad[3, 7] = one_bad[3, 0]     # a repeated index
    one_bad[5, 2] = 52                # an index outside the compacted list
    all_bad = np.full((its, 8), -1, np.int32)
    nan_key = dict(s, keys1=s["keys1"].copy())
    nan_key["keys1"][3, 0] = np.nan
    far_match = dict(s, matches12=s["matches12"].copy())
    far_match["matches12"][int(np.nonzero(s["matches12"] >= 0)[0][0])] = len(s["keys2"])
    scenes = [s, s, s, nan_key, far_match]
    pr, arrays = _pack(scenes, [seed] * 5)
    out = _run(handle, pr, arrays, its, samples=np.stack([good, one_bad, all_bad, good, good]))
    # the caller's draws of the generator reproduce the generator
    assert _slice(out, pr, 0) == _slice(B["out"], B["pr"], b)
    # a bad row scores 0 with no inliers and a NaN matrix; the other rows are unchanged
    for it in range(its):
        if it in (3, 5):
            assert (out["iter_scores"][1, it] == 0).all() and (out["iter_inliers"][1, it] == 0).all() and np.isnan(out["hypotheses"][1, it]).all()
        else:
            assert out["iter_scores"][1, it].tobytes() == out["iter_scores"][0, it].tobytes() and out["hypotheses"][1, it].tobytes() == out["hypotheses"][0, it].tobytes()
    # no score at all: RH = 0 / 0 is NaN and takes F, which has no matrix
    assert out["status"][2].tolist() == [0, 2, 52, 0, -1, -1, -1, 0] and np.isnan(out["scores"][2, 2]) and _untouched(out, pr, 2)
    # normalisation 5
    for k in (3, 4):
        assert out["status"][k].tolist() == [0, 0, 0, 0, -1, -1, -1, 0] and _untouched(out, pr, k) and (out["iter_inliers"][k] == -1).all()


def test_record_outside_the_arrays_and_capacity(handle, batches):
    from object_slam_amd import initializer as ini
    from object_slam_amd._lib import OSLAM_E_CAPACITY, OSLAM_E_INVALID, OslamError
    B = batches["short"]
    pr = B["pr"].copy()
    pr["off1"][4] = len(B["arrays"][0]) - int(pr["n1"][4]) + 1
    with pytest.raises(OslamError) as ei:
        _run(handle, pr, B["arrays"], B["its"])
    assert ei.value.code == OSLAM_E_INVALID
    out = _run(handle, pr, B["arrays"], B["its"], device=True)
    assert out["status"][4].tolist() == [-1, 0, 0, 0, -1, -1, -1, 0] and _untouched(out, B["pr"], 4)
    for b in range(len(pr)):
        if b != 4:
            assert _slice(out, pr, b) == _slice(B["out"], B["pr"], b)
    small = ini.Initializer(2, 64, 16)
    try:
        L = batches["long"]
        for args in ((B["pr"], B["arrays"], 16), (L["pr"][:1], tuple(a[:n] for a, n in zip(L["arrays"], (L["pr"]["n1"][0], L["pr"]["n1"][0], L["pr"]["n2"][0]))), 16),
                     (B["pr"][:2], tuple(a[:n] for a, n in zip(B["arrays"], (B["pr"]["n1"][:2].sum(), B["pr"]["n1"][:2].sum(), B["pr"]["n2"][:2].sum()))), 17)):
            for device in (False, True):
                with pytest.raises(OslamError) as ei:
                    _run(small, *args, device=device)
                assert ei.value.code == OSLAM_E_CAPACITY
    finally:
        small.close()


def test_batch_independence_and_determinism(handle, batches):
    for w, B in batches.items():
        again = _run(handle, B["pr"], B["arrays"], B["its"])
        assert _same(again, B["out"])
        dev = _run(handle, B["pr"], B["arrays"], B["its"], device=True)
        assert _same(dev, B["out"])
        order = list(range(len(B["scenes"])))[::-1]
        pr, arrays = _pack([B["scenes"][i] for i in order], [B["seeds"][i] for i in order])
        perm = _run(handle, pr, arrays, B["its"])
        for k, i in enumerate(order):
            assert _slice(perm, pr, k) == _slice(B["out"], B["pr"], i), (w, i)
    L = batches["long"]
    for b in (1, 3):
        pr, arrays = _pack([L["scenes"][b]], [L["seeds"][b]])
        alone = _run(handle, pr, arrays, L["its"])
        assert _slice(alone, pr, 0) == _slice(L["out"], L["pr"], b)


def test_adapter_program_matches_ctypes_path(tmp_path, batches):
    from object_slam_amd._lib import KP_DTYPE
    L = batches["long"]
    d = str(tmp_path)
    prog = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adapter_initializer_program.cc"), "-o", prog,
                           "-L", LIBDIR, "-loslam_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    for b in (1, 2):   # the general scene of 300 matches (F) and the planar one of 120 (H)
        s, o, n1 = L["scenes"][b], int(L["pr"]["off1"][b]), int(L["pr"]["n1"][b])
        for name, keys in (("keys1", s["keys1"]), ("keys2", s["keys2"])):
            kp = np.zeros(len(keys), KP_DTYPE)
            kp["x"], kp["y"] = keys[:, 0], keys[:, 1]
            kp.tofile(os.path.join(d, name + ".bin"))
        s["matches12"].astype(np.int32).tofile(os.path.join(d, "matches.bin"))
        with open(os.path.join(d, "meta.txt"), "w") as f:
            for k, v in dict(fx=s["K"][0], fy=s["K"][1], cx=s["K"][2], cy=s["K"][3], seed=L["seeds"][b], iterations=L["its"]).items():
                f.write("%s %r\n" % (k, float(v)))
        r = subprocess.run([prog, d], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        res = dict(line.split() for line in open(os.path.join(d, "out_results.txt")))
        st, out = L["out"]["status"][b], L["out"]
        assert (int(res["ok"]), int(res["model"]), int(res["N"]), int(res["nGood"]), int(res["motion"])) == (1, st[1], st[2], st[3], st[4])
        T = np.fromfile(os.path.join(d, "out_Tcw.bin"), f32).reshape(4, 4)
        assert T[:3, :3].tobytes() == out["R21"][b].tobytes() and T[:3, 3].tobytes() == out["t21"][b].tobytes() and T[3].tolist() == [0, 0, 0, 1]
        assert np.fromfile(os.path.join(d, "out_P3D.bin"), f32).tobytes() == out["P3D"][o:o + n1].tobytes()
        tri = out["triangulated"][o:o + n1].astype(bool)
        m = np.fromfile(os.path.join(d, "out_matches.bin"), np.int32)
        assert np.array_equal(m, np.where(tri, s["matches12"], -1)) and int(res["nmatches"]) == int(((s["matches12"] >= 0) & tri).sum())
