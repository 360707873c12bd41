"""GPU: SearchBySim3 (include/oslam_hip.h, "SearchBySim3") against the numpy restatement of tests/sim3_match_common.py — every entry of match12 and
every nFound, no tolerance — and against the truth of generated keyframe pairs."""
import os
import subprocess

import numpy as np
import pytest

import sim3_match_common as smc
from object_slam_amd import sim3_match   # (at import: every test of this file needs the operator's module)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "object_slam_amd")
FILL = -77   # the pattern the output rows hold before a call


def _pack(pairs, share_kf1=False):
    rows, off1, off2, out_off, m_in = smc.concat_batch(pairs, share_kf1)
    n = len(pairs)
    pr = sim3_match.pack_pairs([len(p["kf1"]["has_mp"]) for p in pairs], off1, [len(p["kf2"]["has_mp"]) for p in pairs], off2, [p["s12"] for p in pairs],
                               np.stack([p["R12"] for p in pairs]).reshape(n, 3, 3), np.stack([p["t12"] for p in pairs]).reshape(n, 3), np.stack([p["T1w"] for p in pairs]),
                               np.stack([p["T2w"] for p in pairs]), [p["th"] for p in pairs], out_off)
    return pr, rows, m_in


def _call(matcher, pr, rows, m_in, device=False):
    out = matcher.search_batch(pr, rows, smc.CAM, smc.BOUNDS, smc.SF, smc.LOG_SF, matched_in=m_in, match12=np.full(len(m_in), FILL, np.int32), n_found=np.full(len(pr), FILL, np.int32),
                               device=device)
    return out["match12"], out["n_found"]


def _run(matcher, pairs, share_kf1=False, device=False):
    """[(match12 of the pair, nFound)] of one call"""
    pr, rows, m_in = _pack(pairs, share_kf1)
    match12, n_found = _call(matcher, pr, rows, m_in, device)
    return [(match12[o:o + n].copy(), int(f)) for o, n, f in zip(pr["out_off"], pr["n1"], n_found)]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(a, b))


@pytest.fixture(scope="module")
def matcher():
    m = sim3_match.Sim3Matcher(64, 2400)
    yield m
    m.close()


@pytest.fixture(scope="module")
def batch():
    """16 generated pairs, one at the 2400-keypoint capacity, one with n1 = 0, one with n2 = 0, and the hand-built cases"""
    gen = list(smc.parity_pairs())
    full = smc.make_pair(201, 2400, 2400, 1.05)
    no1, no2 = dict(gen[1], name="n1_zero", kf1=smc.empty_kf(0), matched_in=None), dict(gen[2], name="n2_zero", kf2=smc.empty_kf(0))
    pairs = gen + [full, no1, no2] + smc.hand_cases()
    return dict(pairs=pairs, n_gen=len(gen), ref=smc.reference_of(pairs, "gpu_batch"))


@pytest.fixture(scope="module")
def first(matcher, batch):
    return _run(matcher, batch["pairs"])


def test_parity_with_the_restatement(batch, first):
    bad = []
    for p, (m_ref, f_ref), (m, f) in zip(batch["pairs"], batch["ref"], first):
        diff = np.nonzero(m != m_ref)[0]
        print("%-16s n1 %4d n2 %4d nFound %4d (restatement %4d), %d entries differ" % (p["name"], len(p["kf1"]["has_mp"]), len(p["kf2"]["has_mp"]), f, f_ref, len(diff)))
        if len(diff) or f != f_ref:
            bad.append((p["name"], diff[:8].tolist(), m[diff[:8]].tolist(), m_ref[diff[:8]].tolist(), f, f_ref))
    assert not bad, bad
    assert first[batch["n_gen"]][1] > 500 and first[batch["n_gen"] + 1][1] == 0 and first[batch["n_gen"] + 2][1] == 0
    # both directions are populated, and the matches on entry are honoured, in what was compared
    assert all(f >= 100 for _, f in first[:batch["n_gen"]])
    for p, (m, _) in zip(batch["pairs"][:batch["n_gen"]], first):
        assert not (m[p["matched_in"] != -1] >= 0).any()


def test_hand_built_cases_give_their_known_answers(batch, first):
    for p, (m, f) in zip(batch["pairs"], first):
        if "expect" in p:
            rows = p["expect"].get("rows", list(range(len(m))))
            assert m[rows].tolist() == list(p["expect"]["match12"]), p["name"]
            assert f == int((m >= 0).sum())


def test_kernel_recovers_the_truth(batch, first):
    for p, (m, f) in zip(batch["pairs"][:batch["n_gen"]], first):
        want, got, false = smc.truth_score(p, m)
        assert want >= 100 and got * 10 >= want * 9 and false == 0 and f == got, (p["name"], want, got, false, f)


def test_pairs_are_independent(matcher, batch, first):
    pairs = batch["pairs"]
    assert _same(_run(matcher, pairs[::-1])[::-1], first)
    for j in list(range(0, batch["n_gen"], 5)) + list(range(batch["n_gen"], len(pairs))):
        assert _same(_run(matcher, [pairs[j]]), [first[j]]), pairs[j]["name"]
    # pairs that share the rows of KF1 (the current keyframe against three candidates) give what separate copies of KF1 give
    a, b, c = pairs[0], pairs[3], pairs[6]
    n1 = len(a["kf1"]["has_mp"])
    fit = lambda m: m[:n1] if len(m) >= n1 else np.concatenate([m, np.full(n1 - len(m), -1, np.int32)])   # (any value is a legal entry)
    trio = [a, dict(b, kf1=a["kf1"], matched_in=fit(b["matched_in"]), th=np.float32(10.0)), dict(c, kf1=a["kf1"], matched_in=None, s12=a["s12"], R12=a["R12"], t12=a["t12"], T1w=a["T1w"])]
    shared, separate = _run(matcher, trio, share_kf1=True), _run(matcher, trio)
    assert _same(shared, separate) and _same(shared[:1], first[:1])
    assert _same(shared, [smc.run_pair(p) for p in trio])


def test_host_and_device_entry_points_agree(matcher, batch, first):
    assert _same(_run(matcher, batch["pairs"], device=True), first)
    # one pair of keyframes without keypoints: no rows at all, so on the device path every per-keypoint array is an empty one, which gets a placeholder address
    empty = [dict(batch["pairs"][1], name="no_rows", kf1=smc.empty_kf(0), kf2=smc.empty_kf(0), matched_in=None)]
    host = _run(matcher, empty)
    assert len(host) == 1 and len(host[0][0]) == 0 and host[0][1] == 0
    assert _same(_run(matcher, empty, device=True), host)


def test_refusals(matcher, batch, first):
    from object_slam_amd._lib import OSLAM_E_CAPACITY, OSLAM_E_INVALID, OslamError
    pairs = batch["pairs"][:3]
    pr, rows, m_in = _pack(pairs)
    with pytest.raises(OslamError) as ei:
        sim3_match.Sim3Matcher(4, 2401)
    assert ei.value.code == OSLAM_E_INVALID
    small = sim3_match.Sim3Matcher(2, 360)
    try:
        cases = [("three pairs, two allowed", small, pr), ("350 .. 400 keypoints, 360 allowed", small, pr[:2])]
        for field in ("n1", "n2"):
            neg = pr.copy()
            neg[field][1] = -1
            cases.append(("negative " + field, matcher, neg))
        for what, m, recs in cases:
            match12, n_found = np.full(len(m_in), FILL, np.int32), np.full(len(recs), FILL, np.int32)
            with pytest.raises(OslamError) as ei:
                m.search_batch(recs, rows, smc.CAM, smc.BOUNDS, smc.SF, smc.LOG_SF, matched_in=m_in, match12=match12, n_found=n_found)
            assert ei.value.code == OSLAM_E_CAPACITY, what
            assert (match12 == FILL).all() and (n_found == FILL).all(), what
        # the device entry point cannot read the records: more pairs than the handle allows is refused, a record that does not fit gets -2 and nothing else
        match12, n_found = np.full(len(m_in), FILL, np.int32), np.full(3, FILL, np.int32)
        with pytest.raises(OslamError) as ei:
            small.search_batch(pr, rows, smc.CAM, smc.BOUNDS, smc.SF, smc.LOG_SF, matched_in=m_in, match12=match12, n_found=n_found, device=True)
        assert ei.value.code == OSLAM_E_CAPACITY and (match12 == FILL).all() and (n_found == FILL).all()
    finally:
        small.close()
    for field, value in (("n1", -1), ("n2", 2401), ("off2", len(rows["has_mp"])), ("out_off", len(m_in))):
        recs = pr.copy()
        recs[field][1] = value
        match12, n_found = _call(matcher, recs, rows, m_in, device=True)
        o, n = pr["out_off"][1], pr["n1"][1]
        assert n_found[1] == -2 and (match12[o:o + n] == FILL).all(), field
        for j in (0, 2):
            assert n_found[j] == first[j][1] and np.array_equal(match12[pr["out_off"][j]:pr["out_off"][j] + pr["n1"][j]], first[j][0]), field
    # a Sim3 or a pose that is not finite, or a scale that is not positive, in one pair of three
    def poison(field, value, index=None):
        recs = pr.copy()
        if index is None:
            recs[field][1] = value
        else:
            recs[field][1][index] = value
        return recs
    for what, recs in (("s12 NaN", poison("s12", np.nan)), ("s12 inf", poison("s12", np.inf)), ("s12 0", poison("s12", 0.0)), ("s12 < 0", poison("s12", -1.0)),
                       ("R12 NaN", poison("R12", np.nan, (1, 2))), ("t12 inf", poison("t12", np.inf, 0)), ("T1w NaN", poison("T1w", np.nan, (2, 3))),
                       ("T2w -inf", poison("T2w", -np.inf, (0, 0)))):
        for device in (False, True):
            match12, n_found = _call(matcher, recs, rows, m_in, device)
            o, n = pr["out_off"][1], pr["n1"][1]
            assert n_found[1] == -1 and (match12[o:o + n] == -1).all(), what
            for j in (0, 2):
                assert n_found[j] == first[j][1] and np.array_equal(match12[pr["out_off"][j]:pr["out_off"][j] + pr["n1"][j]], first[j][0]), what


def test_adapter_program_matches_the_restatement(tmp_path, batch):
    from object_slam_amd import build
    build.build_hip()
    d = str(tmp_path)
    p = batch["pairs"][1]
    for tag, kf, pose in (("1", p["kf1"], p["T1w"]), ("2", p["kf2"], p["T2w"])):
        for name, a in dict(keys=kf["keysUn"], desc=kf["desc"], has_mp=kf["has_mp"], Xw=kf["Xw"], mp_desc=kf["mp_desc"], maxD=kf["maxDistance"], minD=kf["minDistance"],
                            pose=pose).items():
            np.ascontiguousarray(a).tofile(os.path.join(d, name + tag + ".bin"))
    p["matched_in"].astype(np.int32).tofile(os.path.join(d, "matched.bin"))
    np.concatenate([[p["s12"]], p["R12"].reshape(-1), p["t12"]]).astype(np.float32).tofile(os.path.join(d, "sim3.bin"))
    smc.SF.tofile(os.path.join(d, "scale.bin"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        for k, v in dict(fx=smc.CAM[0], fy=smc.CAM[1], cx=smc.CAM[2], cy=smc.CAM[3], minX=smc.BOUNDS[0], minY=smc.BOUNDS[1], maxX=smc.BOUNDS[2], maxY=smc.BOUNDS[3],
                         logScaleFactor=smc.LOG_SF).items():
            f.write("%s %r\n" % (k, float(v)))
    prog = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adapter_sim3_match_program.cc"), "-o", prog,
                           "-L", LIBDIR, "-loslam_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    r = subprocess.run([prog, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    m_ref, f_ref = batch["ref"][1]
    assert lines[0] == "nFound %d" % f_ref and f_ref > 100
    after = np.array([int(l.split()[1]) for l in lines[1:] if l], np.int32)
    assert np.array_equal(after, np.where(m_ref >= 0, m_ref, p["matched_in"]))   # vpMatches12 updated as :1319 does
