"""GPU: the Sim3 projection operators (include/oslam_hip.h, "Sim3 projection") against the sequential numpy restatement of tests/sim3_project_common.py — every
output entry and every count, no tolerance — against hand-written answers and against the truth of generated problems."""
import os
import subprocess

import numpy as np
import pytest

import sim3_project_common as spc
from object_slam_amd import sim3_project   # (at import: every test of this file needs the operator's module)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "object_slam_amd")
FILL = -77   # the pattern the output rows hold before a call


def _pack(problems, share_pts=False):
    kf, pts, skip, kp_off, pt_off, kp_out, pt_out = spc.concat_batch(problems, share_pts)
    n = len(problems)
    pr = sim3_project.pack_problems([len(p["kf"]["state"]) for p in problems], kp_off, [len(p["skip"]) for p in problems], pt_off,
                                    np.stack([p["Scw"] for p in problems]).reshape(n, 4, 4), [p["th"] for p in problems], kp_out, pt_out)
    return pr, kf, pts, skip


def _call(proj, mode, pr, kf, pts, skip, device=False):
    """the raw outputs of one call, over FILL: search (matched, n_matches, n_passes), fuse (fused_kp, replace, n_fused)"""
    n_kp_out, n = len(kf["state"]), len(pr)
    if mode == "search":
        out = proj.search_batch(pr, kf, pts, spc.CAM, spc.BOUNDS, spc.SF, spc.LOG_SF, skip=skip, matched=np.full(n_kp_out, FILL, np.int32), n_matches=np.full(n, FILL, np.int32),
                                n_passes=np.full(n, FILL, np.int32), n_pt_out=len(skip), n_kp_out=n_kp_out, device=device)
        return out["matched"], out["n_matches"], out["n_passes"]
    out = proj.fuse_batch(pr, kf, pts, spc.CAM, spc.BOUNDS, spc.SF, spc.LOG_SF, skip=skip, fused_kp=np.full(len(skip), FILL, np.int32), replace=np.full(len(skip), FILL, np.int32),
                          n_fused=np.full(n, FILL, np.int32), n_pt_out=len(skip), device=device)
    return out["fused_kp"], out["replace"], out["n_fused"]


def _split(mode, pr, raw):
    """per problem, in run_problem's form: search (matched, n), fuse (fused_kp, replace, n)"""
    if mode == "search":
        return [(raw[0][o:o + n].copy(), int(c)) for o, n, c in zip(pr["kp_out_off"], pr["n_kp"], raw[1])]
    return [(raw[0][o:o + n].copy(), raw[1][o:o + n].copy(), int(c)) for o, n, c in zip(pr["pt_out_off"], pr["n_pts"], raw[2])]


def _run(proj, mode, problems, share_pts=False, device=False):
    pr, kf, pts, skip = _pack(problems, share_pts)
    return _split(mode, pr, _call(proj, mode, pr, kf, pts, skip, device))


def _same(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def proj():
    m = sim3_project.Sim3Projector(64, 2400, 40000)
    yield m
    m.close()


@pytest.fixture(scope="module")
def batches():
    """per mode: six generated problems, one at the 2400-keypoint capacity with 6007 points, one with n_pts = 0, one with n_kp = 0, one with both, and the hand cases"""
    out = {}
    for j, mode in enumerate(("search", "fuse")):
        gen = [p for p in spc.parity_problems() if p["mode"] == mode]
        full = spc.full_problems()[j]
        no_pts = dict(gen[1], name="n_pts_zero", pts=spc.empty_pts(0), skip=np.zeros(0, np.uint8))
        no_kp = dict(gen[2], name="n_kp_zero", kf=spc.empty_kf(0))
        neither = dict(gen[3], name="both_zero", kf=spc.empty_kf(0), pts=spc.empty_pts(0), skip=np.zeros(0, np.uint8))
        problems = gen + [full, no_pts, no_kp, neither] + [c for c in spc.hand_cases() if c["mode"] == mode]
        out[mode] = dict(problems=problems, n_gen=len(gen) + 1, ref=spc.reference_of(problems, "gpu_batch_" + mode))
    return out


@pytest.fixture(scope="module")
def first(proj, batches):
    out = {}
    for mode, b in batches.items():
        pr, kf, pts, skip = _pack(b["problems"])
        raw = _call(proj, mode, pr, kf, pts, skip)
        out[mode] = dict(res=_split(mode, pr, raw), passes=raw[2] if mode == "search" else None)
    return out


def test_parity_with_the_restatement(batches, first):
    bad = []
    for mode, b in batches.items():
        for j, (p, ref, got) in enumerate(zip(b["problems"], b["ref"], first[mode]["res"])):
            ndiff = [int((np.asarray(x) != np.asarray(y)).sum()) for x, y in zip(got[:-1], ref[:-1])]
            print("%-6s %-24s n_kp %4d n_pts %4d count %4d (restatement %4d), entries that differ: %s%s" % (mode, p["name"], len(p["kf"]["state"]), len(p["skip"]), got[-1], ref[-1], ndiff,
                                                                                                         "" if mode == "fuse" else ", passes %d" % first[mode]["passes"][j]))
            if any(ndiff) or got[-1] != ref[-1]:
                bad.append((mode, p["name"], ndiff, got[-1], ref[-1]))
    assert not bad, bad
    for mode, b in batches.items():
        res, g = first[mode]["res"], b["n_gen"]
        assert res[g - 1][-1] > 500 and [r[-1] for r in res[g:g + 3]] == [0, 0, 0]
        assert all(r[-1] >= 100 for r in res[:g])
    # every claim needs a pass that confirms it (the hand cases hold the chains that need more)
    assert first["search"]["passes"][:batches["search"]["n_gen"]].min() >= 2
    # ... and so are the three Fuse branches and the "added earlier in this call" answer
    rep = np.concatenate([r[1] for r in first["fuse"]["res"][:batches["fuse"]["n_gen"]]])
    fk = np.concatenate([r[0] for r in first["fuse"]["res"][:batches["fuse"]["n_gen"]]])
    assert (rep == spc.FUSE_ADDED).sum() > 100 and (rep == spc.FUSE_OCCUPANT).sum() > 100 and (rep >= 0).sum() > 10 and ((rep == -1) & (fk >= 0)).sum() > 10


def test_hand_built_cases_give_their_known_answers(batches, first):
    seen = 0
    for mode, b in batches.items():
        for p, got in zip(b["problems"], first[mode]["res"]):
            if "expect" not in p:
                continue
            e = p["expect"]
            seen += 1
            if mode == "search":
                assert got[0].tolist() == list(e["matched"]) and got[1] == e["n"], p["name"]
            else:
                assert got[0].tolist() == list(e["fused_kp"]) and got[1].tolist() == list(e["replace"]) and got[2] == e["n"], p["name"]
    assert seen == len(spc.hand_cases())
    # the chain of ten in windows beyond the candidate cache took a pass per link
    names = [p["name"] for p in batches["search"]["problems"]]
    assert first["search"]["passes"][names.index("big_window")] >= spc.CACHE_CASE_CANDIDATES and first["search"]["passes"][names.index("chain")] >= 4


def test_kernel_recovers_the_truth(batches, first):
    for mode, b in batches.items():
        for p, got in zip(b["problems"][:b["n_gen"]], first[mode]["res"]):
            want, found, false = spc.truth_score(p, got)
            assert want >= 100 and found * 10 >= want * 9 and false == 0 and spc.count_of(got) == found, (p["name"], want, found, false, spc.count_of(got))


def test_problems_are_independent(proj, batches, first):
    for mode, b in batches.items():
        problems, res = b["problems"], first[mode]["res"]
        assert _same(_run(proj, mode, problems[::-1])[::-1], res)
        for j in list(range(0, b["n_gen"], 3)) + list(range(b["n_gen"], len(problems))):
            assert _same(_run(proj, mode, [problems[j]]), [res[j]]), problems[j]["name"]
    # Fuse problems that share one set of point rows (the corrected keyframes of one loop against mvpLoopMapPoints) give what separate copies give
    b = batches["fuse"]
    a = b["problems"][0]
    rng = np.random.default_rng(5)
    others = []
    for j, q in enumerate(b["problems"][1:4]):
        n = len(a["skip"])
        others.append(dict(q, pts=a["pts"], skip=(rng.random(n) < 0.1).astype(np.uint8), th=np.float32(4.0 + j)))
    group = [a, dict(a, name="same_again")] + others
    shared, separate = _run(proj, "fuse", group, share_pts=True), _run(proj, "fuse", group)
    assert _same(shared, separate) and _same(shared[:1], first["fuse"]["res"][:1]) and _same(shared[1:2], shared[:1])
    assert _same(shared, [spc.run_problem(p) for p in group])


def test_host_and_device_entry_points_agree(proj, batches, first):
    for mode, b in batches.items():
        assert _same(_run(proj, mode, b["problems"], device=True), first[mode]["res"])
        # one problem without keypoints and points: no rows at all, so on the device path every array is an empty one, which gets a placeholder address
        empty = [dict(b["problems"][0], name="no_rows", kf=spc.empty_kf(0), pts=spc.empty_pts(0), skip=np.zeros(0, np.uint8))]
        host = _run(proj, mode, empty)
        assert len(host) == 1 and host[0][-1] == 0 and all(len(x) == 0 for x in host[0][:-1])
        assert _same(_run(proj, mode, empty, device=True), host)


def _rows(mode, pr, j):
    return (pr["kp_out_off"][j], pr["n_kp"][j]) if mode == "search" else (pr["pt_out_off"][j], pr["n_pts"][j])


@pytest.mark.parametrize("mode", ["search", "fuse"])
def test_refusals(proj, batches, first, mode):
    from object_slam_amd._lib import OSLAM_E_CAPACITY, OSLAM_E_INVALID, OslamError
    problems, res = batches[mode]["problems"][:3], first[mode]["res"]
    pr, kf, pts, skip = _pack(problems)
    n_pts_total = len(skip)

    def neighbours_ok(raw, what):
        for j in (0, 2):
            assert _same([_split(mode, pr, raw)[j]], [res[j]]), what

    with pytest.raises(OslamError) as ei:
        sim3_project.Sim3Projector(4, 2401, 1000)
    assert ei.value.code == OSLAM_E_INVALID
    small, few = sim3_project.Sim3Projector(2, 360, 40000), sim3_project.Sim3Projector(4, 2400, n_pts_total - 1)
    try:
        def refused(what, m, recs, code, device=False):
            """the call raises `code` and leaves every output row as it was"""
            outs = [np.full(len(kf["state"]) if mode == "search" else n_pts_total, FILL, np.int32), np.full(len(recs) if mode == "search" else n_pts_total, FILL, np.int32),
                    np.full(len(recs), FILL, np.int32)]
            with pytest.raises(OslamError) as ei:
                if mode == "search":
                    m.search_batch(recs, kf, pts, spc.CAM, spc.BOUNDS, spc.SF, spc.LOG_SF, skip=skip, matched=outs[0], n_matches=outs[1], n_passes=outs[2], n_pt_out=n_pts_total, device=device)
                else:
                    m.fuse_batch(recs, kf, pts, spc.CAM, spc.BOUNDS, spc.SF, spc.LOG_SF, skip=skip, fused_kp=outs[0], replace=outs[1], n_fused=outs[2], n_pt_out=n_pts_total, device=device)
            assert ei.value.code == code, what
            assert all((a == FILL).all() for a in outs), what

        def with_field(field, value):
            recs = pr.copy()
            recs[field][1] = value
            return recs

        refused("three problems, two allowed", small, pr, OSLAM_E_CAPACITY)
        refused("350 .. 400 keypoints, 360 allowed", small, pr[1:3], OSLAM_E_CAPACITY)
        refused("more point rows than max_points_total", few, pr, OSLAM_E_CAPACITY)
        for field in ("n_kp", "n_pts"):
            refused("negative " + field, proj, with_field(field, -1), OSLAM_E_CAPACITY)
        # rows outside the arrays
        for field, value in (("kp_off", len(kf["state"])), ("pt_off", n_pts_total), ("pt_out_off", n_pts_total)) + ((("kp_out_off", len(kf["state"])),) if mode == "search" else ()):
            refused(field + " outside", proj, with_field(field, value), OSLAM_E_INVALID)
        # the device entry points cannot read the records: what the call as a whole exceeds is refused, a record that does not fit gets -2 and nothing else
        refused("problems, device", small, pr, OSLAM_E_CAPACITY, device=True)
        refused("point rows, device", few, pr, OSLAM_E_CAPACITY, device=True)
    finally:
        small.close()
        few.close()
    for field, value in (("n_kp", -1), ("n_pts", -1), ("n_kp", 2401), ("kp_off", len(kf["state"])), ("pt_off", n_pts_total), ("pt_out_off", n_pts_total)) + (
            (("kp_out_off", len(kf["state"])),) if mode == "search" else ()):
        recs = pr.copy()
        recs[field][1] = value
        raw = _call(proj, mode, recs, kf, pts, skip, device=True)
        o, n = _rows(mode, pr, 1)
        assert raw[1 if mode == "search" else 2][1] == -2 and all((a[o:o + n] == FILL).all() for a in (raw[:1] if mode == "search" else raw[:2])), (field, value)
        if mode == "search":
            assert raw[2][1] == FILL
        neighbours_ok(raw, field)
    # an Scw that is not finite, or a scale that is not positive, in one problem of three
    for what, index, value in (("NaN in the rotation", (1, 2), np.nan), ("inf in the translation", (0, 3), np.inf), ("-inf in row 0", (0, 0), -np.inf), ("a zero first row", (0, slice(0, 3)), 0.0)):
        recs = pr.copy()
        recs["Scw"][1][index] = value
        for device in (False, True):
            raw = _call(proj, mode, recs, kf, pts, skip, device)
            o, n = _rows(mode, pr, 1)
            assert raw[1 if mode == "search" else 2][1] == -1 and all((a[o:o + n] == -1).all() for a in (raw[:1] if mode == "search" else raw[:2])), what
            neighbours_ok(raw, what)
    # row 3 of Scw is not read
    recs = pr.copy()
    recs["Scw"][1][3] = np.nan
    assert _same(_split(mode, pr, _call(proj, mode, recs, kf, pts, skip)), res[:3])


def test_adapter_program_matches_the_restatement(tmp_path, batches):
    from object_slam_amd import build
    build.build_hip()
    prog = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adapter_sim3_project_program.cc"), "-o", prog,
                           "-L", LIBDIR, "-loslam_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    base = batches["search"]["problems"][1]
    cut = {k: v[:80] for k, v in base["pts"].items()}
    decisions = []
    for tag, p in (("all", base), ("first80", dict(base, pts=cut, skip=base["skip"][:80]))):
        d = str(tmp_path / tag)
        os.makedirs(d)
        n_kp, n_pts = len(p["kf"]["state"]), len(p["skip"])
        rng = np.random.default_rng(11)
        # vpMatched on entry: the list positions are no map points of the list, so any value other than -1 stands for one (here -5)
        entry = np.where(p["kf"]["state"] != 0, -5, -1).astype(np.int32)
        kf2 = dict(p["kf"], state=rng.choice([0, 1, 2], n_kp, p=[0.5, 0.3, 0.2]).astype(np.uint8))
        skip2 = (rng.random(n_pts) < 0.05).astype(np.uint8)
        fz = dict(p, mode="fuse", kf=kf2, skip=skip2, th=np.float32(4.0))
        files = dict(keys1=p["kf"]["keysUn"], desc1=p["kf"]["desc"], keys2=kf2["keysUn"], desc2=kf2["desc"], state2=kf2["state"], matched=entry, scw1=p["Scw"], scw2=fz["Scw"], Xw=p["pts"]["Xw"],
                     normal=p["pts"]["normal"], pdesc=p["pts"]["desc"], maxD=p["pts"]["maxDistance"], minD=p["pts"]["minDistance"], skip1=p["skip"], skip2=skip2, scale=spc.SF)
        for name, a in files.items():
            np.ascontiguousarray(a).tofile(os.path.join(d, name + ".bin"))
        with open(os.path.join(d, "meta.txt"), "w") as f:
            for k, v in dict(fx=spc.CAM[0], fy=spc.CAM[1], cx=spc.CAM[2], cy=spc.CAM[3], minX=spc.BOUNDS[0], minY=spc.BOUNDS[1], maxX=spc.BOUNDS[2], maxY=spc.BOUNDS[3],
                             logScaleFactor=spc.LOG_SF).items():
                f.write("%s %r\n" % (k, float(v)))
        r = subprocess.run([prog, d], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.split("\n")
        m_ref, n_ref = spc.run_problem(p)
        after_ref = np.where(m_ref >= 0, m_ref, entry)
        total = int((after_ref != -1).sum())
        assert lines[:3] == ["nmatches %d" % n_ref, "nTotalMatches %d" % total, "accept %d" % (total >= 40)], (tag, lines[:3])
        decisions.append(total >= 40)
        after = np.array([int(l.split()[2]) for l in lines if l.startswith("m ")], np.int32)
        assert np.array_equal(after, after_ref)
        fk_ref, rep_ref, nf_ref = spc.run_problem(fz)
        assert "nFused %d" % nf_ref in lines and nf_ref > 10
        rl = np.array([[int(v) for v in l.split()[2:4]] for l in lines if l.startswith("r ")], np.int32).reshape(-1, 2)
        assert np.array_equal(rl[:, 0], np.where(rep_ref == spc.FUSE_ADDED, -1, rep_ref))       # vpReplacePoint: NULL where the point was added
        assert np.array_equal(rl[:, 1], np.where(rep_ref == spc.FUSE_ADDED, fk_ref, -1))        # the added observations
    assert decisions == [True, False]
