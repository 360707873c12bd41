"""GPU: the relocalisation projection operator (include/oslam_hip.h, "Relocalisation projection") against the sequential numpy restatement of
tests/reloc_project_common.py — every output entry and every count, no tolerance — against hand-written answers and against the truth of generated problems."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reloc_project_common as rpc
from object_slam_amd import reloc_project   # (at import: every test of this file needs the operator's module)
from object_slam_amd._lib import check, ptr
from object_slam_amd.matcher import Camera

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "object_slam_amd")
FILL = -77   # the pattern the output rows hold before a call
GAP = 5      # output rows between the problems that no problem owns


def _pack(problems, gap=GAP):
    """the records of a batch; the matched rows of problem j start `gap` rows after those of problem j - 1 end, so that some rows belong to no problem"""
    fr, pts, skip, kp_off, pt_off = rpc.concat_batch(problems)
    n = len(problems)
    kp_out = kp_off + gap * (1 + np.arange(n, dtype=np.int32))
    pr = reloc_project.pack_problems([len(p["frame"]["has_mp"]) for p in problems], kp_off, [len(p["skip"]) for p in problems], pt_off,
                                     np.stack([p["Tcw"] for p in problems]).reshape(n, 4, 4), [p["th"] for p in problems], [p["orb_dist"] for p in problems], kp_out, pt_off)
    return pr, fr, pts, skip, len(fr["has_mp"]) + gap * (n + 1)


def _call(proj, pr, fr, pts, skip, n_kp_out, check_ori=True, device=False):
    """the raw outputs of one call, over FILL: (matched, n_matches, n_removed, n_passes)"""
    n = len(pr)
    out = proj.search_batch(pr, fr, pts, rpc.CAM, rpc.BOUNDS, rpc.SF, rpc.LOG_SF, check_orientation=check_ori, skip=skip, matched=np.full(n_kp_out, FILL, np.int32),
                            n_matches=np.full(n, FILL, np.int32), n_removed=np.full(n, FILL, np.int32), n_passes=np.full(n, FILL, np.int32), n_pt_out=len(skip), n_kp_out=n_kp_out,
                            device=device)
    return out["matched"], out["n_matches"], out["n_removed"], out["n_passes"]


def _split(pr, raw):
    """per problem, in run_problem's form with the passes appended: (matched, n, removed, passes)"""
    return [(raw[0][o:o + n].copy(), int(c), int(r), int(q)) for o, n, c, r, q in zip(pr["kp_out_off"], pr["n_kp"], raw[1], raw[2], raw[3])]


def _run(proj, problems, check_ori=True, device=False):
    pr, fr, pts, skip, n_kp_out = _pack(problems)
    return _split(pr, _call(proj, pr, fr, pts, skip, n_kp_out, check_ori, device))


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and tuple(x[1:]) == tuple(y[1:]) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def proj():
    m = reloc_project.RelocProjector(64, 2400, 20000)
    yield m
    m.close()


@pytest.fixture(scope="module")
def batches():
    """check_orientation -> the problems of one call and the restatement's answers.  True: six generated problems, one at the 2400-keypoint capacity, n_pts = 0,
    n_kp = 0, both, and the hand cases that check the orientation.  False: the other hand cases and three generated problems with the check switched off."""
    every = rpc.batch_problems()
    on = [p for p in every if p["check_ori"]]
    off = [p for p in every if not p["check_ori"]] + [dict(p, name=p["name"] + "_no_ori", check_ori=False) for p in every[:3]]
    assert [p["name"] for p in on[:rpc.N_GENERATED]] == [p["name"] for p in every[:rpc.N_GENERATED]] and len(off) >= 4
    return {True: dict(problems=on, ref=[r for r, _ in rpc.reference_of(on, "gpu_on")]), False: dict(problems=off, ref=[r for r, _ in rpc.reference_of(off, "gpu_off")])}


@pytest.fixture(scope="module")
def first(proj, batches):
    out = {}
    for ori, b in batches.items():
        pr, fr, pts, skip, n_kp_out = _pack(b["problems"])
        raw = _call(proj, pr, fr, pts, skip, n_kp_out, ori)
        out[ori] = dict(pr=pr, raw=raw, res=_split(pr, raw))
    return out


def test_parity_with_the_restatement(batches, first):
    bad = []
    for ori, b in batches.items():
        for p, ref, got in zip(b["problems"], b["ref"], first[ori]["res"]):
            ndiff = int((got[0] != ref[0]).sum())
            print("ori %d %-28s n_kp %4d n_pts %4d count %4d (restatement %4d) removed %3d (%3d), entries that differ: %d, passes %d" % (
                ori, p["name"], len(p["frame"]["has_mp"]), len(p["skip"]), got[1], ref[1], got[2], ref[2], ndiff, got[3]))
            if ndiff or got[1] != ref[1] or got[2] != ref[2]:
                bad.append((ori, p["name"], ndiff, got[1:3], ref[1:]))
            # slot i is final after pass i + 1, and one more pass sees that nothing changed; a refused pose takes none
            assert (got[3] == 0) if ref[1] < 0 else (1 <= got[3] <= len(p["skip"]) + 1), (p["name"], got[3])
    assert not bad, bad
    res, g = first[True]["res"], rpc.N_GENERATED
    assert res[g - 1][1] > 500 and [r[1] for r in res[g:g + 3]] == [0, 0, 0] and [r[3] for r in res[g:g + 3]] == [1, 1, 1]
    assert all(r[1] >= 20 and r[2] > 0 and r[3] >= 3 for r in res[:g])
    # without the orientation check nothing is removed, and the claims are those of the call with the check
    for j, r in enumerate(first[False]["res"][-3:]):
        with_check = first[True]["res"][j]
        assert r[2] == 0 and r[1] == with_check[1] + with_check[2] and np.array_equal(r[0][with_check[0] >= 0], with_check[0][with_check[0] >= 0])


def test_rows_no_problem_owns_keep_their_fill(first):
    for ori, f in first.items():
        owned = np.zeros(len(f["raw"][0]), bool)
        for o, n in zip(f["pr"]["kp_out_off"], f["pr"]["n_kp"]):
            assert not owned[o:o + n].any()
            owned[o:o + n] = True
        assert (~owned).sum() >= GAP * len(f["pr"]) and (f["raw"][0][~owned] == FILL).all() and (f["raw"][0][owned] != FILL).all()


def test_hand_built_cases_give_their_known_answers(batches, first):
    seen = 0
    for ori, b in batches.items():
        for p, got in zip(b["problems"], first[ori]["res"]):
            if "expect" not in p:
                continue
            e = p["expect"]
            seen += 1
            assert got[0].tolist() == list(e["matched"]) and got[1] == e["n"] and got[2] == e["removed"], p["name"]
    assert seen == len(rpc.hand_cases())
    # the chains took a pass per link, also the one in windows beyond the candidate cache
    names = [p["name"] for p in batches[True]["problems"]]
    res = first[True]["res"]
    assert res[names.index("big_window")][3] >= rpc.CACHE_CASE_CANDIDATES and res[names.index("chain")][3] >= 5


def test_kernel_recovers_the_truth(batches, first):
    for p, got in zip(batches[True]["problems"][:rpc.N_GENERATED], first[True]["res"]):
        want, found, false = rpc.truth_score(p, got)
        assert want >= 100 and found * 10 >= want * 9 and false <= 2, (p["name"], want, found, false)


def test_problems_are_independent(proj, batches, first):
    for ori, b in batches.items():
        problems, res = b["problems"], first[ori]["res"]
        assert _same(_run(proj, problems[::-1], ori)[::-1], res)
        rng = np.random.default_rng(3)
        order = rng.permutation(len(problems))
        permuted = _run(proj, [problems[j] for j in order], ori)
        assert _same(permuted, [res[j] for j in order])
        for j in list(range(0, min(rpc.N_GENERATED, len(problems)), 3)) + list(range(rpc.N_GENERATED, len(problems))):
            assert _same(_run(proj, [problems[j]], ori), [res[j]]), problems[j]["name"]


def test_host_and_device_entry_points_agree_and_calls_repeat(proj, batches, first):
    for ori, b in batches.items():
        assert _same(_run(proj, b["problems"], ori, device=True), first[ori]["res"])
        assert _same(_run(proj, b["problems"], ori), first[ori]["res"])
        # one problem without keypoints and slots: no rows at all, so on the device path every array is an empty one, which gets a placeholder address
        empty = [dict(b["problems"][0], name="no_rows", frame=rpc.empty_frame(0), pts=rpc.empty_pts(0), skip=np.zeros(0, np.uint8))]
        host = _run(proj, empty, ori)
        assert len(host) == 1 and host[0][1:] == (0, 0, 1) and len(host[0][0]) == 0
        assert _same(_run(proj, empty, ori, device=True), host)


def test_optional_arrays_may_be_left_out(proj, batches):
    """skip, n_removed and n_passes NULL at the C ABI: nothing is skipped, and the other outputs are those of the restatement"""
    pr, fr, pts, skip, n_kp_out = _pack(batches[True]["problems"][:2])
    matched, n_matches = np.full(n_kp_out, FILL, np.int32), np.full(2, FILL, np.int32)
    frp, ptp = reloc_project.pack_frame_rows(fr), reloc_project.pack_pt_rows(pts)
    rf = reloc_project.FrameRows(len(frp["has_mp"]), *[ptr(frp[k]) for k in reloc_project.FRAME_KEYS])
    rp = reloc_project.PtRows(len(ptp["Xw"]), *[ptr(ptp[k]) for k in reloc_project.PT_KEYS])
    cam, bnd, sf = Camera(*rpc.CAM, 0.0, 0.0), np.array(rpc.BOUNDS, np.float32), np.ascontiguousarray(rpc.SF, np.float32)
    check(proj.L.oslam_match_search_by_projection_reloc_batch(proj.h, 2, ptr(pr), C.byref(rf), C.byref(rp), len(skip), None, n_kp_out, C.addressof(cam), ptr(bnd), ptr(sf), len(sf),
                                                              float(rpc.LOG_SF), 1, ptr(matched), ptr(n_matches), None, None))
    no_skip = [dict(p, skip=np.zeros_like(p["skip"])) for p in batches[True]["problems"][:2]]
    want = [rpc.run_problem(p) for p in no_skip]
    assert [np.array_equal(matched[o:o + n], w[0]) and c == w[1] for o, n, c, w in zip(pr["kp_out_off"], pr["n_kp"], n_matches, want)] == [True, True]
    assert any(not np.array_equal(w[0], r[0]) for w, r in zip(want, batches[True]["ref"][:2]))   # (the skip bytes mattered)


def test_refusals(proj, batches, first):
    from object_slam_amd._lib import OSLAM_E_CAPACITY, OSLAM_E_INVALID, OslamError
    problems, res = batches[True]["problems"][:3], first[True]["res"]
    pr, fr, pts, skip, n_kp_out = _pack(problems)
    n_pts_total, n_rows = len(skip), len(fr["has_mp"])

    def neighbours_ok(raw, what):
        for j in (0, 2):
            assert _same([_split(pr, raw)[j]], [res[j]]), what

    with pytest.raises(OslamError) as ei:
        reloc_project.RelocProjector(4, 2401, 1000)
    assert ei.value.code == OSLAM_E_INVALID
    small, few = reloc_project.RelocProjector(2, 360, 20000), reloc_project.RelocProjector(4, 2400, n_pts_total - 1)
    try:
        def refused(what, m, recs, code, device=False):
            """the call raises `code` and leaves every output row as it was"""
            outs = [np.full(n_kp_out, FILL, np.int32)] + [np.full(len(recs), FILL, np.int32) for _ in range(3)]
            with pytest.raises(OslamError) as ei:
                m.search_batch(recs, fr, pts, rpc.CAM, rpc.BOUNDS, rpc.SF, rpc.LOG_SF, skip=skip, matched=outs[0], n_matches=outs[1], n_removed=outs[2], n_passes=outs[3],
                               n_pt_out=n_pts_total, n_kp_out=n_kp_out, device=device)
            assert ei.value.code == code, what
            assert all((a == FILL).all() for a in outs), what

        def with_field(field, value):
            recs = pr.copy()
            recs[field][1] = value
            return recs

        refused("three problems, two allowed", small, pr, OSLAM_E_CAPACITY)
        refused("300 .. 400 keypoints, 360 allowed", small, pr[1:3], OSLAM_E_CAPACITY)
        refused("more point rows than max_points_total", few, pr, OSLAM_E_CAPACITY)
        for field in ("n_kp", "n_pts"):
            refused("negative " + field, proj, with_field(field, -1), OSLAM_E_CAPACITY)
        for field, value in (("kp_off", n_rows), ("pt_off", n_pts_total), ("pt_out_off", n_pts_total), ("kp_out_off", n_kp_out)):
            refused(field + " outside", proj, with_field(field, value), OSLAM_E_INVALID)
        for value in (256, -1, 1 << 20):
            refused("ORBdist %d" % value, proj, with_field("ORBdist", value), OSLAM_E_INVALID)
        # the device entry point cannot read the records: what the call as a whole exceeds is refused, a record that does not fit gets -2 and nothing else
        refused("problems, device", small, pr, OSLAM_E_CAPACITY, device=True)
        refused("point rows, device", few, pr, OSLAM_E_CAPACITY, device=True)
    finally:
        small.close()
        few.close()
    for field, value in (("n_kp", -1), ("n_pts", -1), ("n_kp", 2401), ("kp_off", n_rows), ("pt_off", n_pts_total), ("pt_out_off", n_pts_total), ("kp_out_off", n_kp_out), ("ORBdist", 256),
                         ("ORBdist", -1)):
        recs = pr.copy()
        recs[field][1] = value
        raw = _call(proj, recs, fr, pts, skip, n_kp_out, device=True)
        o, n = pr["kp_out_off"][1], pr["n_kp"][1]
        assert raw[1][1] == -2 and (raw[0][o:o + n] == FILL).all() and raw[2][1] == FILL and raw[3][1] == FILL, (field, value)
        neighbours_ok(raw, field)
    # ORBdist 0 and 255 are taken
    for value in (0, 255):
        recs = pr.copy()
        recs["ORBdist"][1] = value
        got = _split(pr, _call(proj, recs, fr, pts, skip, n_kp_out))[1]
        want = rpc.run_problem(dict(problems[1], orb_dist=value))
        assert np.array_equal(got[0], want[0]) and got[1:3] == want[1:], value
    # a Tcw that is not finite in one problem of three
    for what, index, value in (("NaN in the rotation", (1, 2), np.nan), ("inf in the translation", (0, 3), np.inf), ("-inf in row 2", (2, 0), -np.inf)):
        recs = pr.copy()
        recs["Tcw"][1][index] = value
        for device in (False, True):
            raw = _call(proj, recs, fr, pts, skip, n_kp_out, device=device)
            o, n = pr["kp_out_off"][1], pr["n_kp"][1]
            assert raw[1][1] == -1 and (raw[0][o:o + n] == -1).all() and raw[2][1] == 0 and raw[3][1] == 0, what
            neighbours_ok(raw, what)
    # row 3 of Tcw is not read
    recs = pr.copy()
    recs["Tcw"][1][3] = np.nan
    assert _same(_split(pr, _call(proj, recs, fr, pts, skip, n_kp_out)), res[:3])


def _ints(line):
    return np.array(line.split()[1:], np.int64)


def _bits(line):
    parts = line.split()
    return np.array([int(ch) for ch in parts[1]], np.uint8) if len(parts) > 1 else np.zeros(0, np.uint8)


def test_adapter_program_matches_the_restatement(tmp_path):
    from object_slam_amd import build
    build.build_hip()
    prog = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adapter_reloc_program.cc"), "-o", prog,
                           "-L", LIBDIR, "-loslam_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    for tag, (counts, n_searches, decision) in sorted(rpc.SCENARIOS.items()):
        s = rpc.make_scenario(17, *counts)
        d = str(tmp_path / tag)
        os.makedirs(d)
        files = dict(keys=s["frame"]["keysUn"], desc=s["frame"]["desc"], tcw=s["Tcw0"], mp=s["mp"], Xw=s["pts"]["Xw"], pdesc=s["pts"]["desc"], maxD=s["pts"]["maxDistance"],
                     minD=s["pts"]["minDistance"], angle=s["pts"]["kf_angle"], bad=s["bad"], scale=rpc.SF)
        for name, a in files.items():
            np.ascontiguousarray(a).tofile(os.path.join(d, name + ".bin"))
        with open(os.path.join(d, "meta.txt"), "w") as f:
            for k, v in dict(fx=rpc.CAM[0], fy=rpc.CAM[1], cx=rpc.CAM[2], cy=rpc.CAM[3], minX=rpc.BOUNDS[0], minY=rpc.BOUNDS[1], maxX=rpc.BOUNDS[2], maxY=rpc.BOUNDS[3],
                             logScaleFactor=rpc.LOG_SF).items():
                f.write("%s %r\n" % (k, float(v)))
        r = subprocess.run([prog, d], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = [l for l in r.stdout.split("\n") if l]
        print(tag, [l for l in lines if l.split()[0] in ("nGood", "search", "nadditional", "decision")])
        # every search, replayed by the restatement from the inputs the program printed
        at = [j for j, l in enumerate(lines) if l.startswith("search ")]
        n_slots = len(s["bad"])
        nadd = []
        for j in at:
            th, orb = float(lines[j].split()[1]), int(lines[j].split()[2])
            Tcw = np.array([float.fromhex(v) for v in lines[j + 1].split()[1:]], np.float32).reshape(4, 4)
            before, has_mp, skip = _ints(lines[j + 2]), _bits(lines[j + 3]), _bits(lines[j + 4])
            n, after = int(lines[j + 5].split()[1]), _ints(lines[j + 6])
            assert np.array_equal(has_mp, (before != -1).astype(np.uint8)) and len(skip) == n_slots
            held = set(before[before >= 0].tolist())
            assert all(skip[i] for i in held) and all(skip[i] for i in np.nonzero(s["bad"])[0])       # what the frame holds is in sFound
            m, n_ref, _ = rpc.search_by_projection(dict(s["frame"], has_mp=has_mp), s["pts"], skip, Tcw, th, orb)
            assert n == n_ref and np.array_equal(after, np.where(m >= 0, m, before)), (tag, th, orb, n, n_ref)
            nadd.append(n)
        # the inlier counts and the decision follow src/Tracking.cc:1707-1752
        good = [int(l.split()[1]) for l in lines if l.startswith("nGood ")]
        searches = [(float(lines[j].split()[1]), int(lines[j].split()[2])) for j in at]
        want_searches, want_good = [], 1
        nGood = good[0]
        if nGood >= 10 and nGood < 50:
            want_searches.append(rpc.COARSE)
            if nadd[0] + nGood >= 50:
                want_good += 1
                nGood = good[1]
                if 30 < nGood < 50:
                    want_searches.append(rpc.FINE)
                    if nGood + nadd[1] >= 50:
                        want_good += 1
                        nGood = good[2]
        assert searches == want_searches and len(good) == want_good and lines[-1] == "decision %d" % (nGood >= 50), (tag, good, searches, nadd)
        # ... and take the path the scenario was built for
        assert (len(searches), int(lines[-1].split()[1])) == (n_searches, decision), (tag, good, nadd)
        final = _ints(lines[-2])
        assert lines[-2].startswith("final") and len(final) == len(s["mp"]) and (final >= 0).sum() >= nGood
