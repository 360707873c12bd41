"""GPU: the batched OptimizeEssentialGraph operator (csrc/essential_graph.hip) against the numpy restatement of tests/essential_graph_common.py, which
test_essential_graph_cpu.py pins on the CPU: parity of status, Sim3s and SE3 poses, the Levenberg-Marquardt decisions on decisive trials, bit-identity
between calls, batch compositions and entry points, the refusals, point correction and the adapter program."""
import os
import subprocess

import numpy as np
import pytest

import essential_graph_common as egc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "object_slam_amd")
FILL_S, FILL_T, FILL_ST = -7.25, np.float32(-3.5), -77


@pytest.fixture(scope="module")
def eg():
    from object_slam_amd import essential_graph
    return essential_graph


@pytest.fixture(scope="module")
def opt(eg):
    h = eg.EssentialGraphOptimizer(64, 1024, 4096, 8192)
    yield h
    h.close()


@pytest.fixture(scope="module")
def batch():
    problems = egc.parity_problems()
    return dict(problems=problems, ref=egc.reference_of(problems, "parity"), rev=egc.reference_of(problems, "parity", "reversed"))


def _pack(eg, problems, extra_rows=0):
    arrays, n_kf, n_ed = egc.concat_batch(problems)
    pr = eg.pack_problems(n_kf, n_ed, [p["fix_scale"] for p in problems])
    if extra_rows:   # rows no problem owns, at the end of the per-keyframe arrays
        arrays["Scw"] = np.concatenate([arrays["Scw"], np.ones((extra_rows, 13), np.float32)])
        arrays["Snc"] = np.concatenate([arrays["Snc"], np.ones((extra_rows, 13), np.float32)])
        arrays["has_nc"] = np.concatenate([arrays["has_nc"], np.zeros(extra_rows, np.uint8)])
        arrays["fixed"] = np.concatenate([arrays["fixed"], np.zeros(extra_rows, np.uint8)])
    return pr, arrays


def _call(opt, pr, a, device=False, trace=False, row_first=None):
    N = len(a["fixed"])
    S, T, st = np.full((N, 13), FILL_S), np.full((N, 4, 4), FILL_T, np.float32), np.full((len(pr), 4), FILL_ST, np.int32)
    return opt.optimize_batch(pr, a["Scw"], a["Snc"], a["has_nc"], a["fixed"], a["edges"], Scw_out=S, Tcw_out=T, status=st, trace=trace, device=device, row_first=row_first)


def _split(pr, out):
    return [(out["status"][j].copy(), out["Scw"][p["kf_offset"]:p["kf_offset"] + p["n_kf"]].copy(), out["Tcw"][p["kf_offset"]:p["kf_offset"] + p["n_kf"]].copy()) for j, p in enumerate(pr)]


def _run(eg, opt, problems, device=False):
    pr, a = _pack(eg, problems)
    return _split(pr, _call(opt, pr, a, device))


def _same(a, b):
    return len(a) == len(b) and all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() and x[2].tobytes() == y[2].tobytes() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def first(eg, opt, batch):
    pr, a = _pack(eg, batch["problems"], extra_rows=3)
    out = _call(opt, pr, a, trace=True)
    return dict(pr=pr, arrays=a, out=out, res=_split(pr, out))


def _rel(a, b):
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()) if a.size else 0.0


def test_parity_with_the_restatement(batch, first):
    """status[0..2], every Scw_out and every Tcw_out within 1e-4 relative to max(1, |.|), no exclusions"""
    for p, r, rv, (st, S, T) in zip(batch["problems"], batch["ref"], batch["rev"], first["res"]):
        assert st[:3].tolist() == r["status"][:3].tolist(), p["name"]
        dS, dT = _rel(S, r["Scw"]), _rel(T.astype(np.float64), r["Tcw"].astype(np.float64))
        own = _rel(rv["Scw"], r["Scw"])
        print("%-22s status %s  |Scw - ref| %.3e  |Tcw - ref| %.3e  restatement forward vs reversed %.3e" % (p["name"], st.tolist(), dS, dT, own))
        assert dS <= 1e-4 and dT <= 1e-4, p["name"]


def test_lm_decisions_on_decisive_trials(batch, first):
    for j, (p, r, rv) in enumerate(zip(batch["problems"], batch["ref"], batch["rev"])):
        if not r["trace"]:
            continue
        dec = egc.decisive_trials(r, rv)
        n = int(first["out"]["trace_n"][j])
        tr = first["out"]["trace"][j, :n]
        compared = 0
        for k, d in enumerate(dec):
            if not d:
                continue
            assert k < n, (p["name"], k, n)
            assert tr[k, 4] == r["trace"][k][4], (p["name"], k, tr[k].tolist(), r["trace"][k])
            assert abs(tr[k, 3] - r["trace"][k][3]) <= 1e-9 * r["trace"][k][3], (p["name"], k, tr[k, 3], r["trace"][k][3])
            compared += 1
        print("%-22s trials %d (kernel %d), compared %d, excluded %d" % (p["name"], len(dec), n, compared, len(dec) - compared))
        if r["F0"] > 0:
            assert compared >= 1


def test_consistent_graph_returns_the_input_bits(batch, first):
    j = [p["name"] for p in batch["problems"]].index("consistent_6")
    p = batch["problems"][j]
    st, S, T = first["res"][j]
    assert st.tolist() == [0, 5, len(p["edges"]), 256 + 1]
    rec = p["Scw"].astype(np.float64)
    assert np.array_equal(S[:, :9], rec[:, 1:10]) and np.array_equal(S[:, 9:12], rec[:, 10:13]) and np.array_equal(S[:, 12], rec[:, 0])
    assert np.array_equal(T[:, :3, :3], p["Scw"][:, 1:10].reshape(-1, 3, 3)) and np.array_equal(T[:, :3, 3], p["Scw"][:, 10:13])
    assert first["out"]["trace"][j, 0, 2] == 0.0 and first["out"]["trace_n"][j] == 1


def test_unmoved_vertices_return_their_input(batch, first):
    """fixed vertices, and every vertex of a problem without edges: the record of the input Sim3, bit for bit"""
    for p, r, (st, S, T) in zip(batch["problems"], batch["ref"], first["res"]):
        fx = np.asarray(p["fixed"]) != 0
        if len(p["edges"]) == 0:
            fx[:] = True
        g = egc.sims_from_floats(p["Scw"])
        for k in np.nonzero(fx)[0]:
            assert S[k].tobytes() == egc.record(g[k]).tobytes() and T[k].tobytes() == egc.tcw_of(g[k]).tobytes(), (p["name"], k)


def test_problems_are_independent_and_calls_repeat(eg, opt, batch, first):
    problems, res = batch["problems"], first["res"]
    assert _same(_run(eg, opt, problems), res)   # a second call
    order = np.random.default_rng(5).permutation(len(problems))
    got = _run(eg, opt, [problems[j] for j in order])
    assert _same(got, [res[j] for j in order])
    for j in range(len(problems)):
        assert _same(_run(eg, opt, [problems[j]]), [res[j]]), problems[j]["name"]


def test_entry_points_agree_and_untouched_rows_keep_their_bytes(eg, opt, batch, first):
    pr, a = first["pr"], first["arrays"]
    dev = _call(opt, pr, a, device=True, trace=True)
    host = first["out"]
    for k in ("Scw", "Tcw", "status", "trace_n"):
        assert host[k].tobytes() == dev[k].tobytes(), k
    for j, n in enumerate(host["trace_n"]):
        assert host["trace"][j, :n].tobytes() == dev["trace"][j, :n].tobytes()
    assert (host["Scw"][-3:] == FILL_S).all() and (host["Tcw"][-3:] == FILL_T).all() and len(host["Scw"]) == int(pr["n_kf"].sum()) + 3
    zero = [p for p in batch["problems"] if p["name"] == "empty_0"]
    assert _same(_run(eg, opt, zero, device=True), _run(eg, opt, zero))


def test_refusals(eg, opt, batch, first):
    from object_slam_amd._lib import OSLAM_E_CAPACITY, OSLAM_E_INVALID, OslamError
    names = ("ring_3_2_fix", "ring_10_4_fix", "two_fixed")
    idx = [[p["name"] for p in batch["problems"]].index(n) for n in names]
    three = [batch["problems"][j] for j in idx]
    want = [first["res"][j] for j in idx]
    pr, a = _pack(eg, three)
    assert _same(_split(pr, _call(opt, pr, a)), want)
    N, E = len(a["fixed"]), len(a["edges"])
    _, blocks = eg.envelope(pr, a["fixed"], a["edges"])
    # each bound of the handle, the envelope's included (the host entry point computes the envelope; the device one checks the first three before it launches)
    for what, args, recs, both in (("problems", (2, N, E, int(blocks.sum())), pr, True), ("keyframes", (3, N - 1, E, int(blocks.sum())), pr, True),
                                   ("edges", (3, N, E - 1, int(blocks.sum())), pr, True), ("envelope", (3, N, E, int(blocks.sum()) - 1), pr, False)):
        small = eg.EssentialGraphOptimizer(*args)
        try:
            for device in ((False, True) if both else (False,)):
                S, T, st = np.full((N, 13), FILL_S), np.full((N, 4, 4), FILL_T, np.float32), np.full((3, 4), FILL_ST, np.int32)
                with pytest.raises(OslamError) as ei:
                    small.optimize_batch(recs, a["Scw"], a["Snc"], a["has_nc"], a["fixed"], a["edges"], Scw_out=S, Tcw_out=T, status=st, device=device)
                assert ei.value.code == OSLAM_E_CAPACITY, what
                assert (S == FILL_S).all() and (T == FILL_T).all() and (st == FILL_ST).all(), what
            if not both:   # the device entry point: the last problem's envelope does not fit the handle's storage: -2 for it alone
                got = _split(pr, _call(small, pr, a, device=True))
                assert got[2][0].tolist() == [-2, FILL_ST, FILL_ST, FILL_ST] and (got[2][1] == FILL_S).all() and (got[2][2] == FILL_T).all()
                assert _same(got[:2], want[:2])
        finally:
            small.close()

    def untouched(got):
        st, S, T = got
        return (S == FILL_S).all() and (T == FILL_T).all()
    # a record that does not lie inside the arrays: refused by the host entry point, -2 and nothing else from the device entry point
    dpr, row_first = eg.with_envelope(pr, a["fixed"], a["edges"])
    for field, value in (("n_kf", -1), ("kf_offset", -1), ("kf_offset", N - 9), ("n_kf", N + 1), ("n_edges", -1), ("edge_offset", E - 3), ("env_blocks", 3), ("env_offset", 1 << 30)):
        recs = pr.copy()
        recs[field][1] = value
        if not field.startswith("env"):
            with pytest.raises(OslamError) as ei:
                _call(opt, recs, a)
            assert ei.value.code == OSLAM_E_INVALID, field
        drecs = dpr.copy()
        drecs[field][1] = value
        got = _split(pr, _call(opt, drecs, a, device=True, row_first=row_first))
        assert got[1][0].tolist() == [-2, FILL_ST, FILL_ST, FILL_ST] and untouched(got[1]), (field, value)
        assert _same([got[0], got[2]], [want[0], want[2]]), field
    # a row_first that leaves an edge outside the envelope
    rf = row_first.copy()
    o = pr["kf_offset"][1]
    rf[o:o + 10] = np.arange(10)
    got = _split(pr, _call(opt, dpr, a, device=True, row_first=rf))
    assert got[1][0][0] == -2 and untouched(got[1]) and _same([got[0], got[2]], [want[0], want[2]])

    # each kind of invalid input in one problem of three
    def poison(field, row, col, value):
        arr = {k: v.copy() for k, v in a.items()}
        arr[field].reshape(len(arr[field]), -1)[row, col] = value
        return arr
    o, eo = int(pr["kf_offset"][1]), int(pr["edge_offset"][1])
    no_fixed = {k: v.copy() for k, v in a.items()}
    no_fixed["fixed"][o:o + 10] = 0
    snc_nan_unread = poison("Snc", o + 2, 4, np.nan)   # has_noncorrected is 0 there: not read, not invalid
    assert _same(_split(pr, _call(opt, pr, snc_nan_unread)), want)
    cases = [("s NaN", poison("Scw", o + 4, 0, np.nan)), ("s 0", poison("Scw", o + 4, 0, 0.0)), ("s < 0", poison("Scw", o + 4, 0, -1.0)), ("R inf", poison("Scw", o + 3, 5, np.inf)),
             ("t -inf", poison("Scw", o + 9, 12, -np.inf)), ("Snc NaN", poison("Snc", o + 9, 3, np.nan)), ("Snc s 0", poison("Snc", o + 9, 0, 0.0)),
             ("i == j", poison("edges", eo + 2, 1, a["edges"][eo + 2, 0])), ("index < 0", poison("edges", eo + 2, 0, -1)), ("index >= n_kf", poison("edges", eo + 2, 1, 10)),
             ("kind 2", poison("edges", eo + 2, 2, 2)), ("no fixed vertex", no_fixed)]
    for what, arr in cases:
        for device in (False, True):
            got = _split(pr, _call(opt, pr, arr, device))
            assert got[1][0].tolist() == [-1, 0, int(pr["n_edges"][1]), 0] and untouched(got[1]), what
            assert _same([got[0], got[2]], [want[0], want[2]]), what


def test_point_correction(eg, opt, batch, first):
    """float output of an fp64 map: 1e-6 relative to max(1, |.|); skipped points keep their bytes"""
    pr, a, out = first["pr"], first["arrays"], first["out"]
    rng = np.random.default_rng(3)
    pp, ref, P = [], [], []
    for j, p in enumerate(pr):
        m = 0 if p["n_kf"] == 0 else 40
        pp += [j] * m
        ref += list(rng.integers(-1, p["n_kf"], m)) if m else []
        P.append(rng.uniform(-5, 5, (m, 3)))
    pp, ref, P = np.array(pp, np.int32), np.array(ref, np.int32), np.concatenate(P).astype(np.float32)
    assert (ref < 0).any()
    st = out["status"].copy()
    bad = [p["name"] for p in batch["problems"]].index("ring_9_3_fix")
    st[bad, 0] = -1   # as if that problem had been invalid: its points are skipped
    fill = np.full_like(P, FILL_T)
    got = opt.correct_points(pr, a["Scw"], out["Scw"], st, pp, ref, P, P_out=fill.copy())
    dev = opt.correct_points(pr, a["Scw"], out["Scw"], st, pp, ref, P, P_out=fill.copy(), device=True)
    assert got.tobytes() == dev.tobytes()
    worst = 0.0
    for j, p in enumerate(pr):
        sel = pp == j
        o, n = p["kf_offset"], p["n_kf"]
        if j == bad:
            assert (got[sel] == FILL_T).all()
            continue
        want = egc.correct_points(a["Scw"][o:o + n], out["Scw"][o:o + n], ref[sel], P[sel], P_out=fill[sel])
        skipped = ref[sel] < 0
        assert (got[sel][skipped] == FILL_T).all()
        worst = max(worst, _rel(got[sel].astype(np.float64), want.astype(np.float64)))
    print("point correction: largest relative difference %.3e" % worst)
    assert worst <= 1e-6


def test_adapter_program_equals_the_ctypes_path(eg, tmp_path):
    from object_slam_amd import build
    build.build_hip()
    prog = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adapter_essential_graph_program.cc"), "-o", prog,
                           "-L", LIBDIR, "-loslam_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    tok = {}
    for l in r.stdout.split("\n"):
        if l:
            tok.setdefault(l.split()[0], []).append(l.split()[1:])
    edges = np.array(tok["edge"], np.int32).reshape(-1, 3)
    n = int(tok["nKF"][0][0])
    hexf = lambda rows, dt: np.array([[int(v, 16) for v in row] for row in rows], np.uint64).astype(dt)
    Scw = hexf(tok["Scw"], np.uint32).view(np.float32).reshape(n, 13)
    Snc = hexf(tok["Snc"], np.uint32).view(np.float32).reshape(n, 13)
    has_nc, fixed = np.array(tok["has_nc"][0], np.uint8), np.array(tok["fixed"][0], np.uint8)
    Tcw = hexf(tok["Tcw"], np.uint32).view(np.float32).reshape(n, 4, 4)
    P_in, P_out = hexf(tok["Pin"], np.uint32).view(np.float32).reshape(-1, 3), hexf(tok["Pout"], np.uint32).view(np.float32).reshape(-1, 3)
    ref = np.array(tok["ref"][0], np.int32)
    # the helper's edges equal the Python helper's on the same map (the program prints its map)
    parent = np.array(tok["parent"][0], np.int32)
    lists = lambda key: [[int(v) for v in row[1:]] for row in tok[key]]
    conn = {int(row[0]): [int(v) for v in row[1::2]] for row in tok.get("conn", [])}
    wts = {(int(row[0]), int(row[1 + 2 * k])): int(row[2 + 2 * k]) for row in tok.get("conn", []) for k in range((len(row) - 1) // 2)}
    cur, loop = int(tok["cur"][0][0]), int(tok["loop"][0][0])
    mine = eg.essential_graph_edges(parent, lists("children"), lists("loops"), lists("covis"), conn, cur, loop, weight=lambda i, j: wts[(i, j)])
    assert np.array_equal(mine, edges) and len(edges) > n
    fix_scale = int(tok["fixScale"][0][0])
    h = eg.EssentialGraphOptimizer(1, n, len(edges), 4096)
    try:
        pr = eg.pack_problems([n], [len(edges)], [fix_scale])
        out = h.optimize_batch(pr, Scw, Snc, has_nc, fixed, edges)
        assert out["status"][0, 0] == 0 and out["status"][0, 3] > 256
        assert out["Tcw"].tobytes() == Tcw.tobytes()
        want = h.correct_points(pr, Scw, out["Scw"], out["status"], np.zeros(len(ref), np.int32), ref, P_in, P_out=P_in.copy())
        assert want.tobytes() == P_out.tobytes() and (ref < 0).any() and not np.array_equal(P_in, P_out)
    finally:
        h.close()
