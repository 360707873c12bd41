"""GPU: k_triangulate (through oslam_mp_triangulate and oslam_mp_triangulate_pairs), svd4_last_row (through the SVD probe) and frustum_point (through its three entry
points) on the hand-built cases of tests/mappoint_common.py, against the numpy restatements there and the answers written in the tables.  Accept flags, counts,
unprojected positions and frustum records bit for bit; positions behind the DLT within the project's 1e-5 relative of the float64-SVD position.

Measured on an MI355X, svd4_last_row through the probe over svd_probe_set(): max angle x gap = 0.546 float epsilons (the oracle's transcription measures the same
0.546; the bound asserted is 4)."""
import ctypes as C

import numpy as np
import pytest

import mappoint_common as mc
from batch_common import dev, host, side_stream, vp
from object_slam_amd import QUERY_DTYPE, MapPointBatch
from object_slam_amd._lib import check, lib
from object_slam_amd.mappoint import TriKF, make_tri_kf

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
PAIRS = {c["name"]: c for c in mc.cached(mc.tri_cases)}
GENERAL = [n for n in PAIRS if PAIRS[n]["settings"] == "general"]
FRUSTUM = mc.cached(mc.frustum_cases)
FRAMES = mc.frustum_frames()
_ref, _single = {}, {}


def _u32(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def reference(name):
    """(ok, x3D, detail) of a pair from the restatement, computed once"""
    if name not in _ref:
        c, d = PAIRS[name], {}
        _ref[name] = mc.restate_triangulate(c["kf1"], c["kf2"], c["idx1"], c["idx2"], c["sf"], c["ls2"], c["rf"], detail=d, margins=False) + (d,)
    return _ref[name]


@pytest.fixture(scope="module")
def mp():
    m = MapPointBatch()
    yield m
    m.close()


def single(mp, name):
    """the pair through oslam_mp_triangulate, once"""
    if name not in _single:
        c = PAIRS[name]
        _single[name] = mp.triangulate(make_tri_kf(*c["kf1"]), [make_tri_kf(*c["kf2"])], [(c["idx1"], c["idx2"])], c["sf"], c["ls2"], c["rf"])      # asserts nnew == sum(ok)
    return _single[name]


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_triangulate_cases(mp, name):
    c = PAIRS[name]
    ok, x = single(mp, name)
    rok, rx, d = reference(name)
    wrong = [(n, int(a), code) for n, a, b, code in zip(c["names"], ok, rok, d["codes"]) if a != b]
    assert not wrong, wrong                                                            # (case, the kernel's flag, the gate the restatement decides at)
    assert np.array_equal(rok, c["ok"]) and d["codes"] == c["codes"]
    assert not x[ok == 0].any()                                                        # rejected rows are zero
    for m, n in enumerate(c["names"]):
        if d["codes"][m] in (mc.UNPROJECT1_OK, mc.UNPROJECT2_OK):
            assert np.array_equal(_u32(x[m]), _u32(rx[m])), (n, x[m], rx[m])
        elif d["codes"][m] == mc.DLT_OK:
            x64 = d["q32"][m]["X64"]
            rel = np.abs(x[m] - x64).max() / max(np.abs(x64).max(), 1e-3)
            assert rel <= 1e-5, (n, rel)


def _pairs_call(L, h, entries, settings):
    """entries: (kf1, kf2, idx1, idx2) per pair -> (ok, x3D) per pair through oslam_mp_triangulate_pairs, with a guard behind the outputs"""
    sf, ls2, rf = mc.SETTINGS[settings]
    kfs = [(make_tri_kf(*e[0]), make_tri_kf(*e[1])) for e in entries]                  # (struct, the arrays it points into) twice per pair
    k1 = (TriKF * len(entries))(*[a[0] for a, _ in kfs])
    k2 = (TriKF * len(entries))(*[b[0] for _, b in kfs])
    start = np.concatenate([[0], np.cumsum([len(e[2]) for e in entries])]).astype(np.int32)
    M, G = int(start[-1]), 5
    i1 = np.concatenate([e[2] for e in entries] + [np.zeros(1, np.int32)]).astype(np.int32)
    i2 = np.concatenate([e[3] for e in entries] + [np.zeros(1, np.int32)]).astype(np.int32)
    ok = np.full(M + G, 0xFF, np.uint8)
    x = np.full((M + G, 3), np.nan, f32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    check(L.oslam_mp_triangulate_pairs(h, len(entries), k1, k2, p(start), p(i1), p(i2), p(sf), p(ls2), len(sf), C.c_float(float(rf)), p(ok), p(x)))
    assert (ok[M:] == 0xFF).all() and np.isnan(x[M:]).all()                            # nothing behind [M]
    return [(ok[start[i]:start[i + 1]].copy(), x[start[i]:start[i + 1]].copy()) for i in range(len(entries))]


def _empty_kf(kf):
    """the keyframe without keypoints (n_kps == 0)"""
    return kf[:3] + tuple(a[:0] for a in kf[3:])


@pytest.mark.parametrize("M", [1, 127, 128, 129])
def test_triangulate_pairs_batches(mp, M):
    """The general cases as pairs of one launch, every pair with its own current keyframe, the rows repeated pair after pair up to M matches in all (the kernel's block
    is 128); the first pair, one in the middle and the last pair are empty, and one pair's keyframe 2 has no keypoints at all."""
    L = lib()
    entries, src, left, k = [], [], M, 0
    while left:
        c = PAIRS[GENERAL[k % len(GENERAL)]]
        n = min(left, len(c["idx1"]))
        entries.append((c["kf1"], c["kf2"], c["idx1"][:n], c["idx2"][:n]))
        src.append((c["name"], n))
        left -= n
        k += 1
    none = np.zeros(0, np.int32)
    far, near = PAIRS["far"], PAIRS["near"]
    entries.insert(0, (near["kf1"], far["kf2"], none, none))
    src.insert(0, None)
    mid = len(entries) // 2 + 1
    entries[mid:mid] = [(far["kf1"], near["kf2"], none, none), (near["kf1"], _empty_kf(near["kf2"]), none, none)]
    src[mid:mid] = [None, None]
    entries.append((far["kf1"], far["kf2"], none, none))
    src.append(None)
    assert sum(len(e[2]) for e in entries) == M and not len(entries[0][2]) and not len(entries[-1][2]) and not len(entries[mid][2]) and len(entries[mid + 1][1][3]) == 0
    h = C.c_void_p()
    check(L.oslam_mappoint_create(C.byref(h), 0))
    got = _pairs_call(L, h, entries, "general")
    rev = _pairs_call(L, h, entries[::-1], "general")[::-1]
    L.oslam_mappoint_destroy(h)
    for (ok, x), (rok, rx), s in zip(got, rev, src):
        if s is None:
            assert len(ok) == 0
            continue
        sok, sx = single(mp, s[0])
        assert np.array_equal(ok, sok[:s[1]]) and np.array_equal(_u32(x), _u32(sx[:s[1]])), s       # the single-keyframe entry point's bits
        assert np.array_equal(rok, ok) and np.array_equal(_u32(rx), _u32(x)), s                    # wherever the pair sits in the batch
        assert np.array_equal(ok, PAIRS[s[0]]["ok"][:s[1]]), s


@pytest.mark.parametrize("settings", ["dyadic", "probe"])
def test_triangulate_pairs_other_settings(mp, settings):
    L = lib()
    names = [n for n in PAIRS if PAIRS[n]["settings"] == settings]
    h = C.c_void_p()
    check(L.oslam_mappoint_create(C.byref(h), 0))
    got = _pairs_call(L, h, [(PAIRS[n]["kf1"], PAIRS[n]["kf2"], PAIRS[n]["idx1"], PAIRS[n]["idx2"]) for n in names], settings)
    L.oslam_mappoint_destroy(h)
    for n, (ok, x) in zip(names, got):
        sok, sx = single(mp, n)
        assert np.array_equal(ok, sok) and np.array_equal(_u32(x), _u32(sx)) and np.array_equal(ok, PAIRS[n]["ok"]), n


# ---- svd4_last_row ---------------------------------------------------------------------------------------------------------------------------------
def test_svd_probe():
    """svd4_last_row against numpy's float64 SVD of the same float matrices, through the operator: one pair per matrix in one launch.  The bound, 4 float epsilons of
    angle x gap, is the oracle's measured 0.39 with room for the device's 1-ulp hypot inside the rotations; a larger value is a finding."""
    L = lib()
    A, v, gap = mc.cached(mc.svd_probe_set)
    exact = sorted(mc.SVD_EXACT)
    probs = [mc.svd_probe_problem(a) for a in A] + [mc.svd_probe_problem(mc.SVD_EXACT[n][0]) for n in exact]
    h = C.c_void_p()
    check(L.oslam_mappoint_create(C.byref(h), 0))
    got = _pairs_call(L, h, [(p["kf1"], p["kf2"], p["idx1"], p["idx2"]) for p in probs], "probe")
    L.oslam_mappoint_destroy(h)
    worst = 0.0
    for (ok, x), vv, g in zip(got, v, gap):
        assert ok[0] == 1                                                              # the probe's other gates are open
        worst = max(worst, mc.angle_gap(x[0], vv, g))
    print("svd4_last_row through the probe: max angle x gap = %.3f float epsilons over %d matrices" % (worst, len(A)))
    assert worst <= 4.0, worst
    for n, (ok, x) in zip(exact, got[len(A):]):
        _, want_ok, want_x = mc.SVD_EXACT[n]
        assert ok[0] == want_ok and np.array_equal(_u32(x[0]), _u32(want_x)), (n, ok, x)


# ---- frustum_point ---------------------------------------------------------------------------------------------------------------------------------
def _frustum_ref(frame):
    _, Tcw, th, rows, Pw = frame
    return mc.restate_frustum(*mc.frustum_args(FRUSTUM, rows, Pw, Tcw, th))


def _differs(names, got, want):
    return [(n, g, w) for n, g, w in zip(names, got, want) if g.tobytes() != w.tobytes()]


@pytest.mark.parametrize("k", range(len(FRAMES)), ids=[f[0] for f in FRAMES])
def test_frustum_cases_host_entry_point(mp, k):
    _, Tcw, th, rows, Pw = FRAMES[k]
    q = mp.isInFrustum(*mc.frustum_args(FRUSTUM, rows, Pw, Tcw, th)[:12], th=float(th))
    assert not _differs([FRUSTUM["names"][r] for r in rows], q, _frustum_ref(FRAMES[k]))
    if k == 0:
        assert [("IN_VIEW" if f & 1 else "out") for f in q["flags"]] == [("IN_VIEW" if c == mc.F_IN_VIEW else "out") for c in FRUSTUM["codes"]]


@pytest.mark.parametrize("resident", [False, True], ids=["batch_device", "batch_resident_device"])
def test_frustum_cases_batch_entry_points(resident):
    """The frames of frustum_frames() as one batch: another count, pose and th per frame, stride_in != stride_out and skip flags in the resident form."""
    import torch
    L = lib()
    B = len(FRAMES)
    SIN = 40
    SOUT = 36 if resident else SIN
    counts = [len(f[3]) for f in FRAMES]
    assert len(set(counts)) == B and max(counts) <= SOUT
    rng = np.random.default_rng(3)
    arr = dict(Pw=np.full((B, SIN, 3), 1e9, f32), Pn=np.zeros((B, SIN, 3), f32), maxD=np.ones((B, SIN), f32), minD=np.ones((B, SIN), f32), obs=np.zeros((B, SIN), np.uint8),
               desc=np.full((B, SIN, 32), 0xAB, np.uint8), skip=np.zeros((B, SOUT), np.uint8), Tcw=np.zeros((B, 16), f32), th=np.zeros(B, f32))
    for b, (_, Tcw, th, rows, Pw) in enumerate(FRAMES):
        n = len(rows)
        arr["Pw"][b, :n], arr["Pn"][b, :n], arr["maxD"][b, :n], arr["minD"][b, :n] = Pw, FRUSTUM["Pn"][rows], FRUSTUM["maxD"][rows], FRUSTUM["minD"][rows]
        arr["obs"][b, :n], arr["desc"][b, :n], arr["Tcw"][b], arr["th"][b] = FRUSTUM["obs"][rows], FRUSTUM["desc"][rows], Tcw.reshape(-1), th
        arr["skip"][b, :n] = rng.random(n) < 0.3
    D = {k: dev(a) for k, a in arr.items()}
    D["M"] = dev(np.array(counts, np.int32))
    out = torch.full((B + 2, SOUT, 64), 0xFF, dtype=torch.uint8, device="cuda")        # a guard row before and behind
    inv = torch.full((B + 2, SOUT), 0xFF, dtype=torch.uint8, device="cuda")
    stream = side_stream()
    s = C.c_void_p(stream.cuda_stream)
    sf = np.ascontiguousarray(mc.SF)
    pts = (vp(D["Pw"]), vp(D["Pn"]), vp(D["maxD"]), vp(D["minD"]), vp(D["obs"]), vp(D["desc"]))
    tail = (vp(D["Tcw"]), vp(D["th"]), (C.c_float * 5)(*[float(v) for v in mc.F_K5]), (C.c_float * 4)(*mc.F_BOUNDS), C.c_float(float(mc.F_COSLIMIT)), C.c_float(float(mc.F_LOGSF)),
            C.c_void_p(sf.ctypes.data), len(sf), vp(out, SOUT * 64), vp(inv, SOUT), s)
    if resident:
        check(L.oslam_frame_is_in_frustum_batch_resident_device(B, SIN, SOUT, vp(D["M"]), *pts, vp(D["skip"]), *tail))
    else:
        check(L.oslam_frame_is_in_frustum_batch_device(B, SIN, vp(D["M"]), *pts, *tail))
    stream.synchronize()
    q = host(out, QUERY_DTYPE, (B + 2, SOUT))
    iv = inv.cpu().numpy()
    sentinel = lambda a: bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())
    assert sentinel(q[0]) and sentinel(q[-1]) and sentinel(iv[0]) and sentinel(iv[-1])
    inactive = np.zeros(1, QUERY_DTYPE)
    inactive["minLevel"] = inactive["maxLevel"] = -1
    skipped_visible = 0
    for b, frame in enumerate(FRAMES):
        n = counts[b]
        want = _frustum_ref(frame)
        if resident:
            sk = arr["skip"][b, :n] != 0
            skipped_visible += int((want["flags"][sk] & 1).sum())
            want[sk] = inactive[0]                                                     # a skipped point: an inactive query, in_view 0
        assert not _differs([FRUSTUM["names"][r] for r in frame[3]], q[b + 1, :n], want), frame[0]
        assert np.array_equal(iv[b + 1, :n], (want["flags"] & 1).astype(np.uint8)), frame[0]
        assert sentinel(q[b + 1, n:]) and sentinel(iv[b + 1, n:])                      # entries beyond d_M[b] are left untouched
    assert not resident or skipped_visible >= 3                                        # skip flags really suppressed visible points
