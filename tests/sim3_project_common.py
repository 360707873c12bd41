"""A numpy restatement of ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (reference src/ORBmatcher.cc:290-403) and of ORBmatcher::Fuse(pKF,
Scw, vpPoints, th, vpReplacePoint) (:977-1100), written from the reference text with the roundings include/oslam_hip.h ("Sim3 projection") lists.  Both are
literally sequential: a Python loop over the points in list order that mutates vpMatched (the search) or the keyframe's map-point table (Fuse), as the
reference does; there is no fixpoint here.  Candidates come from a brute-force window test over all keypoints, put into KeyFrame::GetFeaturesInArea's
visiting order (cell column, cell row, keypoint index).

Also: hand-built problems with known answers written by hand, and a seeded generator of problems with known truth."""
import numpy as np

import sim3_match_common as smc
from object_slam_amd._lib import KP_DTYPE

f32, f64 = np.float32, np.float64
GRID_COLS, GRID_ROWS, TH_LOW = 64, 48, 50     # include/Frame.h:43-44, src/ORBmatcher.cc:37
CAM, BOUNDS, SF, LOG_SF, NLEVELS = smc.CAM, smc.BOUNDS, smc.SF, smc.LOG_SF, smc.NLEVELS
SEARCH_TH, FUSE_TH = 10.0, 4.0                # src/LoopClosing.cc:376, :600
FUSE_OCCUPANT, FUSE_ADDED = -2, -3            # OSLAM_FUSE_OCCUPANT, OSLAM_FUSE_ADDED
KF_KEYS = ("keysUn", "desc", "state")
PT_KEYS = ("Xw", "normal", "desc", "maxDistance", "minDistance")
_NULL, _GOOD, _BAD = -1, -2, -4               # the keyframe's map-point table of the Fuse restatement: no point, its own good point, its own bad point, or a list index


def decompose(Scw):
    """scw, Rcw, tcw, Ow (:299-303)"""
    S = np.asarray(Scw, f32).reshape(4, 4)
    with np.errstate(all="ignore"):
        scw = f32(np.sqrt((f64(S[0, 0]) * f64(S[0, 0]) + f64(S[0, 1]) * f64(S[0, 1])) + f64(S[0, 2]) * f64(S[0, 2])))
        inv = 1.0 / f64(scw)
        Rcw = (S[:3, :3].astype(f64) * inv).astype(f32)
        tcw = (S[:3, 3].astype(f64) * inv).astype(f32)
        Ow = np.array([-((Rcw[0, i] * tcw[0] + Rcw[1, i] * tcw[1]) + Rcw[2, i] * tcw[2]) for i in range(3)], f32)
    return scw, Rcw, tcw, Ow


def _gates(pts, skip, Rcw, tcw, Ow, cam, bounds, log_sf, nlevels):
    """:312-357 / :1000-1046 for all points at once: (passes every gate, u, v, predicted level)"""
    fx, fy, cx, cy = [f32(v) for v in cam]
    minX, minY, maxX, maxY = [f32(v) for v in bounds]
    X = np.asarray(pts["Xw"], f32).reshape(-1, 3)
    Pn = np.asarray(pts["normal"], f32).reshape(-1, 3)
    Pc = smc._gemm(Rcw, X, tcw)
    with np.errstate(all="ignore"):
        z = Pc[:, 2]
        invz = (1.0 / z.astype(f64)).astype(f32)
        u = fx * (Pc[:, 0] * invz) + cx
        v = fy * (Pc[:, 1] * invz) + cy
        PO = X - Ow[None, :]
        assert PO.dtype == f32 and u.dtype == f32
        P64 = PO.astype(f64)
        dist = np.sqrt((P64[:, 0] * P64[:, 0] + P64[:, 1] * P64[:, 1]) + P64[:, 2] * P64[:, 2]).astype(f32)
        maxDistance, minDistance = f32(1.2) * pts["maxDistance"].astype(f32), f32(0.8) * pts["minDistance"].astype(f32)
        N64 = Pn.astype(f64)
        dot = (P64[:, 0] * N64[:, 0] + P64[:, 1] * N64[:, 1]) + P64[:, 2] * N64[:, 2]
        ok = (np.asarray(skip) == 0) & ~(z < 0.0) & (u >= minX) & (u < maxX) & (v >= minY) & (v < maxY) & ~((dist < minDistance) | (dist > maxDistance)) & ~(dot < 0.5 * dist.astype(f64))
        ratio = pts["maxDistance"].astype(f32) / dist
        cl = np.ceil(np.log(ratio.astype(f64)).astype(f32) / f32(log_sf))
    assert ratio.dtype == f32 and cl.dtype == f32
    level = np.array([min(int(c) if 0 <= c < 2147483648.0 else 0, nlevels - 1) for c in cl], np.int32)   # (what does not fit an int is INT_MIN on x86: level 0)
    return ok, u, v, level


class _Window:
    """KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:569-608) of one keyframe: indices() gives vIndices in the reference's order"""

    def __init__(self, keys, bounds):
        self.minX, self.minY, maxX, maxY = [f32(v) for v in bounds]
        self.invW, self.invH = f32(GRID_COLS) / f32(maxX - self.minX), f32(GRID_ROWS) / f32(maxY - self.minY)
        n = len(keys)
        px, py = smc._grid_cells(keys, bounds, self.invW, self.invH)
        self.order = np.lexsort((np.arange(n), py, px))   # ix outer, iy inner, index inside a cell
        self.px, self.py = px[self.order], py[self.order]
        self.kx, self.ky = keys["x"].astype(f32)[self.order], keys["y"].astype(f32)[self.order]

    def indices(self, u, v, r):
        c0x = max(0, int(np.floor(((u - self.minX) - r) * self.invW)))
        c1x = min(GRID_COLS - 1, int(np.ceil(((u - self.minX) + r) * self.invW)))
        c0y = max(0, int(np.floor(((v - self.minY) - r) * self.invH)))
        c1y = min(GRID_ROWS - 1, int(np.ceil(((v - self.minY) + r) * self.invH)))
        if c0x >= GRID_COLS or c1x < 0 or c0y >= GRID_ROWS or c1y < 0:
            return np.zeros(0, np.int64)
        m = (self.px >= c0x) & (self.px <= c1x) & (self.py >= c0y) & (self.py <= c1y) & (np.abs(self.kx - u) < r) & (np.abs(self.ky - v) < r)
        return self.order[np.nonzero(m)[0]]


def _best(vIndices, usable, octave, level, kdesc, dMP, start):
    """the inner loop (:372-392 / :1062-1079): (bestDist, bestIdx)"""
    bestDist, bestIdx = start, -1
    for idx in vIndices:
        if not usable(idx):
            continue
        if octave[idx] < level - 1 or octave[idx] > level:
            continue
        d = int(smc._POP[np.bitwise_xor(kdesc[idx], dMP)].sum())
        if d < bestDist:
            bestDist, bestIdx = d, int(idx)
    return bestDist, bestIdx


def search_by_projection(kf, pts, skip, Scw, th, cam=CAM, bounds=BOUNDS, sf=SF, log_sf=LOG_SF):
    """(matched [n_kp] int32: the list index of the point the call wrote into vpMatched[idx], -1 where it wrote nothing; nmatches).  kf["state"] != 0: vpMatched[idx] is
    not NULL on entry.  (-1, all -1) for an Scw that is not finite or has no positive scale, as the operator declares."""
    n_kp, n_pts = len(kf["state"]), len(pts["maxDistance"])
    scw, Rcw, tcw, Ow = decompose(Scw)
    if not (np.isfinite(np.asarray(Scw, f32).reshape(4, 4)[:3]).all() and np.isfinite(scw) and scw > 0):
        return np.full(n_kp, -1, np.int32), -1
    vpMatched = np.where(np.asarray(kf["state"]) != 0, -2, -1).astype(np.int64)   # -1 NULL, -2 a point on entry, >= 0 list point
    nmatches = 0
    if n_pts and n_kp:
        ok, u, v, level = _gates(pts, skip, Rcw, tcw, Ow, cam, bounds, log_sf, len(sf))
        win = _Window(kf["keysUn"], bounds)
        octave = kf["keysUn"]["octave"]
        for iMP in range(n_pts):
            if not ok[iMP]:
                continue
            radius = f32(th) * sf[level[iMP]]
            vIndices = win.indices(u[iMP], v[iMP], radius)
            bestDist, bestIdx = _best(vIndices, lambda idx: vpMatched[idx] == -1, octave, level[iMP], kf["desc"], pts["desc"][iMP], 256)
            if bestDist <= TH_LOW:
                vpMatched[bestIdx] = iMP
                nmatches += 1
    return np.where(vpMatched >= 0, vpMatched, -1).astype(np.int32), nmatches


def fuse(kf, pts, skip, Scw, th, cam=CAM, bounds=BOUNDS, sf=SF, log_sf=LOG_SF):
    """(fused_kp [n_pts], replace [n_pts], nFused).  kf["state"]: 0 GetMapPoint(idx) is NULL, 1 a point that is not bad, 2 a bad one."""
    n_kp, n_pts = len(kf["state"]), len(pts["maxDistance"])
    fused_kp, replace = np.full(n_pts, -1, np.int32), np.full(n_pts, -1, np.int32)
    scw, Rcw, tcw, Ow = decompose(Scw)
    if not (np.isfinite(np.asarray(Scw, f32).reshape(4, 4)[:3]).all() and np.isfinite(scw) and scw > 0):
        return fused_kp, replace, -1
    table = np.array([{0: _NULL, 1: _GOOD, 2: _BAD}[int(s)] for s in kf["state"]], np.int64)
    nFused = 0
    if n_pts and n_kp:
        ok, u, v, level = _gates(pts, skip, Rcw, tcw, Ow, cam, bounds, log_sf, len(sf))
        win = _Window(kf["keysUn"], bounds)
        octave = kf["keysUn"]["octave"]
        for iMP in range(n_pts):
            if not ok[iMP]:
                continue
            radius = f32(th) * sf[level[iMP]]
            vIndices = win.indices(u[iMP], v[iMP], radius)
            bestDist, bestIdx = _best(vIndices, lambda idx: True, octave, level[iMP], kf["desc"], pts["desc"][iMP], 2147483647)
            if bestDist <= TH_LOW:
                pMPinKF = table[bestIdx]
                if pMPinKF != _NULL:
                    if pMPinKF != _BAD:   # (a list point that was added is never bad: bad points are skipped)
                        replace[iMP] = FUSE_OCCUPANT if pMPinKF == _GOOD else pMPinKF
                else:
                    table[bestIdx] = iMP   # AddObservation, AddMapPoint
                    replace[iMP] = FUSE_ADDED
                fused_kp[iMP] = bestIdx
                nFused += 1
    return fused_kp, replace, nFused


def run_problem(p):
    """search: (matched, nmatches); fuse: (fused_kp, replace, nFused)"""
    fn = fuse if p["mode"] == "fuse" else search_by_projection
    return fn(p["kf"], p["pts"], p["skip"], p["Scw"], p["th"])


# ---------------------------------------------------------------------------------------------------------------------------------------------
def empty_kf(n=0):
    return dict(keysUn=np.zeros(n, KP_DTYPE), desc=np.zeros((n, 32), np.uint8), state=np.zeros(n, np.uint8))


def empty_pts(n=0):
    return dict(Xw=np.zeros((n, 3), f32), normal=np.zeros((n, 3), f32), desc=np.zeros((n, 32), np.uint8), maxDistance=np.zeros(n, f32), minDistance=np.zeros(n, f32))


def scaled_pose(s, R=None, t=None):
    """Scw = [s R | s t; 0 1]"""
    S = np.eye(4, dtype=f32)
    S[:3, :3] = f32(s) * (np.eye(3, dtype=f32) if R is None else np.asarray(R, f32))
    S[:3, 3] = f32(s) * (np.zeros(3, f32) if t is None else np.asarray(t, f32))
    return S


def kpt(x, y, octave, desc, state=0):
    return dict(x=x, y=y, oct=octave, desc=desc, state=state)


def pt(u, v, desc, z=2.0, level=0, P=None, normal=(0.0, 0.0, 1.0), maxD=None, minD=None, skip=0, t=(0.0, 0.0, 0.0)):
    """a point that projects to (u, v) at depth z (camera frame = world frame shifted by t: Xw = P - t) and predicts `level`: mfMaxDistance = dist * 1.2^level * 0.999
    (the quotient of PredictScale is then a little below `level`, and ceil gives `level`).  The normal (0, 0, 1) passes the viewing-angle gate of every point
    inside the image of CAM (PO . Pn = z >= 0.5 dist)."""
    P = smc.point_at(u, v, z) if P is None else np.asarray(P, f32)
    d = smc.norm3(P)
    maxD = f32(d * SF[level] * f32(0.999)) if maxD is None else f32(maxD)
    minD = f32(maxD / SF[-1]) if minD is None else f32(minD)
    return dict(X=P - np.asarray(t, f32), n=np.asarray(normal, f32), desc=desc, maxD=maxD, minD=minD, skip=skip)


def _case(name, mode, kps, points, expect, th=None, Scw=None):
    kf, pts = empty_kf(len(kps)), empty_pts(len(points))
    for i, r in enumerate(kps):
        kf["keysUn"][i] = (r["x"], r["y"], 31.0, 0.0, 0.0, r["oct"], -1)
        kf["desc"][i], kf["state"][i] = r["desc"], r["state"]
    for i, r in enumerate(points):
        pts["Xw"][i], pts["normal"][i], pts["desc"][i], pts["maxDistance"][i], pts["minDistance"][i] = r["X"], r["n"], r["desc"], r["maxD"], r["minD"]
    th = (FUSE_TH if mode == "fuse" else SEARCH_TH) if th is None else th
    return dict(name=name, mode=mode, kf=kf, pts=pts, skip=np.array([r["skip"] for r in points], np.uint8), Scw=scaled_pose(1.0) if Scw is None else Scw, th=f32(th), expect=expect)


CACHE_CASE_CANDIDATES = 10   # candidates within TH_LOW in one window of the "big_window" case: more than the kernel's per-point cache holds (7)


def hand_cases():
    """Problems with known answers: dict(name, mode, kf, pts, skip, Scw, th, expect).  expect of a search: dict(matched [n_kp], n); of a Fuse: dict(fused_kp [n_pts],
    replace [n_pts], n).  Identity Scw unless stated, CAM, BOUNDS, 8 levels at 1.2: the cells are 10 x 10 pixels; the radius at level 0 is 10 (search) or 4 (Fuse)."""
    rng = np.random.default_rng(78)
    rd = lambda: rng.integers(0, 256, 32, dtype=np.uint8)
    fb = smc.flip_bits
    A, O = FUSE_ADDED, FUSE_OCCUPANT
    cases = []

    # a claim chain of four: keypoint j has D_j (pairwise 20 apart); point 0 has D_0, point j >= 1 is 6 from D_(j-1) and 14 from D_j.  Point 0 takes k0; point 1's
    # nearest is k0, claimed, so it takes k1; point 2's nearest is k1, claimed by then, so it takes k2; point 3 takes k3.  One pass without claims gives 0, 2, 3, -1.
    B = rd()
    D = [fb(B, range(20 * j, 20 * j + 10)) for j in range(4)]
    Q = [D[0]] + [fb(B, list(range(20 * (j - 1), 20 * (j - 1) + 10)) + list(range(20 * j, 20 * j + 6))) for j in range(1, 4)]
    cases.append(_case("chain", "search", [kpt(100 + j, 100, 0, D[j]) for j in range(4)], [pt(101.5, 100, Q[j]) for j in range(4)], dict(matched=[0, 1, 2, 3], n=4)))

    # the fallback of the later point is 51 away: it gets nothing
    B = rd()
    cases.append(_case("chain_fallback_51", "search", [kpt(300, 100, 0, B), kpt(301, 100, 0, fb(B, range(100, 157)))], [pt(300, 100, B), pt(300, 100, fb(B, range(100, 106)))],
                       dict(matched=[0, -1], n=1)))

    # a keypoint matched on entry is no candidate: the point takes the other one, 30 away
    B = rd()
    cases.append(_case("claimed_on_entry", "search", [kpt(100, 100, 0, B, state=1), kpt(103, 100, 0, fb(B, range(30)))], [pt(100, 100, B)], dict(matched=[-1, 0], n=1)))

    # a skipped point (bad, or already found) that would match exactly
    B, B2 = rd(), rd()
    cases.append(_case("skip", "search", [kpt(100, 100, 0, B), kpt(300, 100, 0, B2)], [pt(100, 100, B, skip=1), pt(300, 100, B2)], dict(matched=[-1, 1], n=1)))

    # a tie between equal distances in two cells: index order says keypoint 0, the traversal (cell column first) reaches keypoint 1 (cell 9, 11) before keypoint 0
    # (cell 11, 9); a row-first traversal would reach keypoint 0 first
    B = rd()
    cases.append(_case("tie", "search", [kpt(105.5, 94.5, 0, fb(B, range(0, 10))), kpt(94.5, 105.5, 0, fb(B, range(20, 30)))], [pt(100, 100, B)], dict(matched=[-1, 0], n=1)))
    # the same with Fuse's radius of 4 around (105, 105): keypoint 0 in cell (11, 10), keypoint 1 in cell (10, 11)
    cases.append(_case("tie_fuse", "fuse", [kpt(107.5, 102.5, 0, fb(B, range(0, 10))), kpt(102.5, 107.5, 0, fb(B, range(20, 30)))], [pt(105, 105, B)],
                       dict(fused_kp=[1], replace=[A], n=1)))

    # the octave gate at predicted level 3: 2 and 3 pass, 1 and 4 do not
    at = [(100, 100), (200, 100), (300, 100), (400, 100)]
    d = [rd() for _ in at]
    cases.append(_case("octave", "search", [kpt(x, y, o, d[j]) for j, ((x, y), o) in enumerate(zip(at, [1, 2, 3, 4]))], [pt(x, y, d[j], level=3) for j, (x, y) in enumerate(at)],
                       dict(matched=[-1, 1, 2, -1], n=2)))

    # TH_LOW: 50 accepted, 51 refused
    d = [rd(), rd()]
    for mode, exp in (("search", dict(matched=[0, -1], n=1)), ("fuse", dict(fused_kp=[0, -1], replace=[A, -1], n=1))):
        cases.append(_case("th_low_" + mode, mode, [kpt(100, 100, 0, d[0]), kpt(300, 100, 0, d[1])], [pt(100, 100, fb(d[0], range(50))), pt(300, 100, fb(d[1], range(51)))], exp))

    # depth: z < 0 is skipped (the point would project onto its keypoint); z == +0 projects to +inf or NaN, which IsInImage rejects; the last point is a control
    at = [(100, 100), (200, 100), (300, 100), (400, 100)]
    d = [rd() for _ in at]
    points = [pt(100, 100, d[0], P=smc.point_at(100, 100, -2.0), maxD=1e9, minD=0), pt(0, 0, d[1], P=[1.0, 0.5, 0.0], maxD=1e9, minD=0), pt(0, 0, d[2], P=[0.0, 0.0, 0.0], maxD=1e9, minD=0),
              pt(400, 100, d[3])]
    cases.append(_case("depth", "search", [kpt(x, y, 0, d[j]) for j, (x, y) in enumerate(at)], points, dict(matched=[-1, -1, -1, 3], n=1)))

    # IsInImage: u == mnMinX and v == mnMinY are inside, u == mnMaxX and v == mnMaxY are not (keypoints wait within the radius of all four)
    d = [rd() for _ in range(4)]
    kps = [kpt(2, 100, 0, d[0]), kpt(634, 200, 0, d[1]), kpt(300, 2, 0, d[2]), kpt(400, 474, 0, d[3])]
    points = [pt(0, 100, d[0]), pt(640, 200, d[1]), pt(300, 0, d[2]), pt(400, 480, d[3])]
    cases.append(_case("in_image", "search", kps, points, dict(matched=[0, -1, 2, -1], n=2)))

    # the distance gate with points on the optical axis (their norm is their depth, exactly): dist == 1.2f * maxD and dist == 0.8f * minD are kept, the next float
    # outside is dropped.  All keypoints sit at the principal point; the descriptors tell them apart.
    maxD, minD = f32(3.0), f32(5.0)
    far, near = f32(1.2) * maxD, f32(0.8) * minD
    d = [rd() for _ in range(4)]
    spec = [(far, maxD, f32(0), 0), (np.nextafter(far, f32(np.inf)), maxD, f32(0), 0), (near, f32(minD * SF[-1]), minD, 7), (np.nextafter(near, f32(0)), f32(minD * SF[-1]), minD, 7)]
    cases.append(_case("distance", "search", [kpt(320, 240, o, d[j]) for j, (_, _, _, o) in enumerate(spec)],
                       [pt(320, 240, d[j], P=[0, 0, z], maxD=mx, minD=mn) for j, (z, mx, mn, _) in enumerate(spec)], dict(matched=[0, -1, 2, -1], n=2)))

    # the viewing angle with PO = (0, 0, 2), dist = 2: PO . Pn == 0.5 * dist == 1 is kept, one step below is dropped
    d = [rd(), rd()]
    points = [pt(320, 240, d[0], P=[0, 0, 2], normal=(0, 0, 0.5)), pt(320, 240, d[1], P=[0, 0, 2], normal=(0, 0, np.nextafter(f32(0.5), f32(0))))]
    cases.append(_case("angle", "search", [kpt(320, 240, 0, d[0]), kpt(320, 240, 0, d[1])], points, dict(matched=[0, -1], n=1)))

    # a window at level 7 (radius 35.8) with ten keypoints, all within TH_LOW of all ten points: keypoint j is j + 1 bits from the common descriptor, so point j, which
    # finds keypoints 0 .. j - 1 claimed, takes keypoint j: a chain of ten, in windows with more candidates than a candidate cache of the kernel holds
    # (window_7: the last count the cache holds; window_8: the first that overflows it)
    B = rd()
    for name, n in (("window_7", 7), ("window_8", 8), ("big_window", CACHE_CASE_CANDIDATES)):
        kps = [kpt(300 + 6 * j - 27, 300 + (j * 37) % 50 - 25, 7 if j % 2 else 6, fb(B, range(j + 1))) for j in range(n)]
        cases.append(_case(name, "search", kps, [pt(300, 300, B, level=7) for _ in range(n)], dict(matched=list(range(n)), n=n)))

    # scw = 1, 0.5 and 2 with exact entries: Scw = s [I | t], t = (0.25, -0.5, 1); the same keyframe and points give the same answer
    t = (0.25, -0.5, 1.0)
    d = [rd(), rd()]
    for s in (1.0, 0.5, 2.0):
        cases.append(_case("scw_%g" % s, "search", [kpt(100, 100, 0, d[0]), kpt(500, 400, 2, d[1])], [pt(100, 100, d[0], t=t), pt(500, 400, d[1], level=2, t=t)],
                           dict(matched=[0, 1], n=2), Scw=scaled_pose(s, t=t)))

    # Fuse onto a NULL keypoint: added; onto a good occupant: the occupant; onto a bad occupant: counted, nothing written
    d = [rd() for _ in range(3)]
    kps = [kpt(100, 100, 0, d[0], 0), kpt(300, 100, 0, d[1], 1), kpt(500, 100, 0, d[2], 2)]
    cases.append(_case("fuse_states", "fuse", kps, [pt(100, 100, d[0]), pt(300, 100, d[1]), pt(500, 100, d[2])], dict(fused_kp=[0, 1, 2], replace=[A, O, -1], n=3)))

    # three list points with the same bestIdx on a NULL keypoint: the first is added, the second and the third both name the first; on an occupied keypoint all
    # name the occupant; on a bad occupant all are counted and none is written.  (Point 1 is the closest in descriptor: that does not matter.)
    B = rd()
    points = [pt(100, 100, fb(B, range(5))), pt(101, 100, B), pt(100, 101, fb(B, range(9)))]
    for state, rep in ((0, [A, 0, 0]), (1, [O, O, O]), (2, [-1, -1, -1])):
        cases.append(_case("fuse_same_kp_state%d" % state, "fuse", [kpt(100, 100, 0, B, state)], points, dict(fused_kp=[0, 0, 0], replace=rep, n=3)))
    # ... and with a skipped first point the second is the one added
    sk = [dict(points[0], skip=1)] + points[1:]
    cases.append(_case("fuse_same_kp_skip", "fuse", [kpt(100, 100, 0, B, 0)], sk, dict(fused_kp=[-1, 0, 0], replace=[-1, A, 1], n=2)))
    return cases


# ---------------------------------------------------------------------------------------------------------------------------------------------
def make_problem(seed, n_kp=350, n_pts=1000, scale=1.0, mode="search", vis=0.45, noise_px=1.0, kp_flips=8, mp_flips=4, angle=0.3):
    """One keyframe with a pose, and n_pts candidate points in random list order:
      - `vis` * n_kp points the keyframe sees at a keypoint (projection plus Gaussian noise; the octave fixes mfMaxDistance = dist * 1.2^octave, mfMinDistance =
        mfMaxDistance / 1.2^7; the keypoint's descriptor is a base descriptor with kp_flips bits flipped and the point's is the keypoint's with mp_flips more, as
        make_pair of sim3_match_common does).  A tenth of them are already found (search: the keypoint is matched on entry; both: skip is set).
      - duplicates of seen points later in the list (the same position, a few more bits flipped): the search gives them nothing, because the keypoint is claimed
        by then; Fuse sends them to the same keypoint.
      - points behind the camera, points out of the scale range (dist > 1.2 mfMaxDistance) and back-facing points (normal towards the far side); the last two kinds
        have a keypoint with their descriptor waiting at their projection, so only the gate keeps them out.
      - points inside the image that no keypoint observes; bad points (skip) that would match.
    The rest of the keypoints are random.  Fuse: the keypoints of seen points are NULL (60 %), good (30 %) or bad (10 %).
    truth [n_pts]: the keypoint a findable point must go to, -1 for the others."""
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3)
    R = smc.rodrigues(angle * ax / np.linalg.norm(ax)).astype(f32)
    t = rng.uniform(-1, 1, 3).astype(f32)
    R64, t64 = R.astype(f64), t.astype(f64)
    world = lambda Pc: (Pc - t64) @ R64            # Xw = Rcw^T (Pc - tcw)
    Ow = -R64.T @ t64
    n_vis = int(vis * n_kp)
    n_dec = int(0.08 * n_kp)                       # decoy keypoints per gated kind
    n_bad = max(2, n_vis // 20)
    rest = n_pts - n_vis - n_bad
    n_dup, n_behind, n_range, n_back = int(0.05 * rest), int(0.3 * rest), int(0.2 * rest), int(0.2 * rest)
    n_unseen = rest - n_dup - n_behind - n_range - n_back
    assert n_unseen >= 0 and n_vis + 2 * n_dec + n_bad <= n_kp and n_range >= n_dec and n_back >= n_dec

    def inside(n, margin=4.0):
        P = np.zeros((0, 3))
        while len(P) < n:
            C = smc._frustum(rng, 2 * n + 8)
            P = np.concatenate([P, C[smc._inside(smc._project(C), C, margin)]])
        return P[:n]

    kf = empty_kf(n_kp)
    kf["keysUn"]["x"], kf["keysUn"]["y"] = rng.uniform(BOUNDS[0], BOUNDS[2], n_kp), rng.uniform(BOUNDS[1], BOUNDS[3], n_kp)
    kf["keysUn"]["octave"] = rng.integers(0, NLEVELS, n_kp)
    kf["keysUn"]["size"], kf["keysUn"]["class_id"] = 31.0, -1
    kf["desc"] = rng.integers(0, 256, (n_kp, 32), dtype=np.uint8)
    free_rows = list(rng.permutation(n_kp))

    def observe(Pc, n_with_kp):
        """point rows for camera points Pc; the first n_with_kp get a keypoint.  Returns (pts dict, keypoint rows [len(Pc)], -1 without)"""
        m = len(Pc)
        p = empty_pts(m)
        Xw = world(Pc)
        p["Xw"] = Xw.astype(f32)
        PO = Xw - Ow
        dist = np.linalg.norm(PO, axis=1)
        p["normal"] = (PO / dist[:, None]).astype(f32)
        octave = rng.integers(0, NLEVELS, m)
        p["maxDistance"] = (dist * SF[octave].astype(f64)).astype(f32)
        p["minDistance"] = p["maxDistance"] / SF[-1]
        p["desc"] = rng.integers(0, 256, (m, 32), dtype=np.uint8)
        rows = np.full(m, -1, np.int64)
        if n_with_kp:
            rows[:n_with_kp] = [free_rows.pop() for _ in range(n_with_kp)]
            r = rows[:n_with_kp]
            uv = smc._project(Pc[:n_with_kp]) + rng.normal(0, noise_px, (n_with_kp, 2))
            kf["keysUn"]["x"][r], kf["keysUn"]["y"][r], kf["keysUn"]["octave"][r] = uv[:, 0], uv[:, 1], octave[:n_with_kp]
            kf["desc"][r] = smc._flip_random(rng, p["desc"][:n_with_kp], kp_flips)
            p["desc"][:n_with_kp] = smc._flip_random(rng, kf["desc"][r], mp_flips)
        return p, rows

    parts, truth, skip = [], [], []
    # seen points
    p_vis, rows_vis = observe(inside(n_vis), n_vis)
    found = rng.permutation(n_vis)[:n_vis // 10]
    sk = np.zeros(n_vis, np.uint8)
    sk[found] = 1
    tr = rows_vis.copy()
    tr[found] = -1
    if mode == "fuse":
        kf["state"][rows_vis] = rng.choice([0, 1, 2], n_vis, p=[0.6, 0.3, 0.1])
        kf["state"][rows_vis[found]] = 1
    else:
        kf["state"][rows_vis[found]] = 1
    parts.append(p_vis); truth.append(tr); skip.append(sk)
    # duplicates of seen points that are not already found
    src = rng.permutation(np.setdiff1d(np.arange(n_vis), found))[:n_dup]
    n_dup = len(src)
    p_dup = {k: p_vis[k][src].copy() for k in PT_KEYS}
    p_dup["desc"] = smc._flip_random(rng, p_dup["desc"], 3)
    parts.append(p_dup); truth.append(rows_vis[src] if mode == "fuse" else np.full(n_dup, -1, np.int64)); skip.append(np.zeros(n_dup, np.uint8))
    # behind the camera
    Pb = smc._frustum(rng, n_behind)
    Pb[:, 2] = -Pb[:, 2]
    p, _ = observe(Pb, 0)
    parts.append(p); truth.append(np.full(n_behind, -1, np.int64)); skip.append(np.zeros(n_behind, np.uint8))
    # out of range, back-facing
    p, _ = observe(inside(n_range), n_dec)
    p["maxDistance"] = (p["maxDistance"] / f32(10.0)).astype(f32)
    p["minDistance"] = p["maxDistance"] / SF[-1]
    parts.append(p); truth.append(np.full(n_range, -1, np.int64)); skip.append(np.zeros(n_range, np.uint8))
    p, _ = observe(inside(n_back), n_dec)
    p["normal"] = -p["normal"]
    parts.append(p); truth.append(np.full(n_back, -1, np.int64)); skip.append(np.zeros(n_back, np.uint8))
    # unseen, bad
    p, _ = observe(inside(n_unseen), 0)
    parts.append(p); truth.append(np.full(n_unseen, -1, np.int64)); skip.append(np.zeros(n_unseen, np.uint8))
    p, _ = observe(inside(n_bad), n_bad)
    parts.append(p); truth.append(np.full(n_bad, -1, np.int64)); skip.append(np.ones(n_bad, np.uint8))

    pts = {k: np.concatenate([q[k] for q in parts]) for k in PT_KEYS}
    truth, skip = np.concatenate(truth), np.concatenate(skip)
    assert len(truth) == n_pts
    # random list order, every duplicate after its original
    order = rng.permutation(n_pts)
    pos = np.empty(n_pts, np.int64)
    pos[order] = np.arange(n_pts)
    for j, s in enumerate(src):
        a, b = pos[s], pos[n_vis + j]
        if b < a:
            order[a], order[b] = order[b], order[a]
            pos[s], pos[n_vis + j] = b, a
    pts = {k: np.ascontiguousarray(v[order]) for k, v in pts.items()}
    return dict(name="generated_%s_%d" % (mode, seed), mode=mode, kf=kf, pts=pts, skip=np.ascontiguousarray(skip[order]), Scw=scaled_pose(scale, R, t),
                th=f32(FUSE_TH if mode == "fuse" else SEARCH_TH), truth=truth[order].astype(np.int32))


def truth_score(p, result):
    """(findable points, how many of them went to their keypoint, how many points went anywhere else).  result: run_problem's, or the kernel's in the same form."""
    truth = p["truth"]
    if p["mode"] == "fuse":
        got_kp = np.asarray(result[0])
    else:
        matched = np.asarray(result[0])
        got_kp = np.full(len(truth), -1, np.int64)
        k = np.nonzero(matched >= 0)[0]
        got_kp[matched[k]] = k
    want = truth >= 0
    return int(want.sum()), int((got_kp[want] == truth[want]).sum()), int(((got_kp >= 0) & (got_kp != truth)).sum())


def count_of(result):
    return int(result[-1])


# seeds, keypoints, points (no multiple of 64), scale, mode
PARITY_SPECS = [(301, 350, 1001, 1.0, "search"), (302, 300, 517, 0.5, "search"), (303, 400, 1499, 2.0, "search"), (304, 333, 777, 1.1, "search"), (305, 377, 1203, 0.9, "search"),
                (306, 350, 899, 1.0, "search"), (307, 350, 1001, 1.0, "fuse"), (308, 300, 517, 1.05, "fuse"), (309, 400, 1499, 0.95, "fuse"), (310, 333, 777, 2.0, "fuse"),
                (311, 377, 1203, 0.5, "fuse"), (312, 350, 899, 1.0, "fuse")]
FULL_SPEC = (401, 2400, 6007, 1.05)
_cache = {}


def parity_problems():
    """12 generated problems (six per mode), made once"""
    if "parity" not in _cache:
        _cache["parity"] = [make_problem(seed, n_kp, n_pts, scale, mode) for seed, n_kp, n_pts, scale, mode in PARITY_SPECS]
    return _cache["parity"]


def full_problems():
    """one problem per mode at the 2400-keypoint capacity with about 6000 points, made once"""
    if "full" not in _cache:
        seed, n_kp, n_pts, scale = FULL_SPEC
        _cache["full"] = [make_problem(seed, n_kp, n_pts, scale, mode, vis=0.4) for mode in ("search", "fuse")]
    return _cache["full"]


def reference_of(problems, key):
    """run_problem of the given problems, computed once per key"""
    if key not in _cache:
        _cache[key] = [run_problem(p) for p in problems]
    return _cache[key]


def concat_batch(problems, share_pts=False):
    """The flat arrays of a batch of problems of ONE mode: (kf rows, pt rows, skip [n_pt_out], kp_off, pt_off, kp_out_off, pt_out_off).  Every problem gets rows of its
    own; with share_pts the problems (which must then have the same points) share the point rows of problems[0], while skip and the outputs stay per problem."""
    kfs, pts, skips, kp_off, pt_off, kp_out, pt_out = [], [], [], [], [], [], []
    kat = pat = oat = 0
    for j, p in enumerate(problems):
        n_kp, n_pts = len(p["kf"]["state"]), len(p["skip"])
        kp_off.append(kat); kp_out.append(kat); kfs.append(p["kf"]); kat += n_kp
        if share_pts and j > 0:
            pt_off.append(pt_off[0])
        else:
            pt_off.append(pat); pts.append(p["pts"]); pat += n_pts
        pt_out.append(oat); oat += n_pts
        skips.append(p["skip"])
    kf_rows = {k: np.concatenate([q[k] for q in kfs]) if kfs else empty_kf()[k] for k in KF_KEYS}
    pt_rows = {k: np.concatenate([q[k] for q in pts]) if pts else empty_pts()[k] for k in PT_KEYS}
    i32 = lambda v: np.array(v, np.int32)
    return kf_rows, pt_rows, (np.concatenate(skips) if skips else np.zeros(0, np.uint8)), i32(kp_off), i32(pt_off), i32(kp_out), i32(pt_out)
