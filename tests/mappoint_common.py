"""Numpy restatements of the per-match core of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:291-432) with KeyFrame::UnprojectStereo (src/KeyFrame.cc:615-631)
and of Frame::isInFrustum (src/Frame.cc:509-565) with MapPoint::PredictScale (src/MapPoint.cc:505-521) and the radius rule of SearchByProjection
(src/ORBmatcher.cc:57-67), written from the reference text, and hand-built cases whose answers are written in the tables.  Never imports the product's kernels.

Rounding points of the triangulation, as csrc/mappoint.hip documents them: a 3x3 by 3x1 product is cv::gemm's small-matrix branch (float products, float sums left to
right, then one double addition of the translation), Mat::dot and cv::norm accumulate in double, the rows of the DLT matrix are cv::addWeighted (double, one
rounding), 1/z goes through double, cos(2*atan2()) are the float overloads (restated as the double functions rounded to float).  The null vector of the DLT
matrix is numpy.linalg.svd in float64 of the float32 matrix: a true SVD, not a transcription of cv::SVD's Jacobi loop."""
import functools

import numpy as np

from object_slam_amd._lib import KP_DTYPE
from object_slam_amd.matcher import QUERY_DTYPE

f32, f64 = np.float32, np.float64
EPS32 = float(np.finfo(f32).eps)
CAM_FIELDS = ("fx", "fy", "cx", "cy", "invfx", "invfy", "mbf", "mb")
SF = (f32(1.2) ** np.arange(8)).astype(f32)                     # tests/batch_common.py's tables
LS2 = (SF * SF).astype(f32)
RATIO = f32(1.5) * f32(1.2)                                     # src/LocalMapping.cc:262
SF_DYADIC = (f32(2.0) ** np.arange(8)).astype(f32)
LS2_DYADIC = (SF_DYADIC * SF_DYADIC).astype(f32)
NLEVELS = 8

# the gate that decided, in the order the reference decides
(DLT_OK, UNPROJECT1_OK, UNPROJECT2_OK, NO_PARALLAX, W_ZERO, DEPTH_NOT_POSITIVE, BEHIND_1, BEHIND_2, REPROJ_1_MONO, REPROJ_1_STEREO, REPROJ_2_MONO, REPROJ_2_STEREO, SCALE_LOW,
 SCALE_HIGH) = TRI_CODES = ("DLT_OK", "UNPROJECT1_OK", "UNPROJECT2_OK", "NO_PARALLAX", "W_ZERO", "DEPTH_NOT_POSITIVE", "BEHIND_1", "BEHIND_2", "REPROJ_1_MONO", "REPROJ_1_STEREO",
                    "REPROJ_2_MONO", "REPROJ_2_STEREO", "SCALE_LOW", "SCALE_HIGH")
OK_CODES = (DLT_OK, UNPROJECT1_OK, UNPROJECT2_OK)
W_ZERO_TOL = 1e-9      # |v[3]| of the unit float64 null vector below which the restatement says w == 0 (the float Jacobi loop gives an exact 0 only for a zero column)


@functools.lru_cache(maxsize=None)
def cached(fn):
    """the case tables and the probe set, made once and left unchanged"""
    return fn()


def up(v):
    return np.nextafter(f32(v), f32(np.inf))


def down(v):
    return np.nextafter(f32(v), f32(-np.inf))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# triangulation
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _dot3(a, b):
    r = f64(0)
    for k in range(3):
        r += f64(a[k]) * f64(b[k])
    return r


def _tri_one(kf, i, sf, ls2, rf, R, wrong, q):
    """One match.  kf = (kf1, kf2), i = (idx1, idx2).  R rounds a float expression: f32 is the reference; f64 is the same chain of operations without the float
    roundings, for the margins.  wrong = (camera field, view): that view reads the field from the other keyframe than the reference does.  Returns (code, X)."""
    T = [np.asarray(k[0]).reshape(4, 4).astype(R) for k in kf]
    W = [np.asarray(k[1]).reshape(4, 4).astype(R) for k in kf]

    def cam(view, field):
        src = 0 if field == "mbf" else view            # mbf is the current keyframe's in both views (:381, :407)
        if wrong == (field, view + 1):
            src = 1 - src
        return R(kf[src][2][CAM_FIELDS.index(field)])

    kp = [kf[v][3][i[v]] for v in (0, 1)]
    kx, ky = [R(k["x"]) for k in kp], [R(k["y"]) for k in kp]
    octv = [int(k["octave"]) for k in kp]
    ur = [R(kf[v][5][i[v]]) for v in (0, 1)]
    depth = [R(kf[v][6][i[v]]) for v in (0, 1)]
    bS = [bool(u >= 0) for u in ur]
    margins = q.setdefault("margins", [])

    def gate(name, a, b, exact):
        a, b = f64(a), f64(b)
        m = max(abs(a), abs(b))
        margins.append((name, float(abs(a - b) / m) if m > 0 else 0.0, exact))

    xn = [(R((kx[v] - cam(v, "cx")) * cam(v, "invfx")), R((ky[v] - cam(v, "cy")) * cam(v, "invfy")), R(1)) for v in (0, 1)]
    ray = [[W[v][r, 0] * xn[v][0] + W[v][r, 1] * xn[v][1] + W[v][r, 2] * xn[v][2] for r in range(3)] for v in (0, 1)]
    cosRays = R(_dot3(ray[0], ray[1]) / (np.sqrt(_dot3(ray[0], ray[0])) * np.sqrt(_dot3(ray[1], ray[1]))))
    cs = [cosRays + R(1), cosRays + R(1)]
    trig = -1
    if bS[0]:
        trig = 0
    elif bS[1]:
        trig = 1
    if trig >= 0:
        cs[trig] = R(np.cos(f64(R(2) * R(np.arctan2(f64(cam(trig, "mb") / R(2)), f64(depth[trig]))))))
    cosStereo = min(cs[0], cs[1])
    q.update(cosRays=float(cosRays), cs1=float(cs[0]), cs2=float(cs[1]), bStereo=tuple(bS), trig=trig >= 0)

    gate("cosRays<cosStereo", cosRays, cosStereo, trig < 0)
    branch = None
    if cosRays < cosStereo:
        gate("cosRays>0", cosRays, 0.0, True)
        if cosRays > 0:
            if bS[0] or bS[1]:
                branch = "DLT"
            else:
                gate("cosRays<0.9998", cosRays, 0.9998, True)
                if f64(cosRays) < 0.9998:
                    branch = "DLT"
    if branch is None:
        if bS[0]:
            gate("cs1<cs2", cs[0], cs[1], False)
        if bS[0] and cs[0] < cs[1]:
            branch = "UNPROJECT1"
        else:
            if bS[1]:
                gate("cs2<cs1", cs[1], cs[0], False)
            if bS[1] and cs[1] < cs[0]:
                branch = "UNPROJECT2"
    q["branch"] = branch
    if branch is None:
        return NO_PARALLAX, None
    exact = branch != "DLT"            # behind an unprojection every operation is + - * / sqrt or a conversion
    if branch == "DLT":
        A = np.zeros((4, 4), R)
        for k in range(4):
            for v in (0, 1):
                for c in (0, 1):
                    A[2 * v + c, k] = R(f64(T[v][2, k]) * f64(xn[v][c]) + f64(T[v][c, k]) * -1.0 + 0.0)
        vt = np.linalg.svd(A.astype(f64))[2][3]
        q.update(A=A.astype(f32), v=vt, w=float(vt[3]))
        if abs(vt[3]) <= W_ZERO_TOL:
            return W_ZERO, None
        margins.append(("w==0", float(abs(vt[3])), False))
        X = [R(vt[k] / vt[3]) for k in range(3)]
        q["X64"] = vt[:3] / vt[3]
    else:
        v = 0 if branch == "UNPROJECT1" else 1
        z = depth[v]
        q["depth"] = float(z)
        if not z > 0:
            return DEPTH_NOT_POSITIVE, None
        raw = kf[v][4][i[v]]
        x = (R(raw["x"]) - cam(v, "cx")) * z * cam(v, "invfx")
        y = (R(raw["y"]) - cam(v, "cy")) * z * cam(v, "invfy")
        X = [R(f64(W[v][r, 0] * x + W[v][r, 1] * y + W[v][r, 2] * z) + f64(W[v][r, 3])) for r in range(3)]
    q["X"] = [float(c) for c in X]

    zc = [R(_dot3(T[v][2, :3], X) + f64(T[v][2, 3])) for v in (0, 1)]
    q.update(z1=float(zc[0]), z2=float(zc[1]))
    for v in (0, 1):
        gate("z%d>0" % (v + 1), zc[v], 0.0, exact)
        if zc[v] <= 0:
            return (BEHIND_1, BEHIND_2)[v], None
    for v in (0, 1):
        sig = R(ls2[octv[v]])
        xc, yc = R(_dot3(T[v][0, :3], X) + f64(T[v][0, 3])), R(_dot3(T[v][1, :3], X) + f64(T[v][1, 3]))
        invz = R(1.0 / f64(zc[v]))
        u = cam(v, "fx") * xc * invz + cam(v, "cx")
        vv = cam(v, "fy") * yc * invz + cam(v, "cy")
        ex, ey = u - kx[v], vv - ky[v]
        if not bS[v]:
            e2, thr = ex * ex + ey * ey, 5.991 * f64(sig)
        else:
            er = (u - cam(v, "mbf") * invz) - ur[v]
            e2, thr = ex * ex + ey * ey + er * er, 7.8 * f64(sig)
        q.update({"e%d" % (v + 1): float(e2), "thr%d" % (v + 1): float(thr)})
        gate("reproj%d" % (v + 1), e2, thr, exact)
        if f64(e2) > thr:
            return ((REPROJ_1_MONO, REPROJ_1_STEREO), (REPROJ_2_MONO, REPROJ_2_STEREO))[v][bS[v]], None
    d = [R(np.sqrt(_dot3([X[k] - W[v][k, 3] for k in range(3)], [X[k] - W[v][k, 3] for k in range(3)]))) for v in (0, 1)]
    q.update(dist1=float(d[0]), dist2=float(d[1]))
    assert d[0] != 0 and d[1] != 0, "dist == 0 behind z > 0: see the comment of tri_cases()"
    ratioDist = d[1] / d[0]
    ratioOct = R(sf[octv[0]]) / R(sf[octv[1]])
    rf = R(rf)
    q.update(ratioDist=float(ratioDist), ratioOctave=float(ratioOct))
    gate("scale_low", ratioDist * rf, ratioOct, exact)
    if ratioDist * rf < ratioOct:
        return SCALE_LOW, None
    gate("scale_high", ratioDist, ratioOct * rf, exact)
    if ratioDist > ratioOct * rf:
        return SCALE_HIGH, None
    return {"DLT": DLT_OK, "UNPROJECT1": UNPROJECT1_OK, "UNPROJECT2": UNPROJECT2_OK}[branch], X


def restate_triangulate(kf1, kf2, idx1, idx2, scaleFactors, levelSigma2, ratioFactor, detail=None, wrong=None, margins=True):
    """kfN = (Tcw [4, 4], Twc [4, 4], cam8 = fx fy cx cy invfx invfy mbf mb, mvKeysUn [N] KP_DTYPE, mvKeys [N], mvuRight [N], mvDepth [N]), the tuple the oracle takes;
    kf1 is mpCurrentKeyFrame.  Returns (ok [M] uint8, x3D [M, 3] float32, zero where rejected).
    detail receives codes [M] (the gate that decided), q [M] (every gate's quantity from the evaluation in float64, with "margins": (gate, relative distance of the
    two sides, whether both sides come from correctly rounded operations only) for each comparison the match met), q32 [M] (the same from the reference's float
    evaluation) and codes64 [M].  wrong = (camera field, view 1 or 2): see _tri_one; for the census of the per-keyframe cases.  margins=False: codes and q32 only."""
    M = len(idx1)
    ok, x = np.zeros(M, np.uint8), np.zeros((M, 3), f32)
    codes, codes64, qs, q32s = [], [], [], []
    with np.errstate(all="ignore"):
        for m in range(M):
            q32, q64 = {}, {}
            code, X = _tri_one((kf1, kf2), (int(idx1[m]), int(idx2[m])), scaleFactors, levelSigma2, ratioFactor, f32, wrong, q32)
            codes.append(code)
            q32s.append(q32)
            if X is not None:
                ok[m], x[m] = 1, X
            if detail is not None and margins:
                codes64.append(_tri_one((kf1, kf2), (int(idx1[m]), int(idx2[m])), scaleFactors, levelSigma2, ratioFactor, f64, wrong, q64)[0])
                qs.append(q64)
    if detail is not None:
        detail.update(codes=codes, codes64=codes64, q=qs, q32=q32s)
    return ok, x


def _rot(axis, ang):
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def _pose(Rcw, centre):
    """(Tcw, Twc) as two tables, each rounded to float on its own"""
    Tcw, Twc = np.eye(4), np.eye(4)
    Tcw[:3, :3], Tcw[:3, 3] = Rcw, -Rcw @ np.asarray(centre, f64)
    Twc[:3, :3], Twc[:3, 3] = Rcw.T, centre
    return Tcw.astype(f32), Twc.astype(f32)


def _cam(fx, fy, cx, cy, mb):
    return np.array([fx, fy, cx, cy, f32(1) / f32(fx), f32(1) / f32(fy), f32(mb) * f32(fx), mb], f32)


CAM_A = _cam(500.0, 480.0, 320.0, 240.0, 0.5)        # keyframe 1 (the current keyframe)
CAM_B = _cam(550.0, 520.0, 300.0, 260.0, 1.5)        # keyframe 2: all eight fields differ
CAM_C = _cam(550.0, 520.0, 128.0, 0.0, 1.5)          # keyframe 2 of the pairs on one optical axis: a point on the axis projects to (128, 0) exactly
IDENT = (np.eye(4, dtype=f32), np.eye(4, dtype=f32))
GARBAGE = (7.0, -3.0)                                # mvKeys - mvKeysUn where mvKeys must not be read (a keypoint that is not unprojected)


class _Pair:
    """Rows of one keyframe pair: match m = (row m of keyframe 1, row n - 1 - m of keyframe 2)"""

    def __init__(self, name, pose1, pose2, cam1, cam2, settings="general"):
        self.name, self.pose, self.cam, self.settings, self.rows = name, (pose1, pose2), (cam1, cam2), settings, []

    def project(self, v, Xw):
        T = self.pose[v][0].astype(f64)
        p = T[:3, :3] @ np.asarray(Xw, f64) + T[:3, 3]
        c = self.cam[v].astype(f64)
        return c[0] * p[0] / p[2] + c[2], c[1] * p[1] / p[2] + c[3], p[2]

    def world(self, Xc1):
        W = self.pose[0][1].astype(f64)
        return W[:3, :3] @ np.asarray(Xc1, f64) + W[:3, 3]

    def obs(self, v, Xw, octave=0, stereo=False, d=(0.25, -0.5), dur=0.0, depth=None, raw=None, mbf=None):
        """Keypoint of view v for the world point Xw: mvKeys at the projection (+ raw), mvKeysUn d pixels from it; a stereo keypoint has mvDepth = z (or depth) and
        mvuRight = u - mbf / z + dur with the CURRENT keyframe's mbf, as the reference's gate reads it (or mbf)."""
        u, vv, z = self.project(v, Xw)
        raw = ((0.0, 0.0) if stereo else GARBAGE) if raw is None else raw
        k = dict(x=f32(u + d[0]), y=f32(vv + d[1]), octave=octave, rx=f32(u + raw[0]), ry=f32(vv + raw[1]), ur=f32(-1), depth=f32(-1))
        if stereo:
            k["depth"] = f32(z if depth is None else depth)
            k["ur"] = f32(u - float(self.cam[0][6] if mbf is None else mbf) / z + dur)
        return k

    def add(self, name, code, k1, k2, why):
        self.rows.append(dict(name=self.name + "/" + name, code=code, ok=int(code in OK_CODES), k=(k1, k2), why=why))

    def build(self):
        n = len(self.rows)
        kfs = []
        for v in (0, 1):
            rows = [r["k"][v] for r in self.rows]
            if v == 1:
                rows = rows[::-1]
            un, raw = np.zeros(n, KP_DTYPE), np.zeros(n, KP_DTYPE)
            for j, r in enumerate(rows):
                un[j]["x"], un[j]["y"], raw[j]["x"], raw[j]["y"] = r["x"], r["y"], r["rx"], r["ry"]
                un[j]["octave"] = raw[j]["octave"] = r["octave"]
            un["size"] = raw["size"] = 31
            kfs.append((self.pose[v][0], self.pose[v][1], self.cam[v], un, raw, np.array([r["ur"] for r in rows], f32), np.array([r["depth"] for r in rows], f32)))
        sf, ls2, rf = SETTINGS[self.settings]
        return dict(name=self.name, kf1=kfs[0], kf2=kfs[1], idx1=np.arange(n, dtype=np.int32), idx2=np.arange(n, dtype=np.int32)[::-1].copy(), sf=sf, ls2=ls2, rf=rf, settings=self.settings,
                    names=[r["name"] for r in self.rows], codes=[r["code"] for r in self.rows], ok=np.array([r["ok"] for r in self.rows], np.uint8), why=[r["why"] for r in self.rows])


SETTINGS = {"general": (SF, LS2, RATIO), "dyadic": (SF_DYADIC, LS2_DYADIC, f32(2.0)), "probe": (SF, LS2, f32(1e30))}


def cos_rays(pair, k1, k2):
    """cosParallaxRays of two keypoints of a _Pair, as the restatement computes it"""
    q = {}
    un = np.zeros(1, KP_DTYPE)
    kfs = []
    for v, k in ((0, k1), (1, k2)):
        a = un.copy()
        a["x"], a["y"] = k["x"], k["y"]
        kfs.append((pair.pose[v][0], pair.pose[v][1], pair.cam[v], a, a, np.array([-1], f32), np.array([-1], f32)))
    _tri_one(kfs, (0, 0), SF, LS2, RATIO, f32, None, q)
    return f32(q["cosRays"])


def solve_error_sum(T):
    """(ex, ey) float32 with ex = 2 and float(float(ex * ex) + float(ey * ey)) == T, for the float-adjacent error sums: ey is searched among the floats next to
    sqrt(T - 4)"""
    T = f32(T)
    ex = f32(2)
    ey = f32(np.sqrt(f64(T) - 4.0))
    for _ in range(64):
        s = f32(f32(ex * ex) + f32(ey * ey))
        if s == T:
            return ex, ey
        ey = up(ey) if s < T else down(ey)
    raise AssertionError("no float ey reaches the error sum %r" % T)


def straddle(threshold64):
    """the largest float32 that is not > threshold64 as a double, and the next float"""
    lo = f32(threshold64)
    if f64(lo) > threshold64:
        lo = down(lo)
    return lo, up(lo)


def tri_cases():
    """Hand-built keyframe pairs.  Every row names the gate that decides (code) and why.  Keyframe 1 and keyframe 2 differ in all eight camera fields, mvKeys
    differs from mvKeysUn, "far" has poses far from identity.

    Not in the table: dist1 == 0 || dist2 == 0 (:423).  With Twc the inverse of Tcw, z_i = Rcw_i.row(2) . (X - Ow_i), so |z_i| <= dist_i and a point that passed
    z_i > 0 (:356, :360) has dist_i > 0: the decision is unreachable for a keyframe whose two tables agree, and no case is invented for it.  (The SVD probe below
    feeds tables that do not agree, and keeps both centres away from the points it produces.)

    cs1 == cs2 (the final else, :349) is in the table without stereo only, where both are cosRays + 1.  With a stereo keypoint it needs cos(2 atan2()) == cosRays + 1
    exactly: a libm result on a threshold, which the margins of tests/test_mappoint_cases_cpu.py rule out."""
    pairs = []

    # ---- far: world pose far from identity, baseline 1.0 (> mb of keyframe 1, < mb of keyframe 2), points 5 in front: cosRays ~ 0.980 -----------------------------
    Rw = _rot((1, 2, 3), 2.0)
    C1 = np.array([40.0, -25.0, 60.0])
    p = _Pair("far", _pose(Rw, C1), _pose(_rot((0, 1, 0), -0.05) @ Rw, C1 + Rw.T @ np.array([0.8, 0.6, 0.05])), CAM_A, CAM_B)
    X = p.world((0.3, -0.2, 5.0))
    Xb = p.world((-0.6, 0.4, 5.5))
    Xf = p.world((1.5, -1.0, 5.0))
    p.add("dlt_mono", DLT_OK, p.obs(0, Xf, 2), p.obs(1, Xf, 2), "both mono, cosRays 0.982 < 0.9998; a keypoint 100 px and more from either principal point and a diagonal baseline: every "
          "fx fy cx cy invfx invfy read from the other keyframe breaks a reprojection")
    p.add("dlt_stereo1", DLT_OK, p.obs(0, X, 1, True, raw=(30.0, 30.0)), p.obs(1, X, 1), "stereo-1 only: cs1 = cos(2 atan2(0.25, 5)) = 0.995 > cosRays: DLT, mvKeys (30 px off) is not read; "
          "with keyframe 2's mb = 1.5, cs1 = 0.956 < cosRays: UnprojectStereo of the wrong mvKeys")
    p.add("unproject2_stereo2", UNPROJECT2_OK, p.obs(0, X, 1), p.obs(1, X, 1, True), "stereo-2 only: cs2 = cos(2 atan2(0.75, 5)) = 0.956 < cosRays < cs1 = cosRays + 1")
    p.add("dlt_both_stereo", DLT_OK, p.obs(0, Xb, 3, True), p.obs(1, Xb, 3, True, depth=0.2), "both stereo: only cs1 is computed (0.996 > cosRays); cs2 of mvDepth2 = 0.2 would be -0.87 "
          "and send the match to the third branch")
    p.add("dlt_reproj1_mono", REPROJ_1_MONO, p.obs(0, X, 0, d=(0.25, 40.0)), p.obs(1, X, 0), "DLT of a keypoint 40 px off: the error of view 1 is far above 5.991")
    p.add("dlt_reproj1_stereo", REPROJ_1_STEREO, p.obs(0, X, 0, True, dur=30.0), p.obs(1, X, 0), "DLT, view 1 stereo: mvuRight 30 px off")
    p.add("dlt_reproj2_mono", REPROJ_2_MONO, p.obs(0, X, 7), p.obs(1, X, 0, d=(12.0, -12.0)), "DLT: 12 px off in view 2; view 1 at octave 7 takes its share of the error, view 2 at octave 0 does not")
    p.add("dlt_reproj2_stereo", REPROJ_2_STEREO, p.obs(0, X, 1, True), p.obs(1, X, 1, True, dur=30.0), "DLT (both stereo), view 2 stereo: mvuRight 30 px off")
    p.add("dlt_scale_low", SCALE_LOW, p.obs(0, X, 7), p.obs(1, X, 0), "ratioDist ~ 1, ratioOctave = 1.2^7 = 3.58: 1.8 < 3.58")
    p.add("dlt_scale_high", SCALE_HIGH, p.obs(0, X, 0), p.obs(1, X, 7), "ratioDist ~ 1, ratioOctave = 0.279: 1 > 0.502")
    pairs.append(p)

    # ---- wide: the same with a baseline of 2.5 (> mb of keyframe 2), the point 8 in front: cosRays ~ 0.95 ---------------------------------------------------------------
    p = _Pair("wide", _pose(Rw, C1), _pose(_rot((0, 1, 0), -0.1) @ Rw, C1 + Rw.T @ np.array([2.0, 1.5, 0.1])), CAM_A, CAM_B)
    X = p.world((0.8, -0.5, 8.0))
    p.add("dlt_stereo2", DLT_OK, p.obs(0, X, 3), p.obs(1, X, 3, True), "stereo-2 only: cs2 = cos(2 atan2(0.75, 8)) = 0.983 > cosRays: DLT")
    pairs.append(p)

    # ---- near: baseline 0.05, cosRays ~ 0.99995: a stereo keypoint at depth 5 is unprojected ----------------------------------------------------------------------
    R1 = _rot((0, 0, 1), 0.01)
    C1 = np.array([0.1, 0.2, -0.1])
    p = _Pair("near", _pose(R1, C1), _pose(_rot((0, 1, 0), 0.002) @ R1, C1 + R1.T @ np.array([0.04, 0.03, 0.0])), CAM_A, CAM_B)
    X = p.world((0.3, -0.2, 5.0))
    mbf2 = float(CAM_B[6])
    p.add("unproject1", UNPROJECT1_OK, p.obs(0, X, 1, True), p.obs(1, X, 1), "stereo-1 only: cs1 = 0.995 < cosRays; view 1 stereo and view 2 mono pass")
    p.add("unproject2", UNPROJECT2_OK, p.obs(0, X, 1), p.obs(1, X, 1, True), "stereo-2 only: cs2 = 0.956 < cosRays; view 1 mono and view 2 stereo pass")
    p.add("both_stereo_unproject1", UNPROJECT1_OK, p.obs(0, X, 1, True), p.obs(1, X, 1, True, depth=0.2, raw=(30.0, 30.0)), "both stereo: cs2 stays cosRays + 1, so view 1 is unprojected; were "
          "cs2 computed (mvDepth2 = 0.2: -0.87) the wrong mvKeys of view 2 would be unprojected.  View 2's stereo term uses keyframe 1's mbf = 250 (keyframe 2's is 825)")
    p.add("mbf_of_keyframe2_fails", REPROJ_2_STEREO, p.obs(0, X, 1, True), p.obs(1, X, 1, True, mbf=mbf2), "companion: mvuRight2 = u - mbf2 / z, right for keyframe 2's own rig, fails the "
          "reference's gate by (825 - 250) / 5 px and would pass only with keyframe 2's mbf")
    p.add("mono_cs1_eq_cs2", NO_PARALLAX, p.obs(0, X, 1), p.obs(1, X, 1), "both mono, cosRays >= 0.9998: cs1 == cs2 == cosRays + 1, neither unprojection branch is taken")
    p.add("depth_zero", DEPTH_NOT_POSITIVE, p.obs(0, X, 1, True, depth=0.0), p.obs(1, X, 1), "mvuRight1 >= 0 with mvDepth1 == 0: cs1 = cos(2 atan2(0.25, 0)) = -1, UnprojectStereo returns nothing")
    p.add("depth_negative", DEPTH_NOT_POSITIVE, p.obs(0, X, 1, True, depth=-1.0), p.obs(1, X, 1), "mvDepth1 = -1: cs1 = cos(2 atan2(0.25, -1)) = 0.88 < cosRays")
    p.add("reproj1_stereo", REPROJ_1_STEREO, p.obs(0, X, 1, True, dur=5.0), p.obs(1, X, 1), "unprojected from view 1, whose own mvuRight is 5 px off: 25 > 7.8 * 1.44")
    p.add("reproj1_stereo_by_keysun", REPROJ_1_STEREO, p.obs(0, X, 0, True, d=(3.0, 0.0)), p.obs(1, X, 0), "mvKeysUn1 3 px from mvKeys1: ex^2 = 9 > 7.8")
    p.add("reproj2_mono", REPROJ_2_MONO, p.obs(0, X, 1, True), p.obs(1, X, 1, d=(3.0, -1.0)), "view 2 mono 10 px^2 off: > 5.991 * 1.44 = 8.63")
    p.add("reproj2_mono_pass", UNPROJECT1_OK, p.obs(0, X, 1, True), p.obs(1, X, 1, d=(2.5, -1.0)), "view 2 mono 7.25 px^2 off: < 8.63")
    p.add("reproj1_mono", REPROJ_1_MONO, p.obs(0, X, 1, d=(3.0, -1.0)), p.obs(1, X, 1, True), "unprojected from view 2; view 1 mono 10 px^2 off")
    p.add("reproj1_mono_pass", UNPROJECT2_OK, p.obs(0, X, 1, d=(2.5, -1.0)), p.obs(1, X, 1, True), "view 1 mono 7.25 px^2 off")
    p.add("reproj2_stereo", REPROJ_2_STEREO, p.obs(0, X, 1), p.obs(1, X, 1, True, dur=3.4), "unprojected from view 2, whose mvuRight is 3.4 px off: 0.31 + 11.56 > 7.8 * 1.44 = 11.2")
    p.add("reproj2_stereo_pass", UNPROJECT2_OK, p.obs(0, X, 1), p.obs(1, X, 1, True, dur=3.0), "3.0 px off: 0.31 + 9.0 < 11.2")
    pairs.append(p)

    # ---- threshold: identity rotations, centres 0.1 apart on x, keypoint 1 at the principal point: cosRays = 1 / sqrt(1 + xn2^2) -------------------------------------
    p = _Pair("threshold", IDENT, _pose(np.eye(3), (0.1, 0.0, 0.0)), CAM_A, CAM_B)
    k1 = dict(x=CAM_A[2], y=CAM_A[3], octave=0, rx=CAM_A[2] + f32(7), ry=CAM_A[3] - f32(3), ur=f32(-1), depth=f32(-1))
    x = f32(CAM_B[2] - 0.0200040012 * CAM_B[0] - 0.01)       # cos = 0.9998 at xn2 = -0.020004; the scan goes towards the principal point, cosRays rising
    mk = lambda xx: dict(k1, x=xx, y=CAM_B[3], rx=xx + f32(7), ry=CAM_B[3] - f32(3))
    for _ in range(4000):
        if f64(cos_rays(p, k1, mk(up(x)))) >= 0.9998:
            break
        x = up(x)
    else:
        raise AssertionError("0.9998 not crossed")
    p.add("cos_below_9998", DLT_OK, k1, mk(x), "mono-mono, the last float of kp2.x with cosRays < 0.9998: DLT of the point 5 in front")
    p.add("cos_at_9998", NO_PARALLAX, k1, mk(up(x)), "the next float of kp2.x: cosRays is the first float >= 0.9998")
    pairs.append(p)

    # ---- right_angle: Twc2 is an exact rotation by 90 degrees about y (camera 2 looks along world +x) -----------------------------------------------------------------
    Rwc2 = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])
    p = _Pair("right_angle", IDENT, _pose(Rwc2.T, (-2.8, 0.0, 4.4)), CAM_A, CAM_B)
    X0, Xn = np.array([0.0, 0.0, 4.4]), np.array([-2.0, 0.0, 4.0])      # on both optical axes; X - O1 = (-2, 0, 4), X - O2 = (0.8, 0, -0.4): cos = -0.8
    # (octaves 0 and 7 where Xn is accepted: ratioDist = 0.2, ratioOctave = 1.2^-7 = 0.279; depth 4 in view 1 keeps mvuRight1 = 70 - 250 / 4 >= 0)
    p.add("cos_zero_mono", NO_PARALLAX, p.obs(0, X0, 0, d=(0, 0)), dict(p.obs(1, X0, 0), x=CAM_B[2], y=CAM_B[3]), "both keypoints at their principal points: rays (0,0,1) and (1,0,0), cosRays == 0 exactly, "
          "cosRays > 0 fails")
    p.add("cos_zero_stereo1", UNPROJECT1_OK, p.obs(0, X0, 0, True, d=(0, 0), raw=(1.0, 0.5)), dict(p.obs(1, X0, 0), x=CAM_B[2], y=CAM_B[3]), "cosRays == 0 with stereo-1: no DLT, cs1 = 0.994 < cs2 = 1")
    p.add("cos_negative_mono", NO_PARALLAX, p.obs(0, Xn, 0), p.obs(1, Xn, 0), "cosRays = -0.8, mono")
    p.add("cos_negative_both_stereo_unproject2", UNPROJECT2_OK, p.obs(0, Xn, 0, True), p.obs(1, Xn, 7, True), "the one way to UnprojectStereo of view 2 with both stereo: cosRays < 0, so "
          "cs2 = cosRays + 1 = 0.2 < cs1 = 0.992")
    p.add("mb2_selects_unproject2", UNPROJECT2_OK, p.obs(0, Xn, 0), p.obs(1, Xn, 7, True), "stereo-2 only, depth 0.8: cs2 = cos(2 atan2(0.75, 0.8)) = 0.064 < cs1 = 0.2; with keyframe 1's "
          "mb = 0.5 it is 0.82 and the match is dropped")
    pairs.append(p)

    # ---- back / front: both cameras on one optical axis, identity rotations, dyadic translations: every quantity behind UnprojectStereo is exact -----------------------
    def axis_k1(z, octave, stereo=True, d=(0.25, -0.5), depth=None):
        """keypoint of keyframe 1 whose mvKeys is the principal point: UnprojectStereo gives (0, 0, depth) exactly; mvKeysUn d from it (error 0.3125); mvuRight = u - mbf1 / z as the gate computes it"""
        k = dict(x=f32(CAM_A[2] + f32(d[0])), y=f32(CAM_A[3] + f32(d[1])), octave=octave, rx=CAM_A[2], ry=CAM_A[3], ur=f32(-1), depth=f32(-1))
        if stereo:
            k["depth"] = f32(z if depth is None else depth)
            k["ur"] = f32(CAM_A[2] - f32(CAM_A[6] * f32(1.0 / f64(f32(z)))))
        return k

    def axis_k2(z2, octave, stereo=False, d=(0.0, 0.0), depth=None):
        """keypoint of keyframe 2 (principal point (128, 0)): the point on the axis projects to (128, 0) exactly, so the error is (d[0], d[1]) exactly"""
        k = dict(x=f32(f32(128) - f32(d[0])), y=f32(-f32(d[1])), octave=octave, rx=f32(128) + f32(GARBAGE[0]), ry=f32(GARBAGE[1]), ur=f32(-1), depth=f32(-1))
        if stereo:
            k.update(depth=f32(z2 if depth is None else depth), rx=f32(128), ry=f32(0))
            k["ur"] = f32(f32(128) - f32(CAM_A[6] * f32(1.0 / f64(f32(z2)))))      # u_r of the gate with keyframe 1's mbf: errX_r == 0
        return k

    p = _Pair("back", IDENT, _pose(np.eye(3), (0.0, 0.0, -2.0)), CAM_A, CAM_C)             # camera 2 two behind camera 1: z2 = z + 2
    for thr, tag, st2, o2 in ((5.991, "mono_5991", False, 1), (7.8, "stereo_78", True, 2)):
        lo, hi = straddle(thr * f64(LS2[o2]))
        p.add("adjacent_%s_pass" % tag, UNPROJECT1_OK, axis_k1(4.0, 3), axis_k2(6.0, o2, st2, solve_error_sum(lo)), "view 2 error sum = the last float <= %g * sigma2[%d]" % (thr, o2))
        p.add("adjacent_%s_fail" % tag, (REPROJ_2_MONO, REPROJ_2_STEREO)[st2], axis_k1(4.0, 3), axis_k2(6.0, o2, st2, solve_error_sum(hi)), "the next float")
    p.add("sigma_view1_octave7", UNPROJECT1_OK, axis_k1(1.0, 7, d=(4.0, -2.0)), axis_k2(3.0, 0), "view 1 (stereo) 20 px^2 off at octave 7 = nLevels - 1, view 2 exact at octave 0: "
          "passes only with sigma2[kp1.octave] = 12.8 in view 1 (7.8 * 1 < 20 < 7.8 * 12.8); ratioDist = 3, ratioOctave = 3.58")
    p.add("sigma_view2_octave0", REPROJ_2_MONO, axis_k1(1.0, 7), axis_k2(3.0, 0, d=(4.0, -2.0)), "view 2 (mono) 20 px^2 off at octave 0, view 1 at octave 7: fails with sigma2[kp2.octave] = 1, "
          "would pass with kp1's")
    p.add("scale_high_fail", SCALE_HIGH, axis_k1(2.375, 2), axis_k2(4.375, 2), "ratioDist = 4.375 / 2.375 = 1.842 > 1 * 1.8")
    p.add("scale_high_pass", UNPROJECT1_OK, axis_k1(2.625, 2), axis_k2(4.625, 2), "ratioDist = 1.762 <= 1.8")
    p.add("scale_low_fail", SCALE_LOW, axis_k1(2.0625, 7), axis_k2(4.0625, 0), "ratioDist = 1.970, * 1.8 = 3.545 < ratioOctave = 3.583")
    p.add("scale_low_pass", UNPROJECT1_OK, axis_k1(1.9375, 7), axis_k2(3.9375, 0), "ratioDist = 2.032, * 1.8 = 3.658 >= 3.583 (and 2.03 <= 6.45)")
    p.add("behind1", BEHIND_1, axis_k1(1.0, 0, False), axis_k2(1.96875, 0, True, (0.25, -0.5)), "stereo-2 only, parallel rays: view 2 unprojected at depth 63/32 = world z -1/32: behind camera 1 alone (mvuRight2 >= 0 needs depth >= 1.96)")
    p.add("behind1_z_zero", BEHIND_1, axis_k1(1.0, 0, False), axis_k2(2.0, 0, True, (0.25, -0.5)), "depth 2: z1 == 0 exactly, rejected by <=")
    pairs.append(p)

    p = _Pair("front", IDENT, _pose(np.eye(3), (0.0, 0.0, 1.5)), CAM_A, CAM_C)             # camera 2 1.5 in front of camera 1: z2 = z - 1.5
    p.add("behind2", BEHIND_2, axis_k1(1.0, 0), axis_k2(1.0, 0), "view 1 unprojected at depth 1: z2 = -0.5, behind camera 2 alone")
    p.add("behind2_z_zero", BEHIND_2, axis_k1(1.5, 0), axis_k2(1.0, 0), "depth 1.5: z2 == 0 exactly")
    p.add("sigma_view2_octave7", UNPROJECT1_OK, axis_k1(2.0, 0), axis_k2(0.5, 7, d=(4.0, -2.0)), "view 2 (mono) 20 px^2 off at octave 7, view 1 at octave 0: passes only with "
          "sigma2[kp2.octave]; ratioDist = 0.25, ratioOctave = 0.279")
    p.add("sigma_view1_octave0", REPROJ_1_STEREO, axis_k1(2.0, 0, d=(4.0, -2.0)), axis_k2(0.5, 7), "view 1 (stereo) 20 px^2 off at octave 0: fails with sigma2[kp1.octave] = 1")
    pairs.append(p)

    # ---- dyadic: the geometry of "back" with scale factors 2^i and ratioFactor 2: both sides of the scale test are exact ---------------------------------------------
    p = _Pair("dyadic", IDENT, _pose(np.eye(3), (0.0, 0.0, -2.0)), CAM_A, CAM_C, "dyadic")
    p.add("scale_low_equal", UNPROJECT1_OK, axis_k1(2.0, 2), axis_k2(4.0, 0), "dist 2 and 4, ratioOctave = 4 / 1: ratioDist * ratioFactor == ratioOctave == 4 exactly, and < keeps it")
    p.add("scale_high_equal", UNPROJECT1_OK, axis_k1(2.0, 1), axis_k2(4.0, 1), "ratioOctave = 1: ratioDist == ratioOctave * ratioFactor == 2 exactly, and > keeps it")
    p.add("scale_low_below", SCALE_LOW, axis_k1(2.0, 3), axis_k2(4.0, 0), "ratioOctave = 8 > 4")
    p.add("scale_high_above", SCALE_HIGH, axis_k1(2.0, 0), axis_k2(4.0, 1), "ratioOctave = 1 / 2: 2 > 1")
    pairs.append(p)

    # ---- probe: the SVD probe with a matrix whose first column is zero: the null vector is e0 and w == 0 --------------------------------------------------------------
    pr = svd_probe_problem(SVD_EXACT["null_e0"][0])
    pairs.append(dict(pr, name="probe", names=["probe/w_zero_null_e0"], codes=[W_ZERO], ok=np.zeros(1, np.uint8), why=["the DLT matrix has a zero first column: vt.row(3) = e0, w == 0 (:334)"],
                      settings="probe"))
    return [q if isinstance(q, dict) else q.build() for q in pairs]


# the per-keyframe camera reads: (case, field, view) -> the case's accept flag flips when that view reads the field from the other keyframe
CAMERA_FLIPS = [("far/dlt_mono", f, v) for f in ("fx", "fy", "cx", "cy", "invfx", "invfy") for v in (1, 2)] + [
    ("far/dlt_stereo1", "mb", 1), ("right_angle/mb2_selects_unproject2", "mb", 2), ("near/unproject1", "mbf", 1), ("near/both_stereo_unproject1", "mbf", 2),
    ("near/mbf_of_keyframe2_fails", "mbf", 2)]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# svd4_last_row through the operator
# ---------------------------------------------------------------------------------------------------------------------------------------------
def svd_probe_problem(A):
    """The triangulation whose DLT matrix is the float 4x4 A: both keypoints at their principal points (xn = (0, 0, 1)), Tcw1 = [-A[0]; -A[1]; 0 0 0 1], Tcw2 =
    [-A[2]; -A[3]; 0 0 0 1].  Twc is a table of its own that the operator does not cross-check: 11 degrees between the rays (DLT branch), centres away from
    anything the null vector gives.  z = 1 in both views, fx = fy = 1e-6 (2e-6 in keyframe 2: no reprojection error), ratioFactor 1e30: the operator returns v[:3] / v[3]."""
    A = np.asarray(A, f32).reshape(4, 4)
    kfs = []
    for v in (0, 1):
        Tcw = np.zeros((4, 4), f32)
        Tcw[0], Tcw[1], Tcw[2], Tcw[3] = -A[2 * v], -A[2 * v + 1], (0, 0, 0, 1), (0, 0, 0, 1)
        Twc = np.eye(4)
        Twc[:3, :3], Twc[:3, 3] = (np.eye(3), _rot((0, 1, 0), np.deg2rad(11.0)))[v], ((37.0, -29.0, 41.0), (-43.0, 31.0, 53.0))[v]
        cam = np.array([(1e-6, 2e-6)[v], (1e-6, 2e-6)[v], (320.0, 300.0)[v], (240.0, 260.0)[v], (0.002, 0.0018)[v], (0.0021, 0.0019)[v], (250.0, 825.0)[v], (0.5, 1.5)[v]], f32)
        un = np.zeros(1, KP_DTYPE)
        un["x"], un["y"], un["size"] = cam[2], cam[3], 31
        raw = un.copy()
        raw["x"] += 7
        kfs.append((Tcw, Twc.astype(f32), cam, un, raw, np.array([-1], f32), np.array([-1], f32)))
    sf, ls2, rf = SETTINGS["probe"]
    return dict(kf1=kfs[0], kf2=kfs[1], idx1=np.zeros(1, np.int32), idx2=np.zeros(1, np.int32), sf=sf, ls2=ls2, rf=rf)


def svd_probe_set(n=2000, seed=5):
    """n float matrices U diag(1, 0.5, 0.2, s4) V^T, s4 in {0, 1e-3, 0.05, 0.19} in turn, with |v[3]| >= 0.05 of the last right singular vector.  Returns
    (A [n, 4, 4] float32, v [n, 4] and gap [n] = (s3 - s4) / s1 from the float64 SVD of the float32 matrix)."""
    rng = np.random.default_rng(seed)
    As, vs, gaps = [], [], []
    while len(As) < n:
        s4 = (0.0, 1e-3, 0.05, 0.19)[len(As) % 4]
        U, V = np.linalg.qr(rng.normal(size=(4, 4)))[0], np.linalg.qr(rng.normal(size=(4, 4)))[0]
        if abs(V[3, 3]) < 0.06:
            continue
        A = (U @ np.diag([1.0, 0.5, 0.2, s4]) @ V.T).astype(f32)
        _, s, vt = np.linalg.svd(A.astype(f64))
        if abs(vt[3, 3]) < 0.05:
            continue
        As.append(A)
        vs.append(vt[3])
        gaps.append((s[2] - s[3]) / s[0])
    return np.stack(As), np.stack(vs), np.array(gaps)


def angle_gap(X, v, gap):
    """angle between (X, 1) and the null vector v, times the gap, in float epsilons"""
    u = np.concatenate([np.asarray(X, f64), [1.0]])
    u /= np.linalg.norm(u)
    v = v / np.linalg.norm(v)
    return float(np.arcsin(min(1.0, np.linalg.norm(u - (u @ v) * v))) * gap / EPS32)


# name -> (A, accept flag, position): exact answers
SVD_EXACT = {
    "null_e0": (np.array([[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 1, 1, 1]], f32), 0, (0.0, 0.0, 0.0)),           # first column zero: v = e0, w == 0: rejected
    "null_e3": (np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [1, 1, 1, 0]], f32), 1, (0.0, 0.0, 0.0)),           # last column zero: v = e3, X = 0, accepted
    "rank2_tie": (np.array([[1, 2, 0, 0], [3, 1, 0, 0], [0, 1, 0, 0], [2, 0, 0, 0]], f32), 1, (0.0, 0.0, 0.0)),         # two zero singular values: the strict < of the sort
}                                                                                                                         # keeps row 3 = e3 last (<= would put e2 there: w == 0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Frame::isInFrustum
# ---------------------------------------------------------------------------------------------------------------------------------------------
(F_BEHIND, F_U_LOW, F_U_HIGH, F_V_LOW, F_V_HIGH, F_NEAR, F_FAR, F_ANGLE, F_IN_VIEW) = FRUSTUM_CODES = ("BEHIND", "U_LOW", "U_HIGH", "V_LOW", "V_HIGH", "TOO_NEAR", "TOO_FAR", "VIEW_ANGLE",
                                                                                                      "IN_VIEW")
F_K5 = np.array([512.0, 256.0, 320.0, 240.0, 48.0], f32)          # dyadic fx, fy (and z a power of two): the projections of the cases are exact
F_BOUNDS = (0.0, 0.0, 640.0, 480.0)
F_COSLIMIT = f32(0.5)
F_LOGSF = f32(np.log(f64(f32(1.2))))                              # mfLogScaleFactor = log(mfScaleFactor), correctly rounded
F_POSE_SHIFT = np.array([0.5, 0.0, 1.0])
F_POSE_NEGZERO = np.where(np.eye(4) == 1, 1.0, -0.0).astype(f32)  # the identity pose of the cases: PcZ = -0.0 is reachable only when no term of the row is +0.0                        # camera centre of the second pose of the cases (identity rotation, dyadic translation)


def restate_frustum(Pw, Pn, maxDist, minDist, obs_gt0, mp_desc, Tcw, K5, bounds, viewingCosLimit, logScaleFactor, scaleFactors, th, detail=None):
    """src/Frame.cc:509-565 with PredictScale and the radius of SearchByProjection, float32 scalars in the reference's order; double where the C++ expression is one.
    Returns [M] QUERY_DTYPE (a point that is not in view: zeros, levels -1, a zero descriptor).  detail receives codes [M] and, for the points in view, info [M] =
    dict(level before the clamp, radius factor)."""
    Pw = np.asarray(Pw, f32).reshape(-1, 3)
    Pn = np.asarray(Pn, f32).reshape(-1, 3)
    T = np.asarray(Tcw, f32).reshape(4, 4)
    fx, fy, cx, cy, bf = [f32(v) for v in K5]
    minX, minY, maxX, maxY = [f32(v) for v in bounds]
    sf = np.asarray(scaleFactors, f32)
    nLevels = len(sf)
    th, lim, logsf = f32(th), f32(viewingCosLimit), f32(logScaleFactor)
    out = np.zeros(len(Pw), QUERY_DTYPE)
    out["minLevel"] = out["maxLevel"] = -1
    codes, info = [], []
    with np.errstate(all="ignore"):
        Ow = [f32(-1.0 * sum(f64(T[k, r]) * f64(T[k, 3]) for k in range(3))) for r in range(3)]        # mOw = -Rcw^T tcw: one gemm with alpha = -1
        for i, P in enumerate(Pw):
            info.append(None)
            Pc = [f32(f64(T[r, 0] * P[0] + T[r, 1] * P[1] + T[r, 2] * P[2]) + f64(T[r, 3])) for r in range(3)]
            if Pc[2] < f32(0):
                codes.append(F_BEHIND)
                continue
            invz = f32(1) / Pc[2]
            u = fx * Pc[0] * invz + cx
            v = fy * Pc[1] * invz + cy
            if u < minX or u > maxX:
                codes.append(F_U_LOW if u < minX else F_U_HIGH)
                continue
            if v < minY or v > maxY:
                codes.append(F_V_LOW if v < minY else F_V_HIGH)
                continue
            maxDistance, minDistance = f32(1.2) * f32(maxDist[i]), f32(0.8) * f32(minDist[i])
            PO = [P[k] - Ow[k] for k in range(3)]
            dist = f32(np.sqrt(_dot3(PO, PO)))
            if dist < minDistance or dist > maxDistance:
                codes.append(F_NEAR if dist < minDistance else F_FAR)
                continue
            viewCos = f32(_dot3(PO, Pn[i]) / f64(dist))
            if viewCos < lim:
                codes.append(F_ANGLE)
                continue
            ratio = f32(maxDist[i]) / dist
            level = np.ceil(f32(np.log(f64(ratio))) / logsf)                    # std::log(float), restated as the double logarithm rounded to float
            nScale = 0 if level < 0 else nLevels - 1 if level >= nLevels else int(level)
            r = f32(2.5) if f64(viewCos) > 0.998 else f32(4.0)
            info[-1] = dict(level=float(level), r=float(r))
            if th != f32(1):
                r = r * th
            q = out[i]
            q["u"], q["v"], q["ur"], q["radius"] = u, v, u - bf * invz, r * sf[nScale]
            q["minLevel"], q["maxLevel"], q["flags"], q["angle"] = nScale - 1, nScale, 1 | (2 if obs_gt0[i] else 0), viewCos
            q["desc"] = mp_desc[i]
            codes.append(F_IN_VIEW)
    if detail is not None:
        detail.update(codes=codes, info=info)
    return out


def frustum_cases():
    """Points against the identity pose F_POSE_NEGZERO with F_K5 and F_BOUNDS: at z = 2, u = 256 x + 320 and v = 128 y + 240 exactly; on the axis dist = z and viewCos = Pn.z.
    Returns dict(names, codes, Pw, Pn, maxD, minD, obs, desc, expect: name -> fields written in the table, shiftable: the rows whose coordinates stay exact under
    F_POSE_SHIFT)."""
    rows = []

    def add(name, code, P, Pn=(0.0, 0.0, 1.0), maxD=4.0, minD=0.5, obs=1, shift=True, **expect):
        rows.append(dict(name=name, code=code, P=[f32(c) for c in P], Pn=[f32(c) for c in Pn], maxD=f32(maxD), minD=f32(minD), obs=obs, shift=shift, expect=expect))

    tiny, fmin = f32(1e-45), np.finfo(f32).tiny              # the smallest denormal and the smallest normal float
    # depth: PcZ < 0.0f and what 1 / PcZ becomes around zero
    add("z_denormal_below_zero", F_BEHIND, (0.0, 0.0, -tiny), shift=False)
    add("z_normal_below_zero", F_BEHIND, (0.0, 0.0, -fmin), shift=False)
    # PcZ == -0.0 needs every term of the row -0.0: the pose F_POSE_NEGZERO (the identity with -0.0 for its zeros) and +0.0 in the other coordinates
    add("z_minus_zero_x_zero", F_NEAR, (0.0, 0.0, -0.0), shift=False)          # -0.0 < 0 is false; invz = -inf, u = v = 0 * -inf = NaN: no comparison of a NaN rejects; dist = 0 < 0.4
    add("z_minus_zero_x_positive", F_U_LOW, (1.0, 0.0, -0.0), shift=False)     # u = 512 * -inf = -inf
    add("z_minus_zero_y_only", F_V_LOW, (0.0, 1.0, -0.0), shift=False)         # u = NaN passes, v = 256 * -inf = -inf
    add("z_plus_zero_x_zero", F_NEAR, (0.0, 0.0, 0.0), shift=False)            # invz = +inf, u = v = NaN
    add("z_plus_zero_x_positive", F_U_HIGH, (1.0, 0.0, 0.0), shift=False)      # u = +inf
    add("z_plus_zero_x_negative", F_U_LOW, (-1.0, 0.0, 0.0), shift=False)
    add("z_denormal_above_zero", F_U_HIGH, (1.0, 0.0, tiny), shift=False)      # 1 / denormal = inf
    add("z_normal_above_zero", F_NEAR, (0.0, 0.0, fmin), shift=False)          # invz = 8.5e37 is finite, u = cx, v = cy: in the image, and nearer than 0.8 * minDist
    # image bounds at z = 2, inclusive; `u_outside` / `v_outside`: the first float of x / y whose projection leaves the bound
    add("u_at_min", F_IN_VIEW, (-1.25, 0.0, 2.0), u=0.0, v=240.0)
    add("u_at_max", F_IN_VIEW, (1.25, 0.0, 2.0), u=640.0, v=240.0)
    add("v_at_min", F_IN_VIEW, (0.0, -1.875, 2.0), u=320.0, v=0.0)
    add("v_at_max", F_IN_VIEW, (0.0, 1.875, 2.0), u=320.0, v=480.0)
    add("u_below_min", F_U_LOW, (down(-1.25), 0.0, 2.0))                       # u = -2^-15
    add("v_below_min", F_V_LOW, (0.0, down(-1.875), 2.0))
    x = f32(1.25)
    while f32(f32(256) * x + f32(320)) <= f32(640):                            # 256 * ulp(1.25) is half an ulp of 640: the first x above 1.25 still rounds to 640
        x = up(x)
    add("u_above_max", F_U_HIGH, (x, 0.0, 2.0))
    y = f32(1.875)
    while f32(f32(128) * y + f32(240)) <= f32(480):
        y = up(y)
    add("v_above_max", F_V_HIGH, (0.0, y, 2.0))
    # distance, on the axis: dist = z; minDistance = 0.8f * 2, maxDistance = 1.2f * 4
    near, far = f32(0.8) * f32(2), f32(1.2) * f32(4)
    add("dist_at_min", F_IN_VIEW, (0.0, 0.0, near), maxD=4.0, minD=2.0, shift=False)
    add("dist_below_min", F_NEAR, (0.0, 0.0, down(near)), maxD=4.0, minD=2.0, shift=False)
    add("dist_at_max", F_IN_VIEW, (0.0, 0.0, far), maxD=4.0, minD=2.0, shift=False, minLevel=-1, maxLevel=0, radius=2.5)      # ratio 0.8333333: log / log 1.2 = -0.99999994, level -0
    add("dist_above_max", F_FAR, (0.0, 0.0, up(far)), maxD=4.0, minD=2.0, shift=False)
    # viewing angle, on the axis at z = 2: viewCos = Pn.z exactly
    add("viewcos_at_limit", F_IN_VIEW, (0.0, 0.0, 2.0), (0.0, 0.0, 0.5), angle=0.5, radius=4.0 * float(SF[4]))
    add("viewcos_below_limit", F_ANGLE, (0.0, 0.0, 2.0), (0.0, 0.0, down(0.5)))
    lo998, hi998 = straddle(0.998)
    add("viewcos_998_below", F_IN_VIEW, (0.0, 0.0, 2.0), (0.3, 0.0, lo998), radius=4.0 * float(SF[4]))       # ratio 2: log 2 / log 1.2 = 3.8: level 4
    add("viewcos_998_above", F_IN_VIEW, (0.0, 0.0, 2.0), (0.3, 0.0, hi998), radius=2.5 * float(SF[4]))
    # predicted level: ceil(log(maxDist / dist) / log 1.2), clamped to [0, 7]
    # below 0 only where 1.2f * maxDist rounds up (3.5: 4.2000003), so that dist == maxDistance gives a ratio below 1 / 1.2f: -1.0000002 -> level -1 -> 0
    add("level_clamped_at_0", F_IN_VIEW, (0.0, 0.0, f32(1.2) * f32(3.5)), maxD=3.5, minD=2.0, shift=False, minLevel=-1, maxLevel=0, radius=2.5)
    add("level_clamped_at_top", F_IN_VIEW, (0.0, 0.0, 1.0), maxD=64.0, minD=0.5, minLevel=6, maxLevel=7, radius=2.5 * float(SF[7]))             # 22.8 -> 7
    add("level_ratio_1.2", F_IN_VIEW, (0.0, 0.0, 1.0), maxD=f32(1.2), minD=0.5, minLevel=0, maxLevel=1)                                       # log(1.2f) / log(1.2f) = 1 exactly
    add("level_ratio_1.44", F_IN_VIEW, (0.0, 0.0, 1.0), maxD=f32(1.2) * f32(1.2), minD=0.5)                                                   # 2 within an ulp: whichever side
    add("level_ratio_1", F_IN_VIEW, (0.0, 0.0, 2.0), maxD=2.0, minD=0.5, minLevel=-1, maxLevel=0)                                             # log 1 = 0: level 0, no clamp
    add("obs_off", F_IN_VIEW, (0.5, 0.25, 2.0), obs=0, flags=1)
    add("obs_on", F_IN_VIEW, (0.5, 0.25, 2.0), obs=1, flags=3)
    n = len(rows)
    desc = (np.arange(n * 32).reshape(n, 32) % 251 + 1).astype(np.uint8)        # no zero byte: a zeroed descriptor shows
    return dict(names=[r["name"] for r in rows], codes=[r["code"] for r in rows], Pw=np.array([r["P"] for r in rows], f32), Pn=np.array([r["Pn"] for r in rows], f32),
                maxD=np.array([r["maxD"] for r in rows], f32), minD=np.array([r["minD"] for r in rows], f32), obs=np.array([r["obs"] for r in rows], np.uint8), desc=desc,
                expect={r["name"]: r["expect"] for r in rows}, shiftable=np.array([r["shift"] for r in rows]))


def frustum_frames():
    """The frames the cases are run as: (name, Tcw, th, row indices, Pw).  The table's pose with th = 1 (every row decides as the table says), every other row against
    the plain identity with th = 3 (there the -0.0 rows see PcZ = +0.0), and the rows whose coordinates allow it against a
    pose with the camera centre at F_POSE_SHIFT (same camera coordinates, so the same records) with th = 0.75."""
    c = cached(frustum_cases)
    every = np.arange(len(c["names"]))
    sh = every[c["shiftable"]]
    T = np.eye(4, dtype=f32)
    T[:3, 3] = -F_POSE_SHIFT
    Pw_shift = (c["Pw"][sh].astype(f64) + F_POSE_SHIFT).astype(f32)
    assert np.array_equal(Pw_shift.astype(f64) - F_POSE_SHIFT, c["Pw"][sh].astype(f64))          # exact
    return [("negzero_th1", F_POSE_NEGZERO, f32(1.0), every, c["Pw"]), ("identity_th3", np.eye(4, dtype=f32), f32(3.0), every[::2], c["Pw"][::2]),
            ("shifted_th075", T, f32(0.75), sh, Pw_shift)]


def frustum_args(c, rows, Pw, Tcw, th):
    return (Pw, c["Pn"][rows], c["maxD"][rows], c["minD"][rows], c["obs"][rows], c["desc"][rows], Tcw, F_K5, F_BOUNDS, F_COSLIMIT, F_LOGSF, SF, th)
