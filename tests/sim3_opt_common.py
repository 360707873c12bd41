"""Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1046-1241) restated in numpy fp64 from the reference text and the published ORB_SLAM2
Thirdparty/g2o sources (sim3.h, types_seven_dof_expmap, base_binary_edge.hpp, optimization_algorithm_levenberg.cpp), a generator of problems with a
known Sim3 on the geometry of sim3_match_common.make_pair, and hand-built cases with known answers.  Shared by test_sim3_opt_cpu.py (which pins the
restatement against independent facts) and test_sim3_opt_gpu.py (which compares the kernel with it).  Never imports the product's kernels."""
import math

import numpy as np

import sim3_match_common as smc

f32, f64 = np.float32, np.float64
TH2 = f32(10.0)          # src/LoopClosing.cc:327
K = np.array(smc.CAM, f32)
EPS = 0.00001
DELTA = 1e-9
DBL_MAX = 1.7976931348623157e308


# ---------------------------------------------------------------------------------------------------------------------------------------------
# g2o::Sim3 on Eigen::Quaterniond.  A Sim3 is (q = [x, y, z, w], t [3], s); scalars are Python floats (IEEE binary64, one rounding per operator).
def quat_from_R(m):
    """Eigen's matrix -> quaternion; m row-major [9]"""
    m = [float(v) for v in np.asarray(m).reshape(9)]
    q = [0.0] * 4
    t = m[0] + m[4] + m[8]
    if t > 0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[7] - m[5]) * t
        q[1] = (m[2] - m[6]) * t
        q[2] = (m[3] - m[1]) * t
    else:
        i = 0
        if m[4] > m[0]:
            i = 1
        if m[8] > m[i * 3 + i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(m[i * 3 + i] - m[j * 3 + j] - m[k * 3 + k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k * 3 + j] - m[j * 3 + k]) * t
        q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t
        q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t
    return q


def quat_to_R(q):
    """Eigen's toRotationMatrix, row-major [9]"""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)]


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz]


def quat_rot(q, v):
    """Eigen's quaternion * vector; v = three scalars or three arrays"""
    uv0, uv1, uv2 = q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]
    uv0, uv1, uv2 = uv0 + uv0, uv1 + uv1, uv2 + uv2
    return [v[0] + q[3] * uv0 + (q[1] * uv2 - q[2] * uv1), v[1] + q[3] * uv1 + (q[2] * uv0 - q[0] * uv2), v[2] + q[3] * uv2 + (q[0] * uv1 - q[1] * uv0)]


def exp_branch(u):
    """which of the four bodies of Sim3(Vector7d) the update takes: (|sigma| < eps, theta < eps)"""
    theta = math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    return abs(u[6]) < EPS, theta < EPS


def sim3_exp(u):
    """Sim3(const Vector7d& update): (omega, upsilon, sigma)"""
    u = [float(v) for v in u]
    wx, wy, wz, sigma = u[0], u[1], u[2], u[6]
    theta = math.sqrt(wx * wx + wy * wy + wz * wz)
    W = [0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0]
    W2 = [W[i * 3] * W[j] + W[i * 3 + 1] * W[3 + j] + W[i * 3 + 2] * W[6 + j] for i in range(3) for j in range(3)]
    s = math.exp(sigma)
    small = theta < EPS
    if abs(sigma) < EPS:
        C = 1.0
        if small:
            A, B = 1. / 2., 1. / 6.
        else:
            theta2 = theta * theta
            A = (1 - math.cos(theta)) / theta2
            B = (theta - math.sin(theta)) / (theta2 * theta)
    else:
        C = (s - 1) / sigma
        sigma2 = sigma * sigma
        if small:
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)   # as published
        else:
            a, b = s * math.sin(theta), s * math.cos(theta)
            theta2 = theta * theta
            c = theta2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
    eye = [1.0 if i % 4 == 0 else 0.0 for i in range(9)]
    if small:
        R = [(eye[i] + W[i]) + W2[i] for i in range(9)]
    else:
        ra, rb = math.sin(theta) / theta, (1 - math.cos(theta)) / (theta * theta)
        R = [(eye[i] + ra * W[i]) + rb * W2[i] for i in range(9)]
    V = [(A * W[i] + B * W2[i]) + C * eye[i] for i in range(9)]
    t = [V[i * 3] * u[3] + V[i * 3 + 1] * u[4] + V[i * 3 + 2] * u[5] for i in range(3)]
    return quat_from_R(R), t, s


def sim3_mul(a, b):
    rt = quat_rot(a[0], b[1])
    return quat_mul(a[0], b[0]), [a[2] * rt[i] + a[1][i] for i in range(3)], a[2] * b[2]


def sim3_inv(a):
    q, t, s = a
    qc = [-q[0], -q[1], -q[2], q[3]]
    m = -1. / s
    return qc, quat_rot(qc, [m * t[0], m * t[1], m * t[2]]), 1. / s


def sim3_oplus(S, x, fix_scale):
    u = [float(v) for v in x]
    if fix_scale:
        u[6] = 0.0
    return sim3_mul(sim3_exp(u), S)


def sim3_from_floats(s12, R12, t12):
    """g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s) of float R, t, s"""
    return quat_from_R(np.asarray(R12, f32).astype(f64).reshape(9)), [float(v) for v in np.asarray(t12, f32).astype(f64)], float(f32(s12))


def sim3_record(S):
    """the 13 doubles of the ABI: R row-major, t, s"""
    return np.array(quat_to_R(S[0]) + list(S[1]) + [S[2]], f64)


def sim3_matrix(S):
    """the 4 x 4 matrix [sR | t] of a Sim3"""
    M = np.eye(4)
    M[:3, :3] = S[2] * np.array(quat_to_R(S[0])).reshape(3, 3)
    M[:3, 3] = S[1]
    return M


def edge_error(S, P, k4, obs):
    """obs - cam_map(project(S.map(P))); P, obs: arrays [N, 3], [N, 2]"""
    q, t, s = S
    r = quat_rot(q, [P[:, 0], P[:, 1], P[:, 2]])
    x, y, z = s * r[0] + t[0], s * r[1] + t[1], s * r[2] + t[2]
    with np.errstate(all="ignore"):
        return np.stack([obs[:, 0] - ((x / z) * k4[0] + k4[2]), obs[:, 1] - ((y / z) * k4[1] + k4[3])], 1)


def huber(e2, delta):
    """RobustKernelHuber::robustify: rho[0], rho[1]"""
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(e2)
        inl = e2 <= dsqr
        return np.where(inl, e2, 2 * sq * delta - dsqr), np.where(inl, 1.0, delta / sq)


def _seq_sum(terms, order, rows=None):
    """The sum of terms [m, 2, k] (per live pair: its e12 term, then its e21 term) over the pairs.  "forward" / "reversed": one after the other from 0.
    "wavefront": the kernel's own order (include/oslam_hip.h, "OptimizeSim3", normalisation 1) — lane l of 64 adds the pairs l, l + 64, ... of the problem
    in order (rows = the pairs' indices in the problem; a dropped pair adds nothing), then the xor butterfly 32, 16, 8, 4, 2, 1."""
    m, _, k = terms.shape
    if order == "wavefront":
        n_steps = (int(rows.max()) // 64 + 1) if m else 0
        T = np.zeros((n_steps, 64, 2, k))
        T[rows // 64, rows % 64] = terms
        acc = np.zeros((64, k))
        for step in range(n_steps):
            acc = acc + T[step, :, 0]
            acc = acc + T[step, :, 1]
        lanes = np.arange(64)
        for d in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[lanes ^ d]
        return acc[0]
    flat = terms.reshape(2 * m, k)
    if order == "reversed":
        flat = flat[::-1]
    if m == 0:
        return np.zeros(k)
    return np.add.accumulate(flat, axis=0)[-1]


def ldlt_solve(H, b, lam):
    """(H + lam I) x = b by an unpivoted LDL^T; (x, ok)"""
    n = 7
    L = [[0.0] * n for _ in range(n)]
    d = [0.0] * n
    ok = True
    with np.errstate(all="ignore"):
        for j in range(n):
            dj = float(H[j][j]) + lam
            for k in range(j):
                dj -= (L[j][k] * L[j][k]) * d[k]
            ok = ok and dj > 0 and math.isfinite(dj)
            d[j] = dj
            for i in range(j + 1, n):
                s = float(H[j][i])
                for k in range(j):
                    s -= (L[i][k] * L[j][k]) * d[k]
                L[i][j] = s / dj if dj != 0 else math.nan
        y = [0.0] * n
        for i in range(n):
            s = float(b[i])
            for k in range(i):
                s -= L[i][k] * y[k]
            y[i] = s
        x = [0.0] * n
        for i in range(n - 1, -1, -1):
            s = y[i] / d[i] if d[i] != 0 else math.nan
            for k in range(i + 1, n):
                s -= L[k][i] * x[k]
            x[i] = s
    return x, ok


class _Problem:
    def __init__(self, p):
        self.P1, self.P2 = np.asarray(p["X3Dc1"], f32).astype(f64).reshape(-1, 3), np.asarray(p["X3Dc2"], f32).astype(f64).reshape(-1, 3)
        self.o1, self.o2 = np.asarray(p["obs1"], f32).astype(f64).reshape(-1, 2), np.asarray(p["obs2"], f32).astype(f64).reshape(-1, 2)
        self.i1, self.i2 = np.asarray(p["invSigma2_1"], f32).astype(f64).reshape(-1), np.asarray(p["invSigma2_2"], f32).astype(f64).reshape(-1)
        self.K1, self.K2 = [float(v) for v in np.asarray(p["K1"], f32)], [float(v) for v in np.asarray(p["K2"], f32)]
        self.th2 = float(f32(p["th2"]))
        self.delta = float(np.sqrt(f32(p["th2"])))   # const float deltaHuber = sqrt(th2)
        self.fix = bool(p["fix_scale"])
        self.n = len(self.i1)

    def errors(self, S, live):
        """e12 [m, 2], e21 [m, 2] of the live edges at S"""
        return edge_error(S, self.P2[live], self.K1, self.o1[live]), edge_error(sim3_inv(S), self.P1[live], self.K2, self.o2[live])

    def chi2(self, S, live):
        e12, e21 = self.errors(S, live)
        i1, i2 = self.i1[live], self.i2[live]
        return (e12[:, 0] * i1) * e12[:, 0] + (e12[:, 1] * i1) * e12[:, 1], (e21[:, 0] * i2) * e21[:, 0] + (e21[:, 1] * i2) * e21[:, 1]

    def robust_chi2(self, S, live, order):
        c12, c21 = self.chi2(S, live)
        terms = np.stack([huber(c12, self.delta)[0], huber(c21, self.delta)[0]], 1)[:, :, None]   # e12 of a pair before its e21
        return float(_seq_sum(terms, order, np.nonzero(live)[0])[0])

    def jacobians(self, S, live):
        """BaseBinaryEdge::linearizeOplus, numeric: J12, J21 [m, 2, 7]"""
        scalar = 1.0 / (2 * DELTA)
        m = int(live.sum())
        J12, J21 = np.zeros((m, 2, 7)), np.zeros((m, 2, 7))
        for d in range(7):
            u = [0.0] * 7
            u[d] = DELTA
            ep12, ep21 = self.errors(sim3_oplus(S, u, self.fix), live)
            u[d] = -DELTA
            em12, em21 = self.errors(sim3_oplus(S, u, self.fix), live)
            J12[:, :, d], J21[:, :, d] = scalar * (ep12 - em12), scalar * (ep21 - em21)
        return J12, J21

    def build(self, S, live, order):
        """computeActiveErrors + activeRobustChi2 + buildSystem: F, H [7, 7], b [7]"""
        e12, e21 = self.errors(S, live)
        J12, J21 = self.jacobians(S, live)
        m = len(e12)
        terms = np.zeros((m, 2, 36))
        iu = np.triu_indices(7)
        for g, (e, J, info) in enumerate(((e12, J12, self.i1[live]), (e21, J21, self.i2[live]))):
            r0, r1 = huber((e[:, 0] * info) * e[:, 0] + (e[:, 1] * info) * e[:, 1], self.delta)
            w = r1 * info
            or0, or1 = (-(info * e[:, 0])) * r1, (-(info * e[:, 1])) * r1
            j0w, j1w = J[:, 0, :] * w[:, None], J[:, 1, :] * w[:, None]
            terms[:, g, :28] = j0w[:, iu[0]] * J[:, 0, iu[1]] + j1w[:, iu[0]] * J[:, 1, iu[1]]
            terms[:, g, 28:35] = J[:, 0, :] * or0[:, None] + J[:, 1, :] * or1[:, None]
            terms[:, g, 35] = r0
        acc = _seq_sum(terms, order, np.nonzero(live)[0])
        H = np.zeros((7, 7))
        H[iu] = acc[:28]
        H = H + np.triu(H, 1).T
        return float(acc[35]), H, acc[28:35]


def _optimize(pb, S, live, iterations, order, trace):
    """SparseOptimizer::optimize with OptimizationAlgorithmLevenberg.  Returns (estimate, estimate of the last trial, iterations run)."""
    S_last = S
    lam, ni = 0.0, 2.0
    done = 0
    for it in range(iterations):
        current, H, b = pb.build(S, live, order)
        if it == 0:
            lam = 1e-5 * max(abs(float(H[j][j])) for j in range(7))
            ni = 2.0
        rho, qmax = 0.0, 0
        while True:
            x, ok2 = ldlt_solve(H, b, lam)
            if not ok2:
                x = [0.0] * 7
            Sn = sim3_oplus(S, x, pb.fix)
            temp = pb.robust_chi2(Sn, live, order)
            S_last = Sn
            if not ok2:
                temp = DBL_MAX
            rho = current - temp
            scale = 0.0
            for k in range(7):
                scale += x[k] * (lam * x[k] + float(b[k]))
            scale += 1e-3
            rho /= scale
            accepted = rho > 0 and math.isfinite(temp)
            trace.append([current, temp, rho, lam, 1.0 if accepted else 0.0, 1.0 if (it == 0 and qmax == 0) else 0.0])
            if accepted:
                alpha = 1. - (2 * rho - 1) * (2 * rho - 1) * (2 * rho - 1)
                alpha = min(alpha, 2. / 3.)
                lam *= max(1. / 3., alpha)
                ni = 2.0
                current = temp
                S = Sn
            else:
                lam *= ni
                ni *= 2
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        done += 1
        if qmax == 10 or rho == 0:
            break
    return S, S_last, done


def _valid(p):
    vals = [np.asarray(p[k], f32).reshape(-1) for k in ("X3Dc1", "X3Dc2", "obs1", "obs2", "invSigma2_1", "invSigma2_2", "K1", "K2", "R12", "t12")]
    vals += [np.array([p["s12"], p["th2"]], f32)]
    return all(np.isfinite(v).all() for v in vals) and f32(p["s12"]) > 0


def optimize_sim3(p, order="forward"):
    """OptimizeSim3 of one problem p = dict(X3Dc1, X3Dc2, obs1, obs2, invSigma2_1, invSigma2_2, K1, K2, s12, R12, t12, th2, fix_scale).  Returns dict(ret,
    inliers [count] uint8, written, S12 [13] or None, nBad, iterations, trials, trace [trials][6], chi2 = [(chi2 of e12, chi2 of e21) of the live edges of each
    pass]).  order: the order of the sums over the edges — "forward", "reversed" or "wavefront" (the kernel's own, see _seq_sum)."""
    n = len(np.asarray(p["invSigma2_1"]).reshape(-1))
    out = dict(ret=0, inliers=np.zeros(n, np.uint8), written=False, S12=None, nBad=0, iterations=0, trials=0, trace=[], chi2=[], count=n)
    if not _valid(p):
        out["ret"] = -1
        return out
    if n == 0:
        return out
    pb = _Problem(p)
    S = sim3_from_floats(p["s12"], p["R12"], p["t12"])
    live = np.ones(n, bool)
    trace = []
    S, S_last, its = _optimize(pb, S, live, 5, order, trace)
    c12, c21 = pb.chi2(S_last, live)
    out["chi2"].append((c12, c21))
    bad = (c12 > pb.th2) | (c21 > pb.th2)
    live = ~bad
    nBad = int(bad.sum())
    out.update(nBad=nBad, inliers=live.astype(np.uint8), iterations=its, trials=len(trace), trace=trace)
    if n - nBad < 10:
        return out
    S, S_last, its2 = _optimize(pb, S, live, 10 if nBad > 0 else 5, order, trace)
    c12, c21 = pb.chi2(S_last, live)
    out["chi2"].append((c12, c21))
    keep = live.copy()
    keep[live] = ~((c12 > pb.th2) | (c21 > pb.th2))
    out.update(ret=int(keep.sum()), inliers=keep.astype(np.uint8), written=True, S12=sim3_record(S), iterations=its + its2, trials=len(trace))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# generated problems
def inv_level_sigma2(octave):
    """mvInvLevelSigma2 (src/ORBextractor.cc:431-436): 1.0f / (mvScaleFactor[i] * mvScaleFactor[i]) in float"""
    sf = smc.SF[np.asarray(octave)]
    return (f32(1.0) / (sf * sf)).astype(f32)


def make_problem(seed, count, fix_scale, outliers=0.1, noise=0.5, name=None):
    """`count` points seen by two cameras related by a known Sim3 (p_c1 = s R p_c2 + t, the geometry of sim3_match_common.make_pair; s = 1 with fix_scale).
    Observations are projections plus uniform noise of at most `noise` pixels times the scale of the keypoint's octave (so an inlier's chi2 stays below 1
    at the truth), the information is mvInvLevelSigma2 of the octave; `outliers` of the pairs have one observation moved by 25 to 60 pixels times that
    scale (gross: chi2 > 600).  The start is the truth turned by 2 degrees, moved by 2 % of the mean depth and, with a free scale, scaled by 1 +- 0.05."""
    rng = np.random.default_rng(seed)
    s = 1.0 if fix_scale else float(rng.uniform(0.8, 1.25))
    ax = rng.normal(size=3)
    R = smc.rodrigues(0.15 * ax / np.linalg.norm(ax))
    t = rng.uniform(-0.15, 0.15, 3)
    P1 = np.zeros((0, 3))
    while len(P1) < count:
        c = smc._frustum(rng, 4 * count + 16)
        c2 = (c - t) @ R / s
        P1 = np.concatenate([P1, c[smc._inside(smc._project(c2), c2, 4.0) & smc._inside(smc._project(c), c, 4.0)]])
    P1 = P1[:count]
    P2 = (P1 - t) @ R / s
    oct1, oct2 = rng.integers(0, smc.NLEVELS, count), rng.integers(0, smc.NLEVELS, count)
    sf1, sf2 = smc.SF[oct1].astype(f64), smc.SF[oct2].astype(f64)
    obs1 = smc._project(P1) + rng.uniform(-noise, noise, (count, 2)) * sf1[:, None]
    obs2 = smc._project(P2) + rng.uniform(-noise, noise, (count, 2)) * sf2[:, None]
    gross = np.zeros(count, bool)
    n_out = int(round(outliers * count)) if count >= 10 else 0
    gross[rng.permutation(count)[:n_out]] = True
    for i in np.nonzero(gross)[0]:
        ang, mag = rng.uniform(0, 2 * np.pi), rng.uniform(25.0, 60.0)
        if rng.integers(0, 2):
            obs1[i] += mag * sf1[i] * np.array([np.cos(ang), np.sin(ang)])
        else:
            obs2[i] += mag * sf2[i] * np.array([np.cos(ang), np.sin(ang)])
    pa = rng.normal(size=3)
    R0 = smc.rodrigues(np.deg2rad(2.0) * pa / np.linalg.norm(pa)) @ R
    pt = rng.normal(size=3)
    t0 = t + 0.02 * 7.0 * pt / np.linalg.norm(pt)
    s0 = s if fix_scale else s * (1.0 + 0.05 * (1 if rng.integers(0, 2) else -1))
    return dict(name=name or "generated_%d_%d%s" % (seed, count, "_fix" if fix_scale else ""), X3Dc1=P1.astype(f32), X3Dc2=P2.astype(f32), obs1=obs1.astype(f32),
                obs2=obs2.astype(f32), invSigma2_1=inv_level_sigma2(oct1), invSigma2_2=inv_level_sigma2(oct2), K1=K, K2=K, s12=f32(s0), R12=R0.astype(f32),
                t12=t0.astype(f32), th2=TH2, fix_scale=int(fix_scale), gross=gross, truth=(R, t, s))


def _exact(n, z=4.0, seed=7):
    """n pairs whose float coordinates project exactly (power-of-two intrinsics and depths) under the identity Sim3: zero error"""
    rng = np.random.default_rng(seed)
    u, v = rng.permutation(np.arange(40, 600, 8))[:n], rng.permutation(np.arange(40, 440, 8))[:n]
    zs = np.where(np.arange(n) % 2 == 0, z, 2 * z)
    P = np.stack([smc.point_at(u[i], v[i], zs[i]) for i in range(n)]).astype(f32)
    obs = np.stack([u, v], 1).astype(f32)
    return dict(X3Dc1=P.copy(), X3Dc2=P.copy(), obs1=obs.copy(), obs2=obs.copy(), invSigma2_1=np.ones(n, f32), invSigma2_2=np.ones(n, f32), K1=K, K2=K, s12=f32(1),
                R12=np.eye(3, dtype=f32), t12=np.zeros(3, f32), th2=TH2, fix_scale=0)


IDENTITY_RECORD = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1], f64)


def hand_cases():
    """Cases whose answer follows from the reference text alone.  expect: ret, and where known inliers, written, S12 (to 1e-12), nBad."""
    cases = []
    cases.append(dict(_exact(12), name="exact_12_fix", fix_scale=1, expect=dict(ret=12, inliers=[1] * 12, written=True, S12=IDENTITY_RECORD, nBad=0)))
    cases.append(dict(_exact(10), name="exact_10", expect=dict(ret=10, inliers=[1] * 10, written=True, S12=IDENTITY_RECORD, nBad=0)))
    o = dict(_exact(10), name="ten_one_gross")
    o["obs1"][3] += np.array([40.0, -30.0], f32)   # 50 pixels: chi2 = 2500; nine pairs are left, fewer than ten (:1211)
    o["expect"] = dict(ret=0, inliers=[1, 1, 1, 0, 1, 1, 1, 1, 1, 1], written=False, nBad=1)
    cases.append(o)
    # S12.map gives z = -2: the edges have no depth test, the mirrored projection (-0.5 * 512 + 320, -0.5 * 512 + 240) is what they compare with.  Observed
    # exactly there the pair has zero error and survives (a depth test would clear it); one pair is fewer than ten, so the call returns 0.
    b = dict(_exact(1), name="behind_camera")
    b["X3Dc1"] = b["X3Dc2"] = np.array([[1.0, 1.0, -2.0]], f32)
    b["obs1"] = b["obs2"] = np.array([[64.0, -16.0]], f32)
    b["expect"] = dict(ret=0, inliers=[1], written=False, nBad=0)
    cases.append(b)
    return cases


# The generated problems of the parity batch: (seed, count, fix_scale, outliers).  The counts are the wavefront and stride boundaries and the `< 10` gate; the
# last has no outliers, so its first pass has nBad == 0 (five more iterations instead of ten).  The seeds are chosen on the CPU (test_sim3_opt_cpu.py
# asserts it) so that no decision of the run — a chi2 against th2, the sign of a trial's rho — is within rounding noise of its threshold.  With a
# fixed scale the Gauss-Newton steps converge quadratically and every later trial has a rho of rounding noise, so the fixed-scale problems that run
# the second optimize are the exact hand-built ones; with a free scale the published exponential map (the B of its |sigma| >= eps, theta < eps branch)
# throws a step now and then, the damping rises, and all fifteen iterations make decided progress.
PARITY_SPECS = [(11, 0, 0, 0.1), (2, 1, 1, 0.1), (1, 9, 0, 0.1), (2, 10, 1, 0.1), (1, 11, 0, 0.1), (4, 63, 0, 0.1), (3, 64, 0, 0.1), (1, 65, 0, 0.1), (7, 129, 0, 0.1),
                (4, 300, 0, 0.1), (10, 2400, 0, 0.1), (1, 100, 0, 0.0)]
_cache = {}


def parity_problems():
    if "problems" not in _cache:
        _cache["problems"] = hand_cases() + [make_problem(s, n, fx, outliers=o) for s, n, fx, o in PARITY_SPECS]
    return _cache["problems"]


def reference_of(problems, key, order="forward"):
    """optimize_sim3 of every problem, computed once per key"""
    k = (key, order)
    if k not in _cache:
        _cache[k] = [optimize_sim3(p, order) for p in problems]
    return _cache[k]


def concat_batch(problems):
    """the packed arrays of a batch and the offsets of its problems"""
    cat = lambda k, w: np.concatenate([np.asarray(p[k], f32).reshape((-1, w) if w else (-1,)) for p in problems]) if problems else np.zeros((0, w) if w else (0,), f32)
    counts = np.array([len(np.asarray(p["invSigma2_1"]).reshape(-1)) for p in problems], np.int32)
    return dict(X3Dc1=cat("X3Dc1", 3), X3Dc2=cat("X3Dc2", 3), obs1=cat("obs1", 2), obs2=cat("obs2", 2), invSigma2_1=cat("invSigma2_1", 0), invSigma2_2=cat("invSigma2_2", 0)), counts


def sim3_error(rec, truth):
    """(largest |R - R*|, largest |t - t*|, |s / s* - 1|) of a 13-double record against (R, t, s)"""
    R, t, s = truth
    return float(np.abs(rec[:9].reshape(3, 3) - R).max()), float(np.abs(rec[9:12] - t).max()), abs(float(rec[12]) / s - 1.0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the caller's side (src/Optimizer.cc:1099-1137) on a keyframe pair of sim3_match_common.make_pair
INV_SIGMA2 = inv_level_sigma2(np.arange(smc.NLEVELS))   # mvInvLevelSigma2


def problem_of_pair(pair, vpMatches1, fix_scale):
    """The rows OptimizeSim3 builds from a pair and vpMatches1 (as SearchBySim3 leaves it: -1 = NULL, a value in [0, n2) = the map point of that keypoint of
    KF2, anything else = a map point without an index in KF2), and vnIndexEdge.  The camera-frame points are the float cv::Mat expression R X + t."""
    kf1, kf2 = pair["kf1"], pair["kf2"]
    n2 = len(kf2["has_mp"])
    m = np.asarray(vpMatches1)
    idx = np.array([i for i in range(len(m)) if 0 <= m[i] < n2 and kf1["has_mp"][i] and kf2["has_mp"][m[i]]], np.int64)
    k2 = m[idx].astype(np.int64)
    T1, T2 = np.asarray(pair["T1w"], f32), np.asarray(pair["T2w"], f32)
    p = dict(X3Dc1=smc._gemm(T1[:3, :3], kf1["Xw"][idx], T1[:3, 3]), X3Dc2=smc._gemm(T2[:3, :3], kf2["Xw"][k2], T2[:3, 3]),
             obs1=np.stack([kf1["keysUn"]["x"][idx], kf1["keysUn"]["y"][idx]], 1).astype(f32), obs2=np.stack([kf2["keysUn"]["x"][k2], kf2["keysUn"]["y"][k2]], 1).astype(f32),
             invSigma2_1=INV_SIGMA2[kf1["keysUn"]["octave"][idx]], invSigma2_2=INV_SIGMA2[kf2["keysUn"]["octave"][k2]], K1=K, K2=K, s12=pair["s12"], R12=pair["R12"],
             t12=pair["t12"], th2=TH2, fix_scale=int(fix_scale))
    return p, idx


def compute_sim3_step(pair, fix_scale):
    """SearchBySim3, OptimizeSim3 and the decision of src/LoopClosing.cc:324-330 on a pair: dict(nFound, nInliers, bMatch, vpMatches, S12 [13], result)"""
    match12, n_found = smc.run_pair(pair)
    vp = np.where(match12 >= 0, match12, pair["matched_in"]).astype(np.int32)
    p, idx = problem_of_pair(pair, vp, fix_scale)
    r = optimize_sim3(p)
    vp[idx[r["inliers"] == 0]] = -1
    S = r["S12"] if r["written"] else np.concatenate([np.asarray(pair["R12"], f32).astype(f64).reshape(9), np.asarray(pair["t12"], f32).astype(f64), [f64(f32(pair["s12"]))]])
    return dict(nFound=n_found, nInliers=max(r["ret"], 0), bMatch=r["ret"] >= 20, vpMatches=vp, S12=S, result=r, problem=p)
