"""Shared by tests/test_pnp_cpu.py and tests/test_pnp_gpu.py: a numpy restatement of ORB_SLAM2::PnPsolver (src/PnPsolver.cc) — SetRansacParameters,
the counter-based generator and draw rule of include/oslam_hip.h, compute_pose (EPnP), CheckInliers and the control flow of iterate — and the scene
generator of the PnP tests.  Independent of the library: nothing here calls it."""
import math

import numpy as np

TUM1 = (517.306408, 516.469215, 318.643040, 255.313989)
REF = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991)
f32 = np.float32


def ransac_params(N, probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5):
    """src/PnPsolver.cc:121-157 with its mixed arithmetic: (min_inliers, epsilon, iterations, no_more)."""
    eps = f32(epsilon)
    n_min = int(f32(N) * eps)                       # int nMinInliers = N*mRansacEpsilon (float product, truncated)
    n_min = max(n_min, min_inliers, min_set)
    no_more = N < n_min
    if N > 0 and eps < f32(n_min) / f32(N):
        eps = f32(n_min) / f32(N)
    if no_more:
        return n_min, float(eps), 0, True
    if n_min == N:
        it = 1
    else:
        d = math.log(1 - probability) / math.log(1 - math.pow(float(eps), 3))
        it = int(math.ceil(d))
    return n_min, float(eps), max(1, min(it, max_iterations)), False


def _mix(x):
    x &= 0xffffffff
    x ^= x >> 16; x = (x * 0x85EBCA6B) & 0xffffffff
    x ^= x >> 13; x = (x * 0xC2B2AE35) & 0xffffffff
    x ^= x >> 16
    return x


def pnp_hash(seed, iteration, draw):
    return _mix(_mix((seed + 0x9E3779B9 * (iteration + 1)) & 0xffffffff) ^ ((0x85EBCA6B * (draw + 1)) & 0xffffffff))


def swap_with_back(N, randis):
    """src/PnPsolver.cc:188-201 with the list spelled out: entry randi is taken, the last entry moves into its place."""
    avail = list(range(N))
    out = []
    for r in randis:
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


def draw(seed, iteration, N):
    return swap_with_back(N, [(pnp_hash(seed, iteration, k) * (N - k)) >> 32 for k in range(4)])


def compute_pose(pw, us, K, eig="eigh"):
    """src/PnPsolver.cc:477-525 in float64: (mean reprojection error, R, t).  eig: "eigh" or "svd" for the eigenvectors of MtM."""
    pw, us = np.asarray(pw, np.float64), np.asarray(us, np.float64)
    fu, fv, uc, vc = [float(k) for k in K]
    n = len(pw)
    c0 = pw.sum(0) / n
    P = pw - c0
    U, D, _ = np.linalg.svd(P.T @ P)
    for i in range(3):   # normalisation 6 of include/oslam_hip.h: the largest component of a PCA axis is positive (the first of equals)
        if U[np.argmax(np.abs(U[:, i])), i] < 0:
            U[:, i] = -U[:, i]
    cws = np.vstack([c0] + [c0 + np.sqrt(D[i] / n) * U[:, i] for i in range(3)])
    ci = np.linalg.pinv((cws[1:] - cws[0]).T)
    a = np.zeros((n, 4))
    a[:, 1:] = (pw - cws[0]) @ ci.T
    a[:, 0] = 1 - a[:, 1] - a[:, 2] - a[:, 3]
    M = np.zeros((2 * n, 12))
    for i in range(4):
        M[0::2, 3 * i] = a[:, i] * fu; M[0::2, 3 * i + 2] = a[:, i] * (uc - us[:, 0])
        M[1::2, 3 * i + 1] = a[:, i] * fv; M[1::2, 3 * i + 2] = a[:, i] * (vc - us[:, 1])
    MtM = M.T @ M
    if eig == "svd":
        ut = np.linalg.svd(MtM)[0].T
    else:
        ut = np.linalg.eigh(MtM)[1][:, ::-1].T
    v = [ut[11], ut[10], ut[9], ut[8]]
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    dv = np.array([[vi[3 * p:3 * p + 3] - vi[3 * q:3 * q + 3] for (p, q) in pairs] for vi in v])
    L = np.zeros((6, 10))
    for i in range(6):
        d = dv[:, i]
        L[i] = [d[0] @ d[0], 2 * d[0] @ d[1], d[1] @ d[1], 2 * d[0] @ d[2], 2 * d[1] @ d[2], d[2] @ d[2], 2 * d[0] @ d[3], 2 * d[1] @ d[3], 2 * d[2] @ d[3], d[3] @ d[3]]
    rho = np.array([((cws[p] - cws[q]) ** 2).sum() for (p, q) in pairs])
    solve = lambda A, b: np.linalg.lstsq(A, b, rcond=None)[0]

    def b1():
        b = solve(L[:, [0, 1, 3, 6]], rho); s = -1 if b[0] < 0 else 1
        b0 = np.sqrt(s * b[0])
        return np.array([b0, s * b[1] / b0, s * b[2] / b0, s * b[3] / b0])

    def b23(cols):
        b = solve(L[:, cols], rho)
        if b[0] < 0:
            b0 = np.sqrt(-b[0]); bb = np.sqrt(-b[2]) if b[2] < 0 else 0.
        else:
            b0 = np.sqrt(b[0]); bb = np.sqrt(b[2]) if b[2] > 0 else 0.
        if b[1] < 0:
            b0 = -b0
        return np.array([b0, bb, b[3] / b0 if len(cols) == 5 else 0., 0.])

    def gn(be):
        be = be.copy()
        for _ in range(5):
            A = np.zeros((6, 4)); r = np.zeros(6)
            for i in range(6):
                l = L[i]
                A[i] = [2 * l[0] * be[0] + l[1] * be[1] + l[3] * be[2] + l[6] * be[3], l[1] * be[0] + 2 * l[2] * be[1] + l[4] * be[2] + l[7] * be[3],
                        l[3] * be[0] + l[4] * be[1] + 2 * l[5] * be[2] + l[8] * be[3], l[6] * be[0] + l[7] * be[1] + l[8] * be[2] + 2 * l[9] * be[3]]
                r[i] = rho[i] - (l[0] * be[0] ** 2 + l[1] * be[0] * be[1] + l[2] * be[1] ** 2 + l[3] * be[0] * be[2] + l[4] * be[1] * be[2] + l[5] * be[2] ** 2
                                 + l[6] * be[0] * be[3] + l[7] * be[1] * be[3] + l[8] * be[2] * be[3] + l[9] * be[3] ** 2)
            be += solve(A, r)
        return be

    def Rt(be):
        ccs = sum(be[i] * v[i].reshape(4, 3) for i in range(4))
        pcs = a @ ccs
        if pcs[0, 2] < 0:
            pcs = -pcs
        pc0 = pcs.sum(0) / n; pw0 = pw.sum(0) / n
        U_, _, Vt_ = np.linalg.svd((pcs - pc0).T @ (pw - pw0))
        R = U_ @ Vt_
        if np.linalg.det(R) < 0:
            R[2] = -R[2]
        t = pc0 - R @ pw0
        pc = pw @ R.T + t
        e = np.sqrt((us[:, 0] - (uc + fu * pc[:, 0] / pc[:, 2])) ** 2 + (us[:, 1] - (vc + fv * pc[:, 1] / pc[:, 2])) ** 2).sum() / n
        return e, R, t

    with np.errstate(all="ignore"):
        res = [Rt(gn(b1())), Rt(gn(b23([0, 1, 2]))), Rt(gn(b23([0, 1, 2, 3, 4])))]
    k = 0
    if res[1][0] < res[0][0]:
        k = 1
    if res[2][0] < res[k][0]:
        k = 2
    return res[k]


def check_inliers(R, t, P3Dw, P2D, sigma2, K, th2):
    """src/PnPsolver.cc:308-339 with its float / double mix: the inlier flags."""
    fu, fv, uc, vc = [float(f32(k)) for k in K]
    P = np.asarray(P3Dw, f32).astype(np.float64)
    with np.errstate(all="ignore"):
        Xc = (R[0, 0] * P[:, 0] + R[0, 1] * P[:, 1] + R[0, 2] * P[:, 2] + t[0]).astype(f32)
        Yc = (R[1, 0] * P[:, 0] + R[1, 1] * P[:, 1] + R[1, 2] * P[:, 2] + t[1]).astype(f32)
        invZc = (1 / (R[2, 0] * P[:, 0] + R[2, 1] * P[:, 1] + R[2, 2] * P[:, 2] + t[2])).astype(f32)
        ue = uc + fu * Xc.astype(np.float64) * invZc.astype(np.float64)
        ve = vc + fv * Yc.astype(np.float64) * invZc.astype(np.float64)
        p2 = np.asarray(P2D, f32)
        dX = (p2[:, 0].astype(np.float64) - ue).astype(f32)
        dY = (p2[:, 1].astype(np.float64) - ve).astype(f32)
        e2 = dX * dX + dY * dY
        return e2 < np.asarray(sigma2, f32) * f32(th2)


def iterate(P3Dw, P2D, sigma2, K, seed, params=REF, samples=None):
    """iterate (src/PnPsolver.cc:165-258), one shot: dict(kind, nInliers, iterations, chosen, Tcw, inliers, counts)."""
    N = len(P3Dw)
    n_min, _, its, no_more = ransac_params(N, params["probability"], params["min_inliers"], params["max_iterations"], params["min_set"], params["epsilon"])
    out = dict(kind=0, nInliers=0, iterations=0, chosen=-1, Tcw=None, inliers=None, counts=[])
    if no_more:
        return out
    Kd = [float(f32(k)) for k in K]
    pw, us = np.asarray(P3Dw, f32).astype(np.float64), np.asarray(P2D, f32).astype(np.float64)
    T = lambda R, t: np.vstack([np.hstack([R, t[:, None]]), [[0, 0, 0, 1]]]).astype(f32)
    best, best_flags, best_T, best_it = 0, None, None, -1
    for it in range(its):
        s = list(samples[it]) if samples is not None else draw(seed, it, N)
        _, R, t = compute_pose(pw[s], us[s], Kd)
        flags = check_inliers(R, t, P3Dw, P2D, sigma2, K, params["th2"]) if np.isfinite(R).all() and np.isfinite(t).all() else np.zeros(N, bool)
        cnt = int(flags.sum())
        out["counts"].append(cnt)
        if cnt >= n_min:
            if cnt > best:
                best, best_flags, best_T, best_it = cnt, flags, T(R, t), it
            idx = np.nonzero(best_flags)[0]
            _, Rr, tr = compute_pose(pw[idx], us[idx], Kd)
            rf = check_inliers(Rr, tr, P3Dw, P2D, sigma2, K, params["th2"])
            if int(rf.sum()) > n_min:
                out.update(kind=1, nInliers=int(rf.sum()), iterations=it + 1, chosen=best_it, Tcw=T(Rr, tr), inliers=rf)
                return out
    out["iterations"] = its
    if best >= n_min:
        out.update(kind=2, nInliers=best, chosen=best_it, Tcw=best_T, inliers=best_flags)
    return out


def rodrigues(ax):
    th = np.linalg.norm(ax)
    if th == 0:
        return np.eye(3)
    k = ax / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def make_scene(seed, N, outlier_frac=0.0, noise=0.0, K=TUM1):
    """N correspondences of one camera: points in a box 2-6 m in front of the camera, a pose of up to 0.3 rad and 0.3 m, inputs rounded to float32,
    sigma2 = 1.2^(2 octave) with octaves 0..7, `outlier_frac` of the observations redrawn until they lie at least 20 px from the true projection (so the true
    inlier set is unambiguous at th2 = 5.991).  dict(P3Dw, P2D, sigma2, truth (bool), R, t, K, depth)."""
    rng = np.random.default_rng(seed)
    fu, fv, uc, vc = K
    ax = rng.normal(size=3)
    ax *= rng.uniform(0.05, 0.3) / np.linalg.norm(ax)
    R = rodrigues(ax)
    t = rng.uniform(-0.3, 0.3, 3)
    pc = rng.uniform([-1.5, -1.0, 2.0], [1.5, 1.0, 6.0], (N, 3))     # camera frame: in front of the camera by construction
    pw = (pc - t) @ R                                                # Xw = R^T (Xc - t)
    pw = pw.astype(f32)
    pcd = pw.astype(np.float64) @ R.T + t
    proj = np.stack([uc + fu * pcd[:, 0] / pcd[:, 2], vc + fv * pcd[:, 1] / pcd[:, 2]], 1)
    us = proj + (rng.normal(0, noise, proj.shape) if noise > 0 else 0.0)
    truth = np.ones(N, bool)
    n_out = int(round(outlier_frac * N))
    for i in rng.permutation(N)[:n_out]:
        while True:
            cand = rng.uniform([0, 0], [640, 480])
            if np.hypot(*(cand - proj[i])) >= 20.0:
                break
        us[i] = cand
        truth[i] = False
    octave = rng.integers(0, 8, N)
    sigma2 = (f32(1.2) ** (2 * octave)).astype(f32)
    return dict(P3Dw=pw, P2D=us.astype(f32), sigma2=sigma2, truth=truth, R=R, t=t, K=tuple(float(f32(k)) for k in K), depth=float(pcd[:, 2].mean()) if N else 4.0)
