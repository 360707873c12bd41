"""Shared by tests/test_sim3_cpu.py and tests/test_sim3_gpu.py: a numpy restatement of ORB_SLAM2::Sim3Solver (src/Sim3Solver.cc) — SetRansacParameters,
the three-index draw with the generator of include/oslam_hip.h, ComputeSim3 (Horn in float64, rounded to float32 where the reference stores CV_32F),
CheckInliers with the truncated thresholds and float arithmetic, iterate with resumable state — the scene generator of the Sim3 tests, and the scenes,
seeds and rule of the hypothesis-parity test.  Independent of the library: nothing here calls it."""
import functools
import math

import numpy as np

from pnp_common import pnp_hash, rodrigues, swap_with_back

TUM1 = (517.306408, 516.469215, 318.643040, 255.313989)
REF = dict(probability=0.99, min_inliers=20, max_iterations=300)   # src/LoopClosing.cc:276
f32 = np.float32


def ransac_params(N, probability=0.99, min_inliers=20, max_iterations=300):
    """src/Sim3Solver.cc:114-138 with its mixed arithmetic: (iterations, no_more).  N < 3 is no_more too (normalisation 4 of include/oslam_hip.h)."""
    if N < min_inliers or N < 3:
        return 0, True
    if min_inliers == N:
        it = 1
    else:
        eps = f32(min_inliers) / f32(N)                       # float epsilon = (float)mRansacMinInliers/N
        den = math.log(1 - math.pow(float(eps), 3))
        d = -math.inf if den == 0 else math.ceil(math.log(1 - probability) / den)
        it = 1 if d < 1 else (max_iterations if d >= max_iterations else int(d))
    return max(1, min(it, max_iterations)), False


def draw(seed, iteration, N):
    """The three indices of src/Sim3Solver.cc:163-177 with the counter-based generator."""
    return swap_with_back(N, [(pnp_hash(seed, iteration, k) * (N - k)) >> 32 for k in range(3)])


def compute_sim3(P1, P2, fix_scale):
    """src/Sim3Solver.cc:226-316 for three point pairs ([point][coordinate]): Horn in float64 from the float32 inputs; R, then s, then t rounded to float32.
    Returns (R, t, s, gap): gap = the difference of the two largest eigenvalues of N relative to the largest magnitude."""
    P1, P2 = np.asarray(P1, f32).astype(np.float64), np.asarray(P2, f32).astype(np.float64)
    O1 = (P1[0] + P1[1] + P1[2]) / 3.0
    O2 = (P2[0] + P2[1] + P2[2]) / 3.0
    Pr1, Pr2 = P1 - O1, P2 - O2
    M = np.array([[Pr2[0, i] * Pr1[0, j] + Pr2[1, i] * Pr1[1, j] + Pr2[2, i] * Pr1[2, j] for j in range(3)] for i in range(3)])   # Pr2 * Pr1^T
    N = np.zeros((4, 4))
    N[0, 0] = M[0, 0] + M[1, 1] + M[2, 2]
    N[0, 1] = M[1, 2] - M[2, 1]
    N[0, 2] = M[2, 0] - M[0, 2]
    N[0, 3] = M[0, 1] - M[1, 0]
    N[1, 1] = M[0, 0] - M[1, 1] - M[2, 2]
    N[1, 2] = M[0, 1] + M[1, 0]
    N[1, 3] = M[2, 0] + M[0, 2]
    N[2, 2] = -M[0, 0] + M[1, 1] - M[2, 2]
    N[2, 3] = M[1, 2] + M[2, 1]
    N[3, 3] = -M[0, 0] - M[1, 1] + M[2, 2]
    N = N + np.triu(N, 1).T
    bad = (np.full((3, 3), np.nan, f32), np.full(3, np.nan, f32), f32(np.nan), 0.0)
    if not np.isfinite(N).all():
        return bad
    w, V = np.linalg.eigh(N)
    scale = np.abs(w).max()
    gap = (w[3] - w[2]) / scale if scale > 0 else 0.0
    q = V[:, 3]
    with np.errstate(all="ignore"):
        nrm = math.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
        ang = math.atan2(nrm, q[0])
        if nrm == 0:
            return bad[:3] + (gap,)                              # vec / norm(vec) is 0 / 0 in the reference
        r = np.array([2 * ang * q[1] / nrm, 2 * ang * q[2] / nrm, 2 * ang * q[3] / nrm])
        theta = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
        if theta < np.finfo(np.float64).eps:                     # cv::Rodrigues
            R = np.eye(3)
        else:
            c, s, c1 = math.cos(theta), math.sin(theta), 1.0 - math.cos(theta)
            r = r * (1.0 / theta)
            rx = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
            R = (c * np.eye(3) + c1 * np.outer(r, r)) + s * rx
        Rf = R.astype(f32)
        Rd = Rf.astype(np.float64)
        if fix_scale:
            sf = f32(1.0)
        else:
            nom = den = 0.0
            for i in range(3):
                for k in range(3):
                    p3 = Rd[i, 0] * Pr2[k, 0] + Rd[i, 1] * Pr2[k, 1] + Rd[i, 2] * Pr2[k, 2]
                    nom += Pr1[k, i] * p3
                    den += p3 * p3
            sf = f32(nom / den) if den != 0 else f32(np.nan if nom == 0 else math.copysign(np.inf, nom))
        sd = float(sf)
        t = np.array([O1[i] - (((sd * Rd[i, 0]) * O2[0] + (sd * Rd[i, 1]) * O2[1]) + (sd * Rd[i, 2]) * O2[2]) for i in range(3)])
    return Rf, t.astype(f32), sf, gap


def transforms(R, t, s):
    """src/Sim3Solver.cc:318-336 in float32: the first three rows of T12 = [sR | t] and T21 = [(1 / s) R^T | -(1 / s) R^T t]."""
    R, t, s = np.asarray(R, f32), np.asarray(t, f32), f32(s)
    with np.errstate(all="ignore"):
        inv = f32(1.0 / float(s)) if s != 0 else f32(math.copysign(np.inf, float(s)))
        sR = (s * R).astype(f32)
        sRinv = (inv * R.T).astype(f32)
        tinv = -((sRinv[:, 0] * t[0] + sRinv[:, 1] * t[1]) + sRinv[:, 2] * t[2])
    return np.hstack([sR, t[:, None]]).astype(f32), np.hstack([sRinv, tinv[:, None]]).astype(f32)


def to_image(X, K):
    """FromCameraToImage (src/Sim3Solver.cc:405-423), float32."""
    fx, fy, cx, cy = [f32(k) for k in K]
    X = np.asarray(X, f32)
    with np.errstate(all="ignore"):
        invz = f32(1.0) / X[:, 2]
        return np.stack([fx * (X[:, 0] * invz) + cx, fy * (X[:, 1] * invz) + cy], 1)


def project(X, T, K):
    """Project (src/Sim3Solver.cc:382-403), float32; T = three rows of a transform."""
    X = np.asarray(X, f32)
    with np.errstate(all="ignore"):
        Xc = np.stack([((T[i, 0] * X[:, 0] + T[i, 1] * X[:, 1]) + T[i, 2] * X[:, 2]) + T[i, 3] for i in range(3)], 1)
    return to_image(Xc, K)


def max_errors(sigma2):
    """mvnMaxError (src/Sim3Solver.cc:87-88): 9.210 * sigmaSquare as a double product, truncated by the push into a vector<size_t>; float32 for the comparison."""
    return np.floor(9.210 * np.asarray(sigma2, f32).astype(np.float64)).astype(f32)


def check_inliers(R, t, s, sc):
    """CheckInliers (src/Sim3Solver.cc:340-364): (flags, err1, err2) in float32; the comparison is strict on both sides."""
    T12, T21 = transforms(R, t, s)
    with np.errstate(all="ignore"):
        d1 = to_image(sc["X1"], sc["K1"]) - project(sc["X2"], T12, sc["K1"])
        d2 = project(sc["X1"], T21, sc["K2"]) - to_image(sc["X2"], sc["K2"])
        e1 = d1[:, 0] * d1[:, 0] + d1[:, 1] * d1[:, 1]
        e2 = d2[:, 0] * d2[:, 0] + d2[:, 1] * d2[:, 1]
        return (e1 < max_errors(sc["sigma2_1"])) & (e2 < max_errors(sc["sigma2_2"])), e1, e2


def undetermined(gap, e1, e2, sc):
    """The rule of the parity test: a count that a rounding may move (an error within 1e-3 of its threshold, relatively, on either side) or a
    hypothesis the eigen-solver chooses (relative gap of the two largest eigenvalues of N below 1e-6)."""
    m1, m2 = max_errors(sc["sigma2_1"]).astype(np.float64), max_errors(sc["sigma2_2"]).astype(np.float64)
    with np.errstate(all="ignore"):
        near = (np.abs(e1.astype(np.float64) - m1) <= 1e-3 * m1) | (np.abs(e2.astype(np.float64) - m2) <= 1e-3 * m2)
    return bool(near.any()) or not gap >= 1e-6


class Solver:
    """Sim3Solver with its state (mnIterations, mnBestInliers, the best transform): iterate(n) resumes.  `log` gets one record per evaluated iteration:
    dict(it, count, R, t, s, undetermined)."""

    def __init__(self, scene, seed, params=REF, samples=None):
        self.sc, self.seed, self.params, self.samples = scene, seed, params, samples
        self.N = len(scene["sigma2_1"])
        self.iterations, self.never = ransac_params(self.N, params["probability"], params["min_inliers"], params["max_iterations"])
        if not all(np.isfinite(np.asarray(scene[k], np.float64)).all() for k in ("X1", "X2", "sigma2_1", "sigma2_2", "K1", "K2")):
            self.never = True                                   # normalisation 4
        self.iterations_done, self.best_inliers, self.best_iteration = 0, 0, -1
        self.R, self.t, self.s = np.zeros((3, 3), f32), np.zeros(3, f32), f32(0)
        self.log = []

    def iterate(self, n):
        out = dict(returned=0, nInliers=0, ran=0, no_more=0, T12=None, inliers=None)
        if self.never:
            out["no_more"] = 1
            return out
        sc = self.sc
        while self.iterations_done < self.iterations and out["ran"] < n:
            it = self.iterations_done
            out["ran"] += 1
            self.iterations_done += 1
            idx = list(self.samples[it]) if self.samples is not None else draw(self.seed, it, self.N)
            R, t, s, gap = compute_sim3(sc["X1"][idx], sc["X2"][idx], sc["fix_scale"])
            finite = bool(np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(s))
            flags, e1, e2 = check_inliers(R, t, s, sc)
            cnt = int(flags.sum()) if finite else 0
            self.log.append(dict(it=it, count=cnt, R=R, t=t, s=s, undetermined=(not finite) or undetermined(gap, e1, e2, sc)))
            if finite and cnt >= self.best_inliers:             # (a hypothesis that is not finite never becomes the best: normalisation 3)
                self.best_inliers, self.best_iteration, self.R, self.t, self.s = cnt, it, R, t, s
                if cnt > self.params["min_inliers"]:
                    T12 = np.vstack([transforms(R, t, s)[0], np.array([[0, 0, 0, 1]], f32)])
                    out.update(returned=1, nInliers=cnt, T12=T12, inliers=flags)
                    return out
        if self.iterations_done >= self.iterations:
            out["no_more"] = 1
        return out


def run_budget(scene, seed, chunk, params=REF, samples=None):
    """iterate(chunk) until bNoMore: (the solver, the list of (returning iteration, nInliers, T12, inliers))."""
    S = Solver(scene, seed, params, samples)
    returns = []
    while True:
        r = S.iterate(chunk)
        if r["returned"]:
            returns.append((S.iterations_done - 1, r["nInliers"], r["T12"], r["inliers"]))
        if r["no_more"]:
            return S, returns


def make_scene(seed, N, outlier_frac=0.0, scale=None, K=TUM1):
    """N point pairs: X2 in a box 2-6 m in front of camera 2, X1 = s R X2 + t with a rotation of at most 0.4 rad, |t_i| <= 0.3 m and s = 1 (scale None:
    the problem fixes the scale) or `scale`; inputs rounded to float32; sigma2 = 1.2^(2 octave), octaves 0..7 per side; `outlier_frac` of the X1 replaced
    by points whose image in camera 1 lies at least 40 px from the true one, so that the true inlier set is unambiguous (the largest threshold is 118 px^2)."""
    rng = np.random.default_rng(seed)
    fu, fv, uc, vc = K
    ax = rng.normal(size=3)
    ax *= rng.uniform(0.05, 0.4) / np.linalg.norm(ax)
    R = rodrigues(ax)
    t = rng.uniform(-0.3, 0.3, 3)
    s = 1.0 if scale is None else float(scale)
    box = ([-1.5, -1.0, 2.0], [1.5, 1.0, 6.0])
    X2 = rng.uniform(*box, (N, 3)).astype(f32)
    X1d = s * (X2.astype(np.float64) @ R.T) + t
    img = lambda X: np.stack([uc + fu * X[:, 0] / X[:, 2], vc + fv * X[:, 1] / X[:, 2]], 1)
    truth = np.ones(N, bool)
    for i in rng.permutation(N)[:int(round(outlier_frac * N))]:
        while True:
            cand = rng.uniform(*box)
            if np.hypot(*(img(cand[None])[0] - img(X1d[i:i + 1])[0])) >= 40.0:
                break
        X1d[i] = cand
        truth[i] = False
    o1, o2 = rng.integers(0, 8, N), rng.integers(0, 8, N)
    Kf = tuple(float(f32(k)) for k in K)
    return dict(X1=X1d.astype(f32), X2=X2, sigma2_1=(f32(1.2) ** (2 * o1)).astype(f32), sigma2_2=(f32(1.2) ** (2 * o2)).astype(f32), truth=truth, R=R, t=t, s=s,
                fix_scale=scale is None, K1=Kf, K2=Kf, depth=float(X2[:, 2].mean()) if N else 4.0)


# ---- the batch of the GPU tests: counts that straddle a wave (65), four waves (257), the strict `> minInliers` edge (21, 20), no_more (19, 3) and empty ----
PARITY_COUNTS = (257, 65, 60, 60, 25, 21, 20, 19, 3, 0)
PARITY_OUTLIERS = (0.2, 0.2, 0.2, 0.5, 0.12, 0.0, 0.0, 0.0, 0.0, 0.0)
PARITY_SCALES = (None, 1.3, None, 1.3, 1.3, None, 1.3, None, 1.3, None)   # None: fix_scale
PARITY_SEEDS = tuple(2000 + i for i in range(len(PARITY_COUNTS)))
PARITY_CHUNK = 300


@functools.lru_cache(maxsize=None)
def parity_scenes():
    return tuple(make_scene(300 + i, N, outlier_frac=f, scale=sc) for i, (N, f, sc) in enumerate(zip(PARITY_COUNTS, PARITY_OUTLIERS, PARITY_SCALES)))


@functools.lru_cache(maxsize=None)
def parity_reference():
    """The restatement over the whole budget of every problem of the batch, computed once: a tuple of (solver, returns) (run_budget).  Read only."""
    return tuple(run_budget(sc, seed, PARITY_CHUNK) for sc, seed in zip(parity_scenes(), PARITY_SEEDS))
