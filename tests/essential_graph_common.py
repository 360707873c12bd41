"""Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:781-1044) restated in numpy fp64 from the reference text and the published ORB_SLAM2
Thirdparty/g2o sources (sim3.h, types_seven_dof_expmap, base_binary_edge.hpp, optimization_algorithm_levenberg.cpp, block_solver.hpp), on the Sim3 pieces
of sim3_opt_common.py; its edge selection and point correction; generators of drifted rings.  The system is assembled densely, edge after edge, and
solved with numpy.linalg.cholesky.  Shared by test_essential_graph_cpu.py (which pins the restatement against independent facts) and
test_essential_graph_gpu.py (which compares the kernel with it).  Never imports the product's kernels."""
import math

import numpy as np

import sim3_opt_common as soc

f32, f64 = np.float32, np.float64
EPS, DELTA, DBL_MAX = soc.EPS, soc.DELTA, soc.DBL_MAX
MIN_FEAT = 100


# ---------------------------------------------------------------------------------------------------------------------------------------------
# g2o::Sim3::log.  A Sim3 is (q = [x, y, z, w], t [3], s) as in sim3_opt_common; every component may be a scalar or an array (one entry per edge).
def log_branch(S):
    """which of the four bodies of Sim3::log the transform takes: (|sigma| < eps, d > 1 - eps)"""
    R = soc.quat_to_R(S[0])
    return abs(math.log(S[2])) < EPS, 0.5 * (R[0] + R[4] + R[8] - 1) > 1 - EPS


def sim3_log(S):
    """Sim3::log(): [..., 7] = (omega, upsilon, sigma)"""
    q, t, s = S
    s = np.asarray(s, f64)
    with np.errstate(all="ignore"):
        sigma = np.log(s)
        R = [np.asarray(v, f64) for v in soc.quat_to_R(q)]
        d = 0.5 * (R[0] + R[4] + R[8] - 1)
        dR = [R[7] - R[5], R[2] - R[6], R[3] - R[1]]
        small_s, small_r = np.abs(sigma) < EPS, d > 1 - EPS
        theta = np.arccos(d)
        theta2 = theta * theta
        f = np.where(small_r, 0.5, theta / (2 * np.sqrt(1 - d * d)))
        om = [f * v for v in dR]
        sigma2 = sigma * sigma
        C = np.where(small_s, 1.0, (s - 1) / sigma)
        a, b, c = s * np.sin(theta), s * np.cos(theta), theta2 + sigma * sigma
        A = np.where(small_s, np.where(small_r, 1. / 2., (1 - np.cos(theta)) / theta2),
                     np.where(small_r, ((sigma - 1) * s + 1) / sigma2, (a * sigma + (1 - b) * theta) / (theta * c)))
        B = np.where(small_s, np.where(small_r, 1. / 6., (theta - np.sin(theta)) / (theta2 * theta)),
                     np.where(small_r, ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma), (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2))   # as published
    z = np.zeros_like(d)
    O = np.stack([np.stack([z, -om[2], om[1]], -1), np.stack([om[2], z, -om[0]], -1), np.stack([-om[1], om[0], z], -1)], -2)
    W = A[..., None, None] * O + B[..., None, None] * (O @ O) + C[..., None, None] * np.eye(3)
    tt = np.stack([np.asarray(v, f64) + z for v in t], -1)
    ups = np.linalg.solve(W, tt[..., None])[..., 0]   # W.lu().solve(t): LAPACK's LU with row pivoting
    return np.concatenate([np.stack(om, -1), ups, (sigma + z)[..., None]], -1)


def sim3_log1(S):
    return [float(v) for v in sim3_log(S)]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# sets of Sim3 as arrays
def sims_from_floats(rec):
    """[n, 13] float32 (s, R row-major, t) -> list of Sim3, as g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s)"""
    rec = np.asarray(rec, f32).reshape(-1, 13)
    return [soc.sim3_from_floats(r[0], r[1:10], r[10:13]) for r in rec]


def _cols(sims, idx):
    """the Sim3s sims[idx] as one Sim3 of arrays"""
    Q = np.array([sims[i][0] for i in idx], f64).reshape(-1, 4)
    T = np.array([sims[i][1] for i in idx], f64).reshape(-1, 3)
    return [Q[:, 0], Q[:, 1], Q[:, 2], Q[:, 3]], [T[:, 0], T[:, 1], T[:, 2]], np.array([sims[i][2] for i in idx], f64)


def _one(Sa, k):
    return [float(v[k]) for v in Sa[0]], [float(v[k]) for v in Sa[1]], float(Sa[2][k])


def record(S):
    return soc.sim3_record(S)


def tcw_of(S):
    """[R | t * (1. / s)] as float (:992-1009)"""
    T = np.eye(4, dtype=f32)
    T[:3, :3] = np.array(soc.quat_to_R(S[0]), f64).reshape(3, 3).astype(f32)
    inv = 1. / S[2]
    T[:3, 3] = np.array([S[1][0] * inv, S[1][1] * inv, S[1][2] * inv], f64).astype(f32)
    return T


class _Graph:
    def __init__(self, p):
        self.n = len(np.asarray(p["fixed"]).reshape(-1))
        self.fixed = np.asarray(p["fixed"], np.uint8).reshape(-1) != 0
        self.has_nc = np.asarray(p["has_nc"], np.uint8).reshape(-1) != 0
        self.edges = np.asarray(p["edges"], np.int64).reshape(-1, 3)
        self.fix = bool(p["fix_scale"])
        self.Scw, self.Snc = sims_from_floats(p["Scw"]), sims_from_floats(np.where(self.has_nc[:, None], np.asarray(p["Snc"], f32).reshape(-1, 13), np.asarray(p["Scw"], f32).reshape(-1, 13)))
        self.free = np.nonzero(~self.fixed)[0]
        self.fidx = np.full(self.n, -1)
        self.fidx[self.free] = np.arange(len(self.free))
        i, j, kind = self.edges[:, 0], self.edges[:, 1], self.edges[:, 2]
        # the measurements (:857-867, :889-972): Sji = Sjw * Swi
        src = lambda k, v: self.Snc[v] if (k == 1 and self.has_nc[v]) else self.Scw[v]
        Cs = [soc.sim3_mul(src(kind[e], j[e]), soc.sim3_inv(src(kind[e], i[e]))) for e in range(len(i))]
        self.C = _cols(Cs, range(len(Cs)))

    def errors(self, Si, Sj):
        """EdgeSim3::computeError of every edge: (C * v0 * v1.inverse()).log(), [E, 7]"""
        if len(self.edges) == 0:
            return np.zeros((0, 7))
        return sim3_log(soc.sim3_mul(soc.sim3_mul(self.C, Si), soc.sim3_inv(Sj)))

    def errors_at(self, est):
        return self.errors(_cols(est, self.edges[:, 0]), _cols(est, self.edges[:, 1]))

    def chi2(self, est, order):
        e = self.errors_at(est)
        c = np.zeros(len(e))
        for k in range(7):
            c = c + e[:, k] * e[:, k]
        if order == "reversed":
            c = c[::-1]
        return float(np.add.accumulate(c)[-1]) if len(c) else 0.0

    def build(self, est, order):
        """computeActiveErrors, linearizeOplus (numeric, both vertices), buildSystem: F, H [7 n_free, 7 n_free], b"""
        E = len(self.edges)
        i, j = self.edges[:, 0], self.edges[:, 1]
        Si, Sj = _cols(est, i), _cols(est, j)
        e = self.errors(Si, Sj)
        scalar = 1.0 / (2 * DELTA)
        J = np.zeros((2, E, 7, 7))
        for d in range(7):
            pert = []
            for sgn in (DELTA, -DELTA):
                u = [0.0] * 7
                u[d] = sgn
                pert.append([soc.sim3_oplus(S, u, self.fix) for S in est])
            J[0, :, :, d] = scalar * (self.errors(_cols(pert[0], i), Sj) - self.errors(_cols(pert[1], i), Sj))
            J[1, :, :, d] = scalar * (self.errors(Si, _cols(pert[0], j)) - self.errors(Si, _cols(pert[1], j)))
        nf = len(self.free)
        H, b, F = np.zeros((7 * nf, 7 * nf)), np.zeros(7 * nf), 0.0
        for k in (range(E) if order == "forward" else range(E - 1, -1, -1)):
            F += float(sum(e[k, m] * e[k, m] for m in range(7)))
            fa, fb = self.fidx[i[k]], self.fidx[j[k]]
            A, B = J[0, k], J[1, k]
            if fa >= 0:
                H[7 * fa:7 * fa + 7, 7 * fa:7 * fa + 7] += A.T @ A
                b[7 * fa:7 * fa + 7] += A.T @ (-e[k])
            if fb >= 0:
                H[7 * fb:7 * fb + 7, 7 * fb:7 * fb + 7] += B.T @ B
                b[7 * fb:7 * fb + 7] += B.T @ (-e[k])
            if fa >= 0 and fb >= 0:
                H[7 * fa:7 * fa + 7, 7 * fb:7 * fb + 7] += A.T @ B
                H[7 * fb:7 * fb + 7, 7 * fa:7 * fa + 7] += B.T @ A
        return F, H, b


def chol_solve(H, b, lam):
    """(H + lam I) x = b by numpy.linalg.cholesky; (x, ok)"""
    try:
        L = np.linalg.cholesky(H + lam * np.eye(len(b)))
    except np.linalg.LinAlgError:
        return np.zeros(len(b)), False
    if not np.isfinite(L).all():
        return np.zeros(len(b)), False
    import scipy.linalg as sl
    y = sl.solve_triangular(L, b, lower=True)
    return sl.solve_triangular(L.T, y, lower=False), True


def valid(p):
    Scw, Snc = np.asarray(p["Scw"], f32).reshape(-1, 13), np.asarray(p["Snc"], f32).reshape(-1, 13)
    has_nc, fixed = np.asarray(p["has_nc"], np.uint8).reshape(-1) != 0, np.asarray(p["fixed"], np.uint8).reshape(-1) != 0
    edges = np.asarray(p["edges"], np.int64).reshape(-1, 3)
    n = len(fixed)
    if not (np.isfinite(Scw).all() and (Scw[:, 0] > 0).all() and np.isfinite(Snc[has_nc]).all() and (Snc[has_nc, 0] > 0).all()):
        return False
    if len(edges) and not (((edges[:, :2] >= 0) & (edges[:, :2] < n)).all() and (edges[:, 0] != edges[:, 1]).all() and np.isin(edges[:, 2], (0, 1)).all()):
        return False
    return n == 0 or bool(fixed.any())


def optimize_essential_graph(p, order="forward"):
    """OptimizeEssentialGraph of one problem p = dict(Scw [n, 13], Snc [n, 13], has_nc [n], fixed [n], edges [E, 3], fix_scale).  Returns dict(status [4],
    Scw [n, 13] float64, Tcw [n, 4, 4] float32, est (the Sim3s), trace [trials][6], F0).  order: the order in which the edges are added up."""
    n, E = len(np.asarray(p["fixed"]).reshape(-1)), len(np.asarray(p["edges"]).reshape(-1, 3))
    if not valid(p):
        return dict(status=np.array([-1, 0, E, 0], np.int32), Scw=None, Tcw=None, est=None, trace=[], F0=None)
    g = _Graph(p)
    est = list(g.Scw)
    trace = []
    its, F0 = 0, None
    if len(g.free) and E:
        lam, ni = 1e-16, 2.0   # setUserLambdaInit(1e-16)
        for it in range(20):
            current, H, b = g.build(est, order)
            if it == 0:
                F0 = current
            rho, qmax = 0.0, 0
            while True:
                x, ok2 = chol_solve(H, b, lam)
                trial = list(est)
                for f, k in enumerate(g.free):
                    trial[k] = soc.sim3_oplus(est[k], x[7 * f:7 * f + 7], g.fix)
                temp = g.chi2(trial, order)
                if not ok2:
                    temp = DBL_MAX
                rho = current - temp
                scale = float(np.add.accumulate(x * (lam * x + b))[-1]) + 1e-3
                with np.errstate(all="ignore"):
                    rho = float(f64(rho) / f64(scale))
                accepted = rho > 0 and math.isfinite(temp)
                trace.append([current, temp, rho, lam, 1.0 if accepted else 0.0, 1.0 if (it == 0 and qmax == 0) else 0.0])
                if accepted:
                    alpha = 1. - (2 * rho - 1) * (2 * rho - 1) * (2 * rho - 1)
                    alpha = min(alpha, 2. / 3.)
                    lam *= max(1. / 3., alpha)
                    ni = 2.0
                    current = temp
                    est = trial
                else:
                    lam *= ni
                    ni *= 2
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            its += 1
            if qmax == 10 or rho == 0:
                break
    return dict(status=np.array([0, len(g.free), E, 256 * its + len(trace)], np.int32), Scw=np.array([record(S) for S in est], f64).reshape(n, 13),
                Tcw=np.array([tcw_of(S) for S in est], f32).reshape(n, 4, 4), est=est, trace=trace, F0=F0, graph=g)


def correct_points(Scw_in, Scw_out, ref, P, P_out=None):
    """:1013-1043 for one problem: P' = correctedSwr.map(Srw.map(P)); Scw_in [n, 13] float32, Scw_out [n, 13] float64 (R, t, s), ref [M], P [M, 3] float32"""
    P = np.asarray(P, f32).reshape(-1, 3)
    out = np.zeros_like(P) if P_out is None else np.array(P_out, f32)
    sims = sims_from_floats(Scw_in)
    for m in range(len(P)):
        r = int(ref[m])
        if r < 0:
            continue
        o = np.asarray(Scw_out[r], f64)
        Swr = soc.sim3_inv((soc.quat_from_R(o[:9]), [float(v) for v in o[9:12]], float(o[12])))
        smap = lambda S, x: [S[2] * v + S[1][k] for k, v in enumerate(soc.quat_rot(S[0], x))]
        out[m] = np.array(smap(Swr, smap(sims[r], [float(v) for v in P[m].astype(f64)])), f64).astype(f32)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the edge rules of :847-983 over flat views, written as the reference's loops
def essential_graph_edges(parent, children, loop_edges, covisibles, loop_connections, cur, loop, weight=None):
    out, inserted = [], set()
    for i in sorted(loop_connections):
        for j in sorted(set(loop_connections[i])):
            w = 0 if weight is None else weight(i, j)
            if (i != cur or j != loop) and w < MIN_FEAT:
                continue
            out.append((i, j, 0))
            inserted.add((min(i, j), max(i, j)))
    for i in range(len(parent)):
        if parent[i] >= 0:
            out.append((i, parent[i], 1))
        for l in sorted(set(loop_edges[i])):
            if l < i:
                out.append((i, l, 1))
        for n in covisibles[i]:
            if n != parent[i] and n not in children[i] and n not in loop_edges[i]:
                if n < i:
                    if (min(i, n), max(i, n)) in inserted:
                        continue
                    out.append((i, n, 1))
    return np.array(out, np.int32).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# generated graphs
def rodrigues(w):
    th = float(np.linalg.norm(w))
    if th < 1e-12:
        return np.eye(3)
    k = np.asarray(w, f64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def rec13(s, R, t):
    return np.concatenate([[s], np.asarray(R, f64).reshape(9), np.asarray(t, f64).reshape(3)]).astype(f32)


def make_ring(n, seed, fix_scale, sigma=0.01, scale_drift=False, fixed=(0,), extra=3, dup=False, arrow=False, name=None):
    """n keyframes on a circle, looking inwards, walked once.  Keyframe 0 is the loop keyframe and n - 1 the current one: the estimates of 1 .. n - 1 have
    drifted (a random 7-vector of sigma per step composed on the left; its scale component only with scale_drift), the current keyframe has a corrected
    Sim3 (the truth; with scale_drift its scale undoes the drift) beside its non-corrected one.  Edges as the reference forms them: the loop connection
    (n - 1, 0) of kind 0 first, then per keyframe the spanning-tree edge (k, k - 1) and the covisibility edge (k, k - extra), of kind 1.  dup repeats one
    covisibility edge; arrow gives each of the last three keyframes an edge to keyframes 1, 2 and 3."""
    rng = np.random.default_rng(seed)
    true, drift = [], []
    for k in range(n):
        a = 2 * math.pi * k / max(n, 8)
        Rwc = rodrigues([0, a, 0]) @ rodrigues([0.05 * math.sin(3 * a), 0, 0])
        Ow = np.array([4 * math.sin(a), 0.1 * math.cos(2 * a), 4 - 4 * math.cos(a)])
        R = Rwc.T
        true.append((1.0, R, -R @ Ow))
    M = lambda s, R, t: np.block([[s * R, np.asarray(t, f64).reshape(3, 1)], [np.zeros((1, 3)), np.ones((1, 1))]])
    drift.append(true[0])
    for k in range(1, n):
        rel = M(*true[k]) @ np.linalg.inv(M(*true[k - 1]))
        u = sigma * rng.normal(size=7)
        if not scale_drift:
            u[6] = 0.0
        else:
            u[6] = abs(u[6]) + sigma   # the scale drifts one way, as monocular scale does
        q, t, s = soc.sim3_exp(u)
        D = M(s, np.array(soc.quat_to_R(q)).reshape(3, 3), t) @ rel @ M(*drift[k - 1])
        sc = float(np.cbrt(np.linalg.det(D[:3, :3])))
        drift.append((sc, D[:3, :3] / sc, D[:3, 3]))
    Scw = np.stack([rec13(*d) for d in drift])
    Snc = Scw.copy()
    has_nc = np.zeros(n, np.uint8)
    if n > 1:
        has_nc[n - 1] = 1
        Scw[n - 1] = rec13(*true[n - 1])   # CorrectedSim3[pCurKF]: where the loop says the keyframe is (scale 1: the drifted scale is what gets corrected)
    fx = np.zeros(n, np.uint8)
    fx[list(fixed)] = 1
    edges = [(n - 1, 0, 0)] if n > 1 else []
    for k in range(1, n):
        edges.append((k, k - 1, 1))
        if k - extra >= 0 and not (k == n - 1 and k - extra == 0):
            edges.append((k, k - extra, 1))
            if dup and k == extra + 1:
                edges.append((k, k - extra, 1))
    if arrow:
        for k in range(n - 3, n):
            edges += [(k, m, 1) for m in (1, 2, 3)]
    return dict(name=name or "ring_%d_%d%s" % (n, seed, "_fix" if fix_scale else ""), Scw=Scw, Snc=Snc, has_nc=has_nc, fixed=fx, edges=np.array(edges, np.int32).reshape(-1, 3),
                fix_scale=int(fix_scale))


def make_consistent(n=6):
    """Identity rotations, dyadic translations, unit scales: every product and logarithm is exact, so F = 0 and b = 0 exactly."""
    Scw = np.stack([rec13(1.0, np.eye(3), [0.25 * k, -0.5 * k, 0.125 * (k % 3)]) for k in range(n)])
    edges = [(k, k - 1, 1) for k in range(1, n)] + [(n - 1, 0, 0), (n - 1, 1, 1)]
    fx = np.zeros(n, np.uint8)
    fx[0] = 1
    return dict(name="consistent_%d" % n, Scw=Scw, Snc=Scw.copy(), has_nc=np.zeros(n, np.uint8), fixed=fx, edges=np.array(edges, np.int32), fix_scale=1)


def empty_problem(n=0):
    """n keyframes (keyframe 0 fixed), no edges"""
    Scw = np.stack([rec13(1.0, rodrigues([0.1 * k, 0.2, 0]), [k, 0, 1]) for k in range(n)]) if n else np.zeros((0, 13), f32)
    fx = np.zeros(n, np.uint8)
    fx[:1] = 1
    return dict(name="empty_%d" % n, Scw=Scw, Snc=Scw.copy(), has_nc=np.zeros(n, np.uint8), fixed=fx, edges=np.zeros((0, 3), np.int32), fix_scale=1)


_cache = {}


def parity_problems():
    """The parity batch of the GPU test: rings at the sizes where 7 n_free crosses 64, 128 and 256, one of about 130 keyframes, an arrow, the fixed vertex
    first, in the middle and last, two fixed vertices, a duplicated edge, the consistent graph, both fix_scale values, the free-scale case whose damping
    grows, and empty problems."""
    if "p" not in _cache:
        ps = [make_ring(2, 1, True), make_ring(3, 2, True), make_ring(9, 3, True), make_ring(10, 4, True), make_ring(19, 5, True), make_ring(20, 6, False),
              make_ring(37, 7, True), make_ring(38, 8, True), make_ring(130, 9, True, name="ring_130"), make_ring(17, 10, True, arrow=True, name="arrow_17"),
              make_ring(12, 11, True, fixed=(6,), name="fixed_middle"), make_ring(12, 12, True, fixed=(11,), name="fixed_last"),
              make_ring(12, 13, True, fixed=(0, 7), name="two_fixed"), make_ring(12, 14, True, dup=True, name="dup_edge"), make_consistent(),
              make_ring(9, 15, False, name="free_9"), make_ring(17, 16, False, scale_drift=True, name="free_scale_drift_17"), empty_problem(0), empty_problem(4)]
        _cache["p"] = ps
    return _cache["p"]


def reference_of(problems, key, order="forward"):
    k = (key, order)
    if k not in _cache:
        _cache[k] = [optimize_essential_graph(p, order) for p in problems]
    return _cache[k]


def concat_batch(problems):
    """the packed arrays of a batch: dict(Scw, Snc, has_nc, fixed, edges), n_kf [n], n_edges [n]"""
    cat = lambda k, shape, dt: np.concatenate([np.asarray(p[k], dt).reshape(shape) for p in problems]) if problems else np.zeros(tuple(max(s, 0) for s in shape), dt)
    n_kf = np.array([len(np.asarray(p["fixed"]).reshape(-1)) for p in problems], np.int32)
    n_ed = np.array([len(np.asarray(p["edges"]).reshape(-1, 3)) for p in problems], np.int32)
    return dict(Scw=cat("Scw", (-1, 13), f32), Snc=cat("Snc", (-1, 13), f32), has_nc=cat("has_nc", (-1,), np.uint8), fixed=cat("fixed", (-1,), np.uint8),
                edges=cat("edges", (-1, 3), np.int32)), n_kf, n_ed


def decisive_trials(fwd, rev):
    """Per trial of the forward run: decisive = |F - F'| > 1e-9 max(F, F') and the reversed run made the same decision at the same position (and has run
    the same trials up to there)."""
    out = []
    same = True
    for k, t in enumerate(fwd["trace"]):
        if k >= len(rev["trace"]):
            same = False
        F, Ft = t[0], t[1]
        dec = same and abs(F - Ft) > 1e-9 * max(F, Ft) and rev["trace"][k][4] == t[4]
        if same and rev["trace"][k][4] != t[4]:
            same = False
        out.append(bool(dec))
    return out
