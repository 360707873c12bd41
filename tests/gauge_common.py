"""World poses far from the identity for the pose-consuming operators: a rigid motion G of the world (Xw' = G Xw, Tcw' = Tcw G^-1, observations unchanged)
leaves every residual of a problem as it is and turns the rotation of every pose by G's, so the matrix -> quaternion conversion at the head of each
optimiser (csrc/se3_math.h quat_from_R) takes another of its four bodies and the float kernels that read rows of Tcw / Twc see negative diagonal
entries, a far camera centre and a view direction along -z.  G is applied in float64 and the result rounded once to float32; the generators themselves
(object_slam_amd/synth.py, tests/*_common.py) are not changed.  Shared by test_far_pose_cpu.py (census of the bodies reached, decidability of the
reference on the moved inputs) and test_far_pose_gpu.py (kernel against the reference on the same moved inputs).  Never imports the product's kernels."""
import math

import numpy as np

f32, f64 = np.float32, np.float64


def quat_branch(R):
    """Which body Eigen's matrix -> quaternion rule (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>) takes for R: 0 if the
    trace is positive; otherwise 1 + i with i the row of the largest diagonal entry as Eigen finds it (i = 0; if m11 > m00: i = 1; if m22 > m_ii: i = 2),
    so ties go to the lower index."""
    R = np.asarray(R, f64)
    m = R.reshape(4, 4)[:3, :3] if R.size == 16 else R.reshape(3, 3)
    if m[0, 0] + m[1, 1] + m[2, 2] > 0:
        return 0
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    return 1 + i


def rot(axis, degrees):
    k = np.asarray(axis, f64) / np.linalg.norm(axis)
    th = math.radians(degrees)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


PI_X, PI_Y, PI_Z = np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0])   # exactly pi about an axis: w = 0
CYCLIC = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])                                 # trace exactly 0, all diagonal entries equal
HAND_ROTATIONS = dict(pi_x=PI_X, pi_y=PI_Y, pi_z=PI_Z, cyclic=CYCLIC)

# name -> (rotation, translation [m], at most 10 m long: the relative bar |d| / max(1, |ref|max) of the parity tests must not loosen)
GAUGES = dict(
    rx170=(rot([1, 0, 0], 170.0), [3.0, -2.0, 5.0]),
    ry175=(rot([0, 1, 0], 175.0), [-6.0, 1.0, 4.0]),
    rz150=(rot([0, 0, 1], 150.0), [2.0, 7.0, -3.0]),
    rx150=(rot([1, 0, 0], 150.0), [-1.0, 4.0, 2.0]),
    ry160=(rot([0, 1, 0], 160.0), [5.0, 0.5, -6.0]),
    r111_130=(rot([1, 1, 1], 130.0), [-4.0, -5.0, 3.0]),
    ry119_5=(rot([0, 1, 0], 119.5), [1.0, -3.0, 8.0]),      # trace = 1 + 2 cos = 0.015: the poses of one window fall on both sides of trace = 0
    pi_x=(PI_X, [0.5, -2.0, 4.0]),
    pi_y=(PI_Y, [-3.0, 0.25, 1.0]),
    pi_z=(PI_Z, [2.0, 1.5, -0.5]),
    cyclic=(CYCLIC, [-1.0, 2.0, 6.0]),
)


def gauge(name):
    """the 4 x 4 float64 matrix of GAUGES[name]"""
    R, t = GAUGES[name]
    G = np.eye(4)
    G[:3, :3] = R
    G[:3, 3] = t
    assert np.linalg.norm(t) <= 10.0
    return G


def inv_rigid(G):
    Gi = np.eye(4)
    Gi[:3, :3] = G[:3, :3].T
    Gi[:3, 3] = -G[:3, :3].T @ G[:3, 3]
    return Gi


def move_poses(T, G):
    """Tcw G^-1 of one pose or a stack of poses, float64 in, float32 out (one rounding)"""
    return (np.asarray(T).astype(f64) @ inv_rigid(G)).astype(f32)


def move_points(X, G):
    """G X of points [..., 3], float32 out (one rounding)"""
    X = np.asarray(X).astype(f64)
    return (X @ G[:3, :3].T + G[:3, 3]).astype(f32)


def poses_back(Tg, G):
    """a pose of the moved world as a pose of the unmoved one (float64)"""
    return np.asarray(Tg).astype(f64) @ G


def points_back(Xg, G):
    return (np.asarray(Xg).astype(f64) - G[:3, 3]) @ G[:3, :3]


def branches(T):
    """quat_branch of every pose of a stack [.., 4, 4] (or [.., 16])"""
    return [quat_branch(t[:3, :3]) for t in np.asarray(T).reshape(-1, 4, 4)]


def hand_gauge(T0, name, t=(0.25, -0.5, 1.0)):
    """The motion G that gives the pose T0 the rotation block HAND_ROTATIONS[name] exactly (and the dyadic translation t): G = H^-1 T0.  Returns (G, H as
    float32, every entry exact)."""
    H = np.eye(4)
    H[:3, :3] = HAND_ROTATIONS[name]
    H[:3, 3] = t
    G = inv_rigid(H) @ np.asarray(T0).astype(f64)
    return G, H.astype(f32)


# ---- the problems of object_slam_amd/synth.py ----
def regauge_pose_problem(p, G, Tcw=None):
    """make_pose_problem / make_semantic_problem output in the world moved by G.  Tcw: the start pose to use instead of the rounded product (hand poses)."""
    q = dict(p, Tcw=move_poses(p["Tcw"], G) if Tcw is None else np.asarray(Tcw, f32), Xw=move_points(p["Xw"], G), T_gt=np.asarray(p["T_gt"], f64) @ inv_rigid(G))
    if "objmp_Xw" in p:
        q["objmp_Xw"] = move_points(p["objmp_Xw"], G)
    return q


regauge_semantic_problem = regauge_pose_problem


def hand_pose_problem(p, name):
    """the pose problem whose start pose has exactly the rotation HAND_ROTATIONS[name]; returns (problem, G)"""
    G, H = hand_gauge(p["Tcw"], name)
    return regauge_pose_problem(p, G, Tcw=H), G


def regauge_lba_problem(q, G):
    """make_lba_problem output in the world moved by G"""
    return dict(q, poses=move_poses(q["poses"], G), points=move_points(q["points"], G))


def lba_args(q):
    return (q["poses"], q["fixed"], q["points"], q["edge_kf"], q["edge_pt"], q["edge_obs"], q["edge_invSigma2"], q["K"])


def pose_args(p):
    return (p["Tcw"], p["Xw"], p["obs"], p["invSigma2"], p["has_mp"], p["K"])


# ---- triangulation (batch_common.tri_pose / tri_make_kf) ----
def regauge_tri(Tcw, G):
    """(Tcw', Twc') of a keyframe in the moved world; Twc' is the float inverse built as batch_common.tri_pose builds it"""
    T = move_poses(Tcw, G)
    W = np.eye(4, dtype=f32)
    W[:3, :3] = T[:3, :3].T
    W[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return T, W


# ---- essential graph (essential_graph_common.make_ring) ----
def regauge_ring(p, G, name=None):
    """A make_ring problem in the world moved by G: every Sim3 record (s, R, t) becomes (s, R Rg^T, t - s R Rg^T tg)."""
    def move(rec):
        rec = np.asarray(rec, f32).astype(f64).reshape(-1, 13)
        out = rec.copy()
        for k, r in enumerate(rec):
            R = r[1:10].reshape(3, 3) @ G[:3, :3].T
            out[k, 1:10] = R.reshape(9)
            out[k, 10:13] = r[10:13] - r[0] * (R @ G[:3, 3])
        return out.astype(f32)
    return dict(p, Scw=move(p["Scw"]), Snc=move(p["Snc"]), name=name or p["name"] + "_moved")


def ring_branches(p):
    return [quat_branch(r[1:10].reshape(3, 3)) for r in np.asarray(p["Scw"], f32).astype(f64).reshape(-1, 13)]


# ---- OptimizeSim3 with a half turn between the two cameras ----
def make_sim3_far_problem(seed, count, fix_scale, axis, degrees=150.0, outliers=0.1, noise=0.5):
    """sim3_opt_common.make_problem with the second camera turned: p_c1 = s R p_c2 + t with R = `degrees` about `axis` (x, y: the cameras face each other
    over the scene; z: the second camera is rolled).  Everything else — noise, information, gross outliers, the start 2 degrees, 2 % of the depth and 5 % of
    the scale off the truth — as make_problem does it."""
    import sim3_match_common as smc
    import sim3_opt_common as soc
    rng = np.random.default_rng(seed)
    s = 1.0 if fix_scale else float(rng.uniform(0.8, 1.25))
    # the second camera's centre in the first camera's frame: on the far side of the scene (depth 4 .. 10) for the facing pairs, looking back at its middle
    t = {"x": np.array([0.0, 3.6, 13.5]), "y": np.array([-3.6, 0.0, 13.5]), "z": np.array([0.1, -0.1, 0.1])}[axis] + rng.uniform(-0.15, 0.15, 3)
    axis_v = {"x": [1, 0, 0], "y": [0, 1, 0], "z": [0, 0, 1]}[axis]
    R = rot(axis_v, degrees) @ smc.rodrigues(0.02 * rng.normal(size=3))
    P1 = np.zeros((0, 3))
    for _ in range(200):
        if len(P1) >= count:
            break
        c = smc._frustum(rng, 8 * count + 64)
        c2 = (c - t) @ R / s
        P1 = np.concatenate([P1, c[smc._inside(smc._project(c2), c2, 4.0) & smc._inside(smc._project(c), c, 4.0) & (c2[:, 2] > 2.0)]])
    assert len(P1) >= count, (axis, len(P1))
    P1 = P1[:count]
    P2 = (P1 - t) @ R / s
    oct1, oct2 = rng.integers(0, smc.NLEVELS, count), rng.integers(0, smc.NLEVELS, count)
    sf1, sf2 = smc.SF[oct1].astype(f64), smc.SF[oct2].astype(f64)
    obs1 = smc._project(P1) + rng.uniform(-noise, noise, (count, 2)) * sf1[:, None]
    obs2 = smc._project(P2) + rng.uniform(-noise, noise, (count, 2)) * sf2[:, None]
    gross = np.zeros(count, bool)
    gross[rng.permutation(count)[:int(round(outliers * count))]] = True
    for i in np.nonzero(gross)[0]:
        ang, mag = rng.uniform(0, 2 * np.pi), rng.uniform(25.0, 60.0)
        if rng.integers(0, 2):
            obs1[i] += mag * sf1[i] * np.array([np.cos(ang), np.sin(ang)])
        else:
            obs2[i] += mag * sf2[i] * np.array([np.cos(ang), np.sin(ang)])
    pa, pt = rng.normal(size=3), rng.normal(size=3)
    R0 = smc.rodrigues(np.deg2rad(2.0) * pa / np.linalg.norm(pa)) @ R
    t0 = t + 0.02 * 7.0 * pt / np.linalg.norm(pt)
    s0 = s if fix_scale else s * (1.0 + 0.05 * (1 if rng.integers(0, 2) else -1))
    return dict(name="far_%s_%d_%d%s" % (axis, seed, count, "_fix" if fix_scale else ""), X3Dc1=P1.astype(f32), X3Dc2=P2.astype(f32), obs1=obs1.astype(f32), obs2=obs2.astype(f32),
                invSigma2_1=soc.inv_level_sigma2(oct1), invSigma2_2=soc.inv_level_sigma2(oct2), K1=soc.K, K2=soc.K, s12=f32(s0), R12=R0.astype(f32), t12=t0.astype(f32),
                th2=soc.TH2, fix_scale=int(fix_scale), gross=gross, truth=(R, t, s))


_sim3 = {}


def sim3_references(case):
    if case not in _sim3:
        import sim3_opt_common as soc
        p = make_sim3_far_problem(*case)
        _sim3[case] = (p, [soc.optimize_sim3(p, o) for o in ("forward", "reversed", "wavefront")])
    return _sim3[case]


def decided_prefix(refs):
    """the number of leading trials whose decision is the same in every summation order with |rho| > 1e-6 in each"""
    n = 0
    for ts in zip(*(r["trace"] for r in refs)):
        if len({t[4] for t in ts}) != 1 or min(abs(t[2]) for t in ts) <= 1e-6:
            break
        n += 1
    return n


def conjugate_ring(p, P, name=None):
    """A make_ring problem with the axes of the world AND of every camera relabelled by the permutation matrix P: (s, R, t) -> (s, P R P^T, P t).  The
    graph's measurements Sj Si^-1 are conjugated by P alike, so it is the same problem; the ring's axis (y as generated) becomes P e_y, and the entries
    are permuted without any rounding."""
    def move(rec):
        rec = np.asarray(rec, f32).reshape(-1, 13)
        out = rec.copy()
        Pf = np.asarray(P, f32)
        for k, r in enumerate(rec):
            out[k, 1:10] = (Pf @ r[1:10].reshape(3, 3) @ Pf.T).reshape(9)
            out[k, 10:13] = Pf @ r[10:13]
        return out
    return dict(p, Scw=move(p["Scw"]), Snc=move(p["Snc"]), name=name or p["name"] + "_conjugated")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The cases of test_far_pose_gpu.py.  test_far_pose_cpu.py asserts for each table that the input poses reach all four bodies and that the reference
# decides every case (same flags as on the unmoved problem); a case that fails there is replaced there, never skipped on the GPU.
# PoseOptimization: (seed, N, gauge); "hand:<name>" = the start pose with exactly that rotation block.  N = 60 with `few`: 8 map points (< 10 edges, one round)
POSE_KW = dict(outlier_frac=0.1, stereo_frac=0.7)
POSE_CASES = [(0, 400, "rx170"), (0, 400, "rz150"), (0, 400, "cyclic"), (0, 400, "hand:pi_y"), (1, 400, "ry175"), (1, 400, "ry119_5"), (1, 400, "r111_130"), (1, 400, "hand:pi_x"),
              (1, 400, "hand:cyclic"), (3, 400, "pi_z"), (3, 400, "cyclic"), (3, 400, "rx150"), (3, 400, "hand:pi_z"), (4, 60, "pi_x"), (4, 60, "ry160"), (4, 60, "rz150"),
              (4, 60, "cyclic"), (4, 60, "hand:pi_y")]
POSE_FEW = [(4, 60, "pi_y"), (4, 60, "rz150"), (4, 60, "rx170"), (4, 60, "cyclic")]       # has_mp cleared but for 8 map points: a single round
POSE_BATCH = [(100, "rx170"), (101, "ry175"), (102, "rz150"), (103, "cyclic"), (104, "ry119_5"), (105, "r111_130"), (106, "hand:pi_x"), (107, "pi_z")]   # N = 400 each
POSE_TRACE = [(0, 400, "rz150"), (1, 400, "rx170"), (1, 400, "ry175")]     # one per non-trace body: the first trial's cost pins the start pose to 1e-7
SEMANTIC_CASES = [(0, "cyclic"), (1, "rx170"), (2, "ry175"), (3, "pi_z"), (1, "ry119_5"), (2, "r111_130")]   # make_semantic_problem(seed, N = 400, n_obj = 3, outlier_frac = 0.1)
# LocalBundleAdjustment: (seed, KL, KF, P) and the gauges of each shape; cyclic, r111_130 and ry119_5 put the keyframes of one window into different bodies
LBA_SHAPES = {"A": (3, 4, 2, 150), "B": (4, 6, 3, 300)}
LBA_CASES = [("A", "rx170"), ("A", "cyclic"), ("A", "ry119_5"), ("B", "rz150"), ("B", "r111_130"), ("B", "ry119_5"), ("B", "pi_y")]
LBA_BATCH = [("A", "rx170"), ("B", "ry119_5"), ("A", "cyclic"), ("B", "rz150"), ("A", "pi_y"), ("B", "r111_130")]
LBA_TRACE = [("A", "cyclic")]
# BundleAdjustment: (layout, robust, iterations, gauge) on make_lba_problem(24, 8, 0, 400) as tests/test_lba_gpu.py runs it.  Without the robust kernel the runs
# take 10 iterations: at 20 the reference's own points move by up to 3.6e-4 of the scene under the float rounding of a moved input (one point of the seed
# sits in a shallow valley by then), beyond the 1e-4 bar, so pose parity is not decidable there; at 10 they move by 1e-6.
BA_CASES = [(0, True, 5, "rx170"), (0, False, 10, "cyclic"), (1, True, 5, "ry119_5"), (1, False, 10, "rz150"), (2, True, 5, "r111_130"), (2, False, 10, "pi_y")]
# OptimizeSim3: (seed, count, fix_scale, axis of the 150 degrees between the cameras)
SIM3_CASES = [(1, 129, 0, "x"), (2, 129, 1, "x"), (1, 129, 0, "y"), (2, 129, 1, "y"), (1, 129, 0, "z"), (2, 129, 1, "z"), (3, 300, 0, "y")]
# OptimizeEssentialGraph: make_ring(12, seed, fix_scale) with the ring's axis along x (P = CYCLIC^T: e_y -> e_x) and z (P = CYCLIC), and one ring in a moved world
RING_CASES = [(21, True, "x"), (22, False, "x"), (21, True, "z"), (22, False, "z"), (23, True, "cyclic")]
# Triangulation: the seeds of tests/test_triangulate_gpu.py (seed, stereo_frac, baseline) at N = 300, 3 pairs
TRI_CASES = [(1, 0.6, 0.5, "rx170"), (2, 0.6, 0.02, "r111_130"), (1, 0.6, 0.5, "rz150"), (2, 0.6, 0.02, "ry175")]


def pose_case(seed, N, g, few=False):
    """(moved problem, unmoved problem, G)"""
    from object_slam_amd import synth
    p = synth.make_pose_problem(seed, N=N, **POSE_KW)
    if few:
        p["has_mp"] = np.zeros(N, np.uint8)
        p["has_mp"][:8] = 1
    if g.startswith("hand:"):
        q, G = hand_pose_problem(p, g[5:])
    else:
        G = gauge(g)
        q = regauge_pose_problem(p, G)
    return q, p, G


def semantic_case(seed, g):
    from object_slam_amd import synth
    p = synth.make_semantic_problem(seed, N=400, n_obj=3, outlier_frac=0.1)
    G = gauge(g)
    return regauge_semantic_problem(p, G), p, G


_lba_cache = {}


def lba_case(shape, g):
    from object_slam_amd import synth
    if shape not in _lba_cache:
        seed, KL, KF, P = LBA_SHAPES[shape]
        _lba_cache[shape] = synth.make_lba_problem(seed, K_local=KL, K_fixed=KF, P=P, stereo_frac=[0.85, 1.0, 0.0][seed % 3])
    G = gauge(g)
    return regauge_lba_problem(_lba_cache[shape], G), _lba_cache[shape], G


def ba_case(robust, g):
    from object_slam_amd import synth
    q0 = synth.make_lba_problem(24, K_local=8, K_fixed=0, P=400, outlier_frac=0.02 if robust else 0.0)
    fixed = np.zeros(8, np.uint8)
    fixed[0] = 1
    q0 = dict(q0, fixed=fixed)
    G = gauge(g)
    return regauge_lba_problem(q0, G), q0, G


def ring_case(seed, fix_scale, how):
    import essential_graph_common as egc
    p0 = egc.make_ring(12, seed, fix_scale)
    if how == "x":
        return conjugate_ring(p0, CYCLIC.T, name="ring_axis_x_%d" % seed), p0
    if how == "z":
        return conjugate_ring(p0, CYCLIC, name="ring_axis_z_%d" % seed), p0
    return regauge_ring(p0, gauge(how), name="ring_%s_%d" % (how, seed)), p0


def tri_case(seed, stereo_frac, baseline, g, N=300, n_pairs=3, n_match=150):
    """tests/test_triangulate_gpu.py's problem at N = 300 with 3 pairs (the first with an empty match list), every pose moved by the gauge.  Returns
    dict(cam8, kf1 = (T1, W1, arrays), pairs = [(T2, W2, arrays, i1, i2)], unmoved = the same with the poses as generated, G)."""
    from batch_common import tri_make_kf, tri_pose
    from object_slam_amd.synth import KITTI_K
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = KITTI_K
    cam8 = np.array([fx, fy, cx, cy, f32(1) / f32(fx), f32(1) / f32(fy), bf, bf / fx], f32)
    X = np.stack([rng.uniform(-15, 15, N), rng.uniform(-4, 4, N), rng.uniform(2, 60, N)], 1)
    X[:20, 2] = rng.uniform(-5, 0.5, 20)          # behind / very close: cheirality and parallax rejections
    G = gauge(g)
    T1, W1 = tri_pose(rng, 0.05)
    a1 = tri_make_kf(rng, X, T1, KITTI_K, stereo_frac, 0.7)
    pairs, plain = [], []
    for p in range(n_pairs):
        T2, W2 = tri_pose(rng, baseline * (p + 1) / 2)
        a = tri_make_kf(rng, X, T2, KITTI_K, stereo_frac, 0.7)
        perm = rng.permutation(N).astype(np.int32)
        a = tuple(v[perm] for v in a)
        inv = np.argsort(perm).astype(np.int32)
        m = rng.choice(N, n_match if p else 0, replace=False).astype(np.int32)
        i2 = inv[m].copy()
        bad = rng.random(len(m)) < 0.15
        i2[bad] = rng.integers(0, N, int(bad.sum()))
        i1, i2 = np.sort(m), i2[np.argsort(m)]
        plain.append((T2, W2, a, i1, i2))
        pairs.append(regauge_tri(T2, G) + (a, i1, i2))
    return dict(cam8=cam8, kf1=regauge_tri(T1, G) + (a1,), pairs=pairs, unmoved=dict(kf1=(T1, W1, a1), pairs=plain), G=G)


def frustum_case(g, M=2000, n_boundary=400):
    """tests/test_mappoint_gpu.py::test_is_in_frustum's problem at M points in the world moved by the gauge, built in the moved world: the block of points
    exactly on predicted-level boundaries (maxD = dist * 1.2^k) takes its distances from the moved float inputs.  Returns the argument tuple without th."""
    from object_slam_amd.synth import KITTI_K
    rng = np.random.default_rng(11)
    K5 = np.asarray(KITTI_K, f32)[:5]
    bounds = np.array([0, 0, 1241, 376], f32)
    a = 0.1
    T0 = np.eye(4)
    T0[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    T0[:3, 3] = [0.3, -0.1, 0.5]
    G = gauge(g)
    Tcw = move_poses(T0, G)
    Pw = move_points(np.concatenate([rng.uniform(-30, 30, (M, 2)), rng.uniform(-5, 60, (M, 1))], 1), G)
    R = Tcw[:3, :3].astype(f64)
    Ow = -R.T @ Tcw[:3, 3].astype(f64)
    dirs = Pw.astype(f64) - Ow
    dist = np.linalg.norm(dirs, axis=1)
    Pn = dirs / dist[:, None] + rng.normal(0, 0.6, (M, 3))
    Pn = (Pn / np.linalg.norm(Pn, axis=1)[:, None]).astype(f32)
    sf = (1.2 ** np.arange(8)).astype(f32)
    maxD = (dist * rng.uniform(0.5, 6.0, M)).astype(f32)
    maxD[:n_boundary] = dist[:n_boundary].astype(f32) * sf[rng.integers(0, 8, n_boundary)]
    minD = (maxD / sf[-1]).astype(f32)
    obs = (rng.random(M) < 0.9).astype(np.uint8)
    desc = rng.integers(0, 256, (M, 32), dtype=np.uint8)
    logsf = f32(np.log(f32(1.2)))
    return (Pw, Pn, maxD, minD, obs, desc, Tcw, K5, bounds, 0.5, logsf, sf)
