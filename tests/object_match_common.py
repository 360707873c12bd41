"""The object association (include/oslam_hip.h, "Object association") restated sequentially in numpy, exactly as that section specifies it: float32 and float64
where it says so, loops in the orders it states.  Pairs are independent of one another, so the pair scores are evaluated for all pairs at once; the loop over the
94 bins, over the observations and over the keypoints, and the loop over the objects with its claims, run in order.  Also: hand-written cases with their answers,
seeded generators and the six-frame fixture of the adapter program.  Never imports the product."""
import functools

import numpy as np

f32, f64 = np.float32, np.float64
BINS = 94
DBL_EPSILON = float(np.finfo(f64).eps)
FLT_MAX = np.finfo(f32).max
PARAMS = dict(min_similarity=0.8, min_iou=0.5, max_mean_dist=0.3, max_min_dist=0.1)
DONE, REFUSED_RECORD, REFUSED_NO_OBSERVATION, REFUSED_NO_KEYPOINT = 0, -1, -2, -3
N_GENERATED = 200


# ------------------------------------------------------------------ appearance ------------------------------------------------------------------

@functools.lru_cache(None)
def hsv_tables():
    """sdiv, hdiv (RGB2HSV_b, hsv_shift 12) and the three calcHist tables as histogram columns (H -> 64 + bin, S -> 32 + bin, V -> bin; -1 = not counted)"""
    sdiv, hdiv = np.zeros(256, np.int64), np.zeros(256, np.int64)
    for i in range(1, 256):
        sdiv[i] = int(np.rint(f64(255 << 12) / f64(1.0 * i)))    # saturate_cast<int>(double): to nearest even
        hdiv[i] = int(np.rint(f64(180 << 12) / f64(6.0 * i)))
    cols = {}
    for name, size, low, high, first in (("h", 30, 0.0, 180.0, 64), ("s", 32, 0.0, 256.0, 32), ("v", 32, 0.0, 256.0, 0)):
        a = f64(size) / f64(high - low)
        b = -a * f64(low)
        idx = np.floor(np.arange(256, dtype=f64) * a + b).astype(np.int64)
        cols[name] = np.where((idx >= 0) & (idx < size), first + idx, -1)
    return sdiv, hdiv, cols


def bgr2hsv(b, g, r):
    """OpenCV's 8-bit BGR2HSV with hue range 180, on integers or integer arrays: (h, s, v) as uchar values"""
    sdiv, hdiv, _ = hsv_tables()
    b, g, r = (np.asarray(x, np.int64) for x in (b, g, r))
    v = np.maximum(b, np.maximum(g, r))
    vmin = np.minimum(b, np.minimum(g, r))
    diff = v - vmin
    s = (diff * sdiv[v] + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv[diff] + (1 << 11)) >> 12     # (>> of a negative int64 is arithmetic)
    h = h + np.where(h < 0, 180, 0)
    return h & 255, s & 255, v & 255


def histogram_counts(hsv, mask):
    """calcHist of the three channels over the pixels whose mask byte is non-zero, columns V, S, H: int64 [94]"""
    _, _, cols = hsv_tables()
    sel = np.asarray(mask).reshape(-1) != 0
    counts = np.zeros(BINS, np.int64)
    for ch, name in zip(hsv, ("h", "s", "v")):
        c = cols[name][np.asarray(ch).reshape(-1)[sel]]
        counts += np.bincount(c[c >= 0], minlength=BINS)
    return counts


def normalize_l1(counts):
    norm = f64(int(np.sum(counts)))
    scale = f64(1.0) / norm if norm > DBL_EPSILON else f64(0.0)
    return np.asarray(counts).astype(f32) * f32(scale)


def hsv_histograms(image, masks):
    """image uint8 [H, W, 3] (B, G, R), masks uint8 [n, H, W] -> (counts int32 [n, 94], hist float32 [n, 94])"""
    hsv = bgr2hsv(image[..., 0], image[..., 1], image[..., 2])
    counts = np.array([histogram_counts(hsv, m) for m in masks], np.int64).reshape(len(masks), BINS)
    hist = np.array([normalize_l1(c) for c in counts], f32).reshape(len(masks), BINS)
    return counts.astype(np.int32), hist


# ------------------------------------------------------------------ the matchers ------------------------------------------------------------------

def cosine(h1, h2):
    """CalCosineSimilarity of every row of h1 [n, 94] with every row of h2 [m, 94] -> float32 [n, m]; the 94 bins in order, per pair the stated arithmetic"""
    h1, h2 = np.asarray(h1, f32).reshape(-1, BINS), np.asarray(h2, f32).reshape(-1, BINS)
    n, m = len(h1), len(h2)
    xy, xx, yy = np.zeros((n, m), f32), np.zeros((n, m), f32), np.zeros((n, m), f32)
    with np.errstate(all="ignore"):
        for k in range(BINS):
            a, b = np.broadcast_to(h1[:, k, None], (n, m)), np.broadcast_to(h2[None, :, k], (n, m))
            xy = (xy + (a * b).astype(f32)).astype(f32)
            xx = (xx.astype(f64) + a.astype(f64) * a.astype(f64)).astype(f32)
            yy = (yy.astype(f64) + b.astype(f64) * b.astype(f64)).astype(f32)
        return (xy / (np.sqrt(xx).astype(f32) * np.sqrt(yy).astype(f32)).astype(f32)).astype(f32)


def box_iou(pre, cur):
    """:131-147 for one pair of boxes x, y, w, h, in float32; 0 where the reference leaves the entry unset"""
    p, c = np.asarray(pre, f32), np.asarray(cur, f32)
    with np.errstate(all="ignore"):
        pre_area, cur_area = f32(p[2] * p[3]), f32(c[2] * c[3])
        P = (p[0], p[1], f32(p[0] + p[2]), f32(p[1] + p[3]))
        Cb = (c[0], c[1], f32(c[0] + c[2]), f32(c[1] + c[3]))
        x1 = P[0] if Cb[0] < P[0] else Cb[0]      # std::max(Cur, Pre)
        x2 = P[2] if P[2] < Cb[2] else Cb[2]      # std::min(Cur, Pre)
        y1 = P[1] if Cb[1] < P[1] else Cb[1]
        y2 = P[3] if P[3] < Cb[3] else Cb[3]
        if x1 >= x2 or y1 >= y2:
            return f32(0.0)
        inter = f32(f32(x2 - x1) * f32(y2 - y1))
        return f32(inter / f32(f32(pre_area + cur_area) - inter))


def match_two_frame(p, params=PARAMS):
    """p = dict(pre=dict(obj3d, label, hist, box), cur=dict(label, hist, box, obj3d)).  Returns (cur_obj3d, similarity [nPre, nCur], iou, n_assigned)."""
    pre, cur = p["pre"], p["cur"]
    n_pre, n_cur = len(pre["label"]), len(cur["label"])
    claim = np.array(cur["obj3d"], np.int32).reshape(n_cur).copy()
    sim, iou = np.full((n_pre, n_cur), np.nan, f32), np.full((n_pre, n_cur), np.nan, f32)
    all_sim = cosine(pre["hist"], cur["hist"]) if n_pre and n_cur else sim
    assigned = 0
    for i in range(n_pre):                                   # :59, from 0
        if pre["obj3d"][i] < 0:                              # :62
            continue
        best, idx = f32(0.0), -1
        for j in range(n_cur):
            if claim[j] >= 0 or cur["label"][j] != pre["label"][i]:   # :98, :101
                continue
            sim[i, j] = all_sim[i, j]
            iou[i, j] = box_iou(pre["box"][i], cur["box"][j])
            if not np.isnan(sim[i, j]) and (idx < 0 or sim[i, j] >= best):   # a stable sort and back(): the largest index among equals
                best, idx = sim[i, j], j
        if idx >= 0 and f64(best) > params["min_similarity"] and f64(iou[i, idx]) > params["min_iou"]:   # :430
            claim[idx] = pre["obj3d"][i]
            assigned += 1
    return claim, sim, iou, assigned


def unprojected_center(kps, Rwc, Ow, K):
    """:567-573 with Frame::UnprojectStereo: float32 [3]"""
    R, Ow = np.asarray(Rwc, f32).reshape(9), np.asarray(Ow, f32).reshape(3)
    fx, fy, cx, cy = (f32(v) for v in K)
    invfx, invfy = f32(f32(1.0) / fx), f32(f32(1.0) / fy)
    s = np.zeros(3, f32)
    kps = np.asarray(kps, f32).reshape(-1, 3)
    for u, v, z in kps:
        x = f32(f32(f32(u - cx) * z) * invfx)
        y = f32(f32(f32(v - cy) * z) * invfy)
        for r in range(3):
            w = f32(f32(f32(f32(R[3 * r] * x) + f32(R[3 * r + 1] * y)) + f32(R[3 * r + 2] * z)) + Ow[r])
            s[r] = f32(s[r] + w)
    return (s * f32(f64(1.0) / f64(len(kps)))).astype(f32)


def distances(obs_center, center):
    """meanDist and minDist over the observations in order (:577-591)"""
    mean, mn = f32(0.0), FLT_MAX
    for oc in np.asarray(obs_center, f32).reshape(-1, 3):
        dx, dy, dz = (f32(oc[k] - center[k]) for k in range(3))
        d = f32(np.sqrt(f64(dx) * f64(dx) + f64(dy) * f64(dy) + f64(dz) * f64(dz)))
        mean = f32(mean + d)
        if d < mn:
            mn = d
    return f32(mean / f32(len(obs_center))), mn


def map_precondition(p):
    """the status a problem gets: DONE, or the refusal of an object without observations / a detection without keypoints"""
    if any(len(c) == 0 for c in p["objs"]["obs_center"]):
        return REFUSED_NO_OBSERVATION
    if any(len(k) == 0 for k in p["cur"]["kps"]):
        return REFUSED_NO_KEYPOINT
    return DONE


def match_map_to_frame(p, params=PARAMS):
    """p = dict(Rwc, Ow, K, cur=dict(label, hist, obj3d, kps=[arrays [n, 3]]), objs=dict(id, label, obs_center=[arrays [n, 3]], obs_hist=[arrays [n, 94]])).
    Returns (cur_obj3d, similarity [nObj, nCur], mean_dist, min_dist, n_by_similarity, n_by_distance)."""
    cur, objs = p["cur"], p["objs"]
    n_cur, n_obj = len(cur["label"]), len(objs["label"])
    claim = np.array(cur["obj3d"], np.int32).reshape(n_cur).copy()
    snapshot = set(int(c) for c in claim if c >= 0)          # :451-459
    sim, mean, mind = (np.full((n_obj, n_cur), np.nan, f32) for _ in range(3))
    centers = [unprojected_center(k, p["Rwc"], p["Ow"], p["K"]) for k in cur["kps"]]
    by_sim = by_dist = 0
    for i in range(n_obj):
        oid = int(objs["id"][i])
        if oid < 0 or oid in snapshot:                       # :468, :470
            continue
        cand = [j for j in range(n_cur) if claim[j] < 0 and cur["label"][j] == objs["label"][i]]   # :507, :512
        if cand:
            per_obs = cosine(objs["obs_hist"][i], np.asarray(cur["hist"], f32).reshape(n_cur, BINS)[cand])   # [nObs, len(cand)]
        best, idx, best2, idx2 = f32(0.0), -1, f32(0.0), -1
        for c, j in enumerate(cand):
            s = f32(0.0)
            for t in per_obs[:, c]:                          # :519-542
                if t > s:
                    s = t
            sim[i, j] = s
            mean[i, j], mind[i, j] = distances(objs["obs_center"][i], centers[j])
            if not np.isnan(s) and (idx < 0 or s >= best):   # back() of a stable sort
                best, idx = s, j
            if not np.isnan(mind[i, j]) and (idx2 < 0 or mind[i, j] < best2):   # front() of a stable sort
                best2, idx2 = mind[i, j], j
        if idx >= 0 and f64(best) > params["min_similarity"] and f64(mean[i, idx]) < params["max_mean_dist"]:   # :783
            claim[idx] = oid
            by_sim += 1
        if idx2 >= 0 and f64(best2) < params["max_min_dist"]:   # :789
            claim[idx2] = oid
            by_dist += 1
    return claim, sim, mean, mind, by_sim, by_dist


# ------------------------------------------------------------------ hand-written cases ------------------------------------------------------------------

def one_hot(*pairs):
    h = np.zeros(BINS, f32)
    for k, v in pairs:
        h[k] = v
    return h


E0, E1, E5 = one_hot((0, 1.0)), one_hot((1, 1.0)), one_hot((5, 1.0))
NEAR0 = one_hot((0, 0.9), (1, 0.1))     # cosine with E0: 0.9 / sqrt(0.82) = 0.9939
HALF = one_hot((0, 0.5), (1, 0.5))      # cosine with E0: 0.7071
BOX = (10.0, 10.0, 20.0, 20.0)
BOX_SHIFT = (15.0, 10.0, 20.0, 20.0)    # IoU with BOX: 300 / 500 = 0.6
BOX_HALF = (20.0, 10.0, 20.0, 20.0)     # IoU with BOX: 200 / 600 = 0.333
BOX_FAR = (100.0, 100.0, 20.0, 20.0)    # no overlap
NAN = float("nan")


def _pair(pre, cur, expect):
    """pre: (id, label, hist, box) each; cur: (label, hist, box, obj3d) each"""
    mk = lambda rows, keys, types: {k: np.array([r[i] for r in rows], t).reshape((len(rows),) + s) for i, (k, t, s) in enumerate(zip(keys, types, ((), (), (BINS,), (4,))))}
    P = mk(pre, ("obj3d", "label", "hist", "box"), (np.int32, np.int32, f32, f32))
    c = [(r[3], r[0], r[1], r[2]) for r in cur]
    Cd = mk(c, ("obj3d", "label", "hist", "box"), (np.int32, np.int32, f32, f32))
    return dict(pre=P, cur=Cd, expect=expect)


def hand_cases_two_frame():
    """name -> problem with expect = dict(cur, n, and optionally sim_nan / iou: the NaN pattern and the IoU entries)"""
    c = {}
    c["claim_hides_detection"] = _pair([(10, 1, E0, BOX), (11, 1, E0, BOX)], [(1, E0, BOX, -1)], dict(cur=[10], n=1, sim_nan=[[False], [True]]))
    c["labels_differ"] = _pair([(10, 1, E0, BOX)], [(2, E0, BOX, -1)], dict(cur=[-1], n=0, sim_nan=[[True]]))
    c["no_overlap_reads_as_zero"] = _pair([(10, 1, E0, BOX)], [(1, E0, BOX_FAR, -1)], dict(cur=[-1], n=0, sim_nan=[[False]], iou=[[0.0]]))
    c["similarity_tie_largest_index"] = _pair([(10, 1, E0, BOX)], [(1, E0, BOX, -1), (1, E0, BOX_SHIFT, -1)], dict(cur=[-1, 10], n=1, iou=[[1.0, 0.6]]))
    c["empty_previous_frame"] = _pair([], [(1, E0, BOX, -1), (1, E1, BOX, 4)], dict(cur=[-1, 4], n=0))
    c["no_detections"] = _pair([(10, 1, E0, BOX)], [], dict(cur=[], n=0))
    c["null_previous_object"] = _pair([(-1, 1, E0, BOX), (12, 1, E0, BOX)], [(1, E0, BOX, -1)], dict(cur=[12], n=1, sim_nan=[[True], [False]]))
    c["claimed_before_the_call"] = _pair([(10, 1, E0, BOX)], [(1, E0, BOX, 3), (1, NEAR0, BOX, -1)], dict(cur=[3, 10], n=1, sim_nan=[[True, False]]))
    c["winner_fails_iou_runner_up_ignored"] = _pair([(10, 1, E0, BOX)], [(1, E0, BOX_HALF, -1), (1, NEAR0, BOX, -1)], dict(cur=[-1, -1], n=0))
    c["similarity_below_threshold"] = _pair([(10, 1, E0, BOX)], [(1, HALF, BOX, -1)], dict(cur=[-1], n=0, iou=[[1.0]]))
    c["two_objects_two_detections_swapped"] = _pair([(10, 1, E0, BOX), (11, 1, E1, BOX_FAR)], [(1, E1, BOX_FAR, -1), (1, E0, BOX, -1)], dict(cur=[11, 10], n=2))
    return c


IDENTITY = dict(Rwc=np.eye(3, dtype=f32).reshape(9), Ow=np.zeros(3, f32), K=(1.0, 1.0, 0.0, 0.0))
C0 = (0.0, 0.0, 2.0)                    # the observed centre of the hand cases
KP_AT = [(0.0, 0.0, 2.0)]               # unprojects to C0: distance 0
KP_005 = [(0.025, 0.0, 2.0)]            # to (0.05, 0, 2)
KP_02 = [(0.1, 0.0, 2.0)]               # to (0.2, 0, 2)
KP_05 = [(0.25, 0.0, 2.0)]              # to (0.5, 0, 2)


def _map(objs, cur, expect):
    """objs: (id, label, [(centre, hist), ...]) each; cur: (label, hist, kps, obj3d) each"""
    O = dict(id=np.array([o[0] for o in objs], np.int32), label=np.array([o[1] for o in objs], np.int32),
             obs_center=[np.array([c for c, _ in o[2]], f32).reshape(-1, 3) for o in objs], obs_hist=[np.array([h for _, h in o[2]], f32).reshape(-1, BINS) for o in objs])
    Cd = dict(label=np.array([c[0] for c in cur], np.int32), hist=np.array([c[1] for c in cur], f32).reshape(-1, BINS), kps=[np.array(c[2], f32).reshape(-1, 3) for c in cur],
              obj3d=np.array([c[3] for c in cur], np.int32))
    return dict(IDENTITY, objs=O, cur=Cd, expect=expect)


def hand_cases_map():
    """name -> problem with expect = dict(cur, by_sim, by_dist)"""
    c = {}
    c["both_rules_fire_onto_two_detections"] = _map([(7, 1, [(C0, E0)])], [(1, E0, KP_02, -1), (1, NEAR0, KP_005, -1)], dict(cur=[7, 7], by_sim=1, by_dist=1))
    c["distance_tie_smallest_index"] = _map([(7, 1, [(C0, E0)])], [(1, E5, KP_005, -1), (1, E5, KP_005, -1)], dict(cur=[7, -1], by_sim=0, by_dist=1))
    c["similarity_tie_largest_index"] = _map([(7, 1, [(C0, E0)])], [(1, E0, KP_02, -1), (1, E0, KP_02, -1)], dict(cur=[-1, 7], by_sim=1, by_dist=0))
    c["already_matched_snapshot"] = _map([(7, 1, [(C0, E0)]), (8, 1, [(C0, E0)])], [(1, E5, KP_05, 7), (1, E0, KP_AT, -1)], dict(cur=[7, 8], by_sim=1, by_dist=1))
    c["empty_map"] = _map([], [(1, E0, KP_AT, -1), (2, E0, KP_AT, 5)], dict(cur=[-1, 5], by_sim=0, by_dist=0))
    c["no_detections"] = _map([(7, 1, [(C0, E0)])], [], dict(cur=[], by_sim=0, by_dist=0))
    c["claim_hides_detection"] = _map([(3, 1, [(C0, E0)]), (4, 1, [(C0, E0)])], [(1, E0, KP_AT, -1)], dict(cur=[3], by_sim=1, by_dist=1))
    c["labels_differ"] = _map([(7, 1, [(C0, E0)])], [(2, E0, KP_AT, -1)], dict(cur=[-1], by_sim=0, by_dist=0))
    c["similar_but_far"] = _map([(7, 1, [(C0, E0)])], [(1, E0, KP_05, -1)], dict(cur=[-1], by_sim=0, by_dist=0))
    c["maximum_over_observations"] = _map([(7, 1, [(C0, E1), (C0, E0), (C0, E5)])], [(1, E0, KP_02, -1)], dict(cur=[7], by_sim=1, by_dist=0))
    c["mean_too_far_min_near"] = _map([(7, 1, [(C0, E0), ((1.0, 0.0, 2.0), E0)])], [(1, E0, KP_005, -1)], dict(cur=[7], by_sim=0, by_dist=1))
    c["null_object"] = _map([(-1, 1, [(C0, E0)]), (9, 1, [(C0, HALF)])], [(1, E0, KP_02, -1)], dict(cur=[-1], by_sim=0, by_dist=0))
    return c


# ------------------------------------------------------------------ generators ------------------------------------------------------------------

def _bases(rng, n=6):
    """appearance prototypes: L1-normalised, a few strong bins per block as a mask of one colour family gives"""
    out = []
    for _ in range(n):
        h = np.zeros(BINS)
        for lo, hi in ((0, 32), (32, 64), (64, 94)):
            k = rng.integers(lo, hi, 3)
            h[k] += rng.random(3) + 0.2
        out.append(h / h.sum())
    return out


def _appearance(rng, base, noise):
    h = base + noise * rng.random(BINS) / BINS * 3.0
    return (h / h.sum()).astype(f32)


def gen_two_frame(seed):
    rng = np.random.default_rng(seed)
    bases = _bases(rng)
    n_pre, n_cur = int(rng.integers(0, 9)), int(rng.integers(0, 9))
    pre = dict(obj3d=np.zeros(n_pre, np.int32), label=np.zeros(n_pre, np.int32), hist=np.zeros((n_pre, BINS), f32), box=np.zeros((n_pre, 4), f32))
    proto = rng.integers(0, len(bases), n_pre)
    for i in range(n_pre):
        pre["obj3d"][i] = -1 if rng.random() < 0.15 else 100 + i
        pre["label"][i] = proto[i] % 3
        pre["hist"][i] = _appearance(rng, bases[proto[i]], 0.05)
        pre["box"][i] = (rng.uniform(0, 500), rng.uniform(0, 350), rng.uniform(30, 120), rng.uniform(30, 120))
    cur = dict(obj3d=np.full(n_cur, -1, np.int32), label=np.zeros(n_cur, np.int32), hist=np.zeros((n_cur, BINS), f32), box=np.zeros((n_cur, 4), f32))
    order = rng.permutation(max(n_pre, n_cur))
    for j in range(n_cur):
        src = int(order[j]) if n_pre and order[j] < n_pre and rng.random() < 0.8 else -1
        if src >= 0:     # the object seen again: appearance noise and box motion of three sizes, so that both thresholds are straddled
            cur["label"][j] = pre["label"][src] if rng.random() < 0.9 else (pre["label"][src] + 1) % 3
            cur["hist"][j] = _appearance(rng, bases[proto[src]], rng.choice([0.05, 0.6, 2.5]))
            shift = rng.choice([0.05, 0.35, 0.8]) * pre["box"][src][2:]
            cur["box"][j] = np.concatenate([pre["box"][src][:2] + shift * rng.choice([-1, 1], 2), pre["box"][src][2:] * rng.uniform(0.9, 1.1, 2)])
        else:
            k = int(rng.integers(0, len(bases)))
            cur["label"][j], cur["hist"][j] = k % 3, _appearance(rng, bases[k], 0.3)
            cur["box"][j] = (rng.uniform(0, 500), rng.uniform(0, 350), rng.uniform(30, 120), rng.uniform(30, 120))
        if rng.random() < 0.1:
            cur["obj3d"][j] = 900 + j
    return dict(pre=pre, cur=cur)


def _rotation(rng, angle):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def gen_map(seed, n_obs_override=None):
    rng = np.random.default_rng(seed)
    bases = _bases(rng)
    n_obj, n_cur = int(rng.integers(0, 13)), int(rng.integers(0, 9))
    Rwc, Ow = _rotation(rng, rng.uniform(0, 0.5)), rng.uniform(-3, 3, 3)
    K = (520.0, 515.0, 320.0, 240.0)
    objs = dict(id=np.zeros(n_obj, np.int32), label=np.zeros(n_obj, np.int32), obs_center=[], obs_hist=[])
    proto, centers = rng.integers(0, len(bases), n_obj), []
    for i in range(n_obj):
        objs["id"][i] = -1 if rng.random() < 0.08 else 10 + i
        objs["label"][i] = proto[i] % 3
        c = Ow + Rwc @ np.array([rng.uniform(-2, 2), rng.uniform(-1, 1), rng.uniform(2, 6)])
        centers.append(c)
        n_obs = int(rng.integers(1, 41)) if n_obs_override is None or i else n_obs_override
        spread = rng.choice([0.01, 0.05, 0.2])
        objs["obs_center"].append((c + rng.normal(size=(n_obs, 3)) * spread).astype(f32))
        objs["obs_hist"].append(np.array([_appearance(rng, bases[proto[i]], rng.choice([0.05, 0.5, 2.5])) for _ in range(n_obs)], f32))
    cur = dict(obj3d=np.full(n_cur, -1, np.int32), label=np.zeros(n_cur, np.int32), hist=np.zeros((n_cur, BINS), f32), kps=[])
    order = rng.permutation(max(n_obj, n_cur))
    for j in range(n_cur):
        src = int(order[j]) if n_obj and order[j] < n_obj and rng.random() < 0.8 else -1
        if src >= 0:
            cur["label"][j] = objs["label"][src] if rng.random() < 0.9 else (objs["label"][src] + 1) % 3
            cur["hist"][j] = _appearance(rng, bases[proto[src]], rng.choice([0.05, 0.6, 2.5]))
            off = rng.normal(size=3)
            c = centers[src] + off / np.linalg.norm(off) * rng.choice([0.02, 0.07, 0.2, 0.6])
        else:
            k = int(rng.integers(0, len(bases)))
            cur["label"][j], cur["hist"][j] = k % 3, _appearance(rng, bases[k], 0.3)
            c = Ow + Rwc @ np.array([rng.uniform(-2, 2), rng.uniform(-1, 1), rng.uniform(2, 6)])
        pts = c + rng.normal(size=(int(rng.integers(1, 30)), 3)) * 0.03
        pc = (pts - Ow) @ Rwc            # Rwc^T (p - Ow), row-wise
        pc[:, 2] = np.maximum(pc[:, 2], 0.3)
        cur["kps"].append(np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3], pc[:, 2]], 1).astype(f32))
        if rng.random() < 0.1:
            cur["obj3d"][j] = int(objs["id"][rng.integers(0, n_obj)]) if n_obj and rng.random() < 0.5 else 900 + j
    return dict(Rwc=Rwc.astype(f32).reshape(9), Ow=Ow.astype(f32), K=K, objs=objs, cur=cur)


@functools.lru_cache(None)
def generated_two_frame():
    """(problems, answers): N_GENERATED problems; the decision of :430 fires in at least a fifth of them and in at least a fifth it does not"""
    ps = [gen_two_frame(1000 + s) for s in range(N_GENERATED)]
    ans = [match_two_frame(p) for p in ps]
    fired = sum(a[3] > 0 for a in ans)
    assert 5 * fired >= N_GENERATED and 5 * (N_GENERATED - fired) >= N_GENERATED, fired
    return ps, ans


@functools.lru_cache(None)
def generated_map():
    """(problems, answers): N_GENERATED problems, one of them with an object of 129 observations; each rule of :783 / :789 fires in at least a fifth, and not in a fifth"""
    ps = [gen_map(5000 + s, n_obs_override=129 if s == 7 else None) for s in range(N_GENERATED)]
    assert any(len(c) == 129 for c in ps[7]["objs"]["obs_center"])
    ans = [match_map_to_frame(p) for p in ps]
    for k in (4, 5):
        fired = sum(a[k] > 0 for a in ans)
        assert 5 * fired >= N_GENERATED and 5 * (N_GENERATED - fired) >= N_GENERATED, (k, fired)
    return ps, ans


def gen_image(rng, W, H, stride=None):
    """uint8 [H, stride]: random colours, with runs of greys, saturated primaries and near-ties of two channels mixed in"""
    stride = 3 * W if stride is None else stride
    px = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    kind = rng.integers(0, 6, (H, W))
    px[kind == 0] = px[kind == 0][:, :1]                                  # greys
    px[kind == 1] = (px[kind == 1] > 127).astype(np.uint8) * 255             # corners of the cube
    px[kind == 2, 1] = px[kind == 2, 0]                                      # b == g
    img = rng.integers(0, 256, (H, stride), dtype=np.uint8)                 # (the padding bytes are not zero)
    img[:, :3 * W] = px.reshape(H, 3 * W)
    return img, px


def gen_masks(rng, n, W, H, mask_stride=None, values=(0, 255)):
    mask_stride = W if mask_stride is None else mask_stride
    m = rng.integers(1, 256, (n, H, mask_stride), dtype=np.uint8)              # (padding bytes set)
    for k in range(n):
        x0, x1 = sorted(rng.integers(0, W + 1, 2))
        y0, y1 = sorted(rng.integers(0, H + 1, 2))
        blob = np.zeros((H, W), np.uint8)
        blob[y0:y1, x0:x1] = 1
        blob ^= (rng.random((H, W)) < 0.1).astype(np.uint8)
        m[k, :, :W] = np.where(blob != 0, rng.choice(values[1:], (H, W)), values[0])
    return m


# ------------------------------------------------------------------ the caller program's fixture ------------------------------------------------------------------

FIXTURE_W, FIXTURE_H = 48, 32
FIXTURE_K = (40.0, 40.0, 24.0, 16.0)


def fixture_frames():
    """Six frames of three objects (a red, a green and a blue block in front of a grey wall), label 1, 1 and 2.  Object 1 leaves after frame 1 and is back in frame
    4, where MatchTwoFrame cannot know it and the map rule recovers it; the two objects that stay swap their order in the detection list between frames 2 and 3.
    Returns a list of dict(image [H, 3W], Rwc, Ow, dets=[dict(label, mask [H, W], box, kps [n, 3], center [3])])."""
    rng = np.random.default_rng(77)
    colours = {0: (30, 40, 220), 1: (40, 200, 50), 2: (210, 60, 30)}          # B, G, R
    labels = {0: 1, 1: 1, 2: 2}
    world = {0: np.array([-0.5, 0.0, 3.0]), 1: np.array([0.0, 0.1, 3.0]), 2: np.array([0.5, -0.1, 3.0])}
    visible = [[0, 1, 2], [0, 1, 2], [0, 2], [2, 0], [2, 1, 0], [1, 0, 2]]
    frames = []
    for f, vis in enumerate(visible):
        Ow = np.array([0.02 * f, 0.0, 0.0])
        Rwc = np.eye(3)
        img = np.full((FIXTURE_H, FIXTURE_W, 3), 128, np.uint8) + rng.integers(0, 3, (FIXTURE_H, FIXTURE_W, 3), dtype=np.uint8)
        dets = []
        for o in vis:
            pc = world[o] - Ow
            u, v = FIXTURE_K[0] * pc[0] / pc[2] + FIXTURE_K[2], FIXTURE_K[1] * pc[1] / pc[2] + FIXTURE_K[3]
            x0, y0 = int(round(u)) - 3, int(round(v)) - 4
            mask = np.zeros((FIXTURE_H, FIXTURE_W), np.uint8)
            mask[y0:y0 + 8, x0:x0 + 6] = 255
            img[mask != 0] = np.array(colours[o], np.uint8) + rng.integers(0, 4, (48, 3), dtype=np.uint8)
            pts = world[o] + rng.normal(size=(5, 3)) * 0.01
            q = pts - Ow
            kps = np.stack([FIXTURE_K[0] * q[:, 0] / q[:, 2] + FIXTURE_K[2], FIXTURE_K[1] * q[:, 1] / q[:, 2] + FIXTURE_K[3], q[:, 2]], 1).astype(f32)
            dets.append(dict(label=labels[o], mask=mask, box=np.array([x0, y0, 6, 8], f32), kps=kps, truth=o))
        for d in dets:
            d["center"] = unprojected_center(d["kps"], Rwc, Ow, FIXTURE_K)      # what the map layer records as ObjectCenterW
        frames.append(dict(image=np.ascontiguousarray(img.reshape(FIXTURE_H, 3 * FIXTURE_W)), Rwc=Rwc.astype(f32).reshape(9), Ow=Ow.astype(f32), dets=dets))
    return frames


def track_fixture(frames, params=PARAMS):
    """Tracking::TrackObject over the frames with the map bookkeeping of the Object3D constructor and Object3D::Update (src/ObjectTypes.cc:44-45, :131-132): the
    track ids per frame, and per frame how many claims each operator made"""
    objects, prev, next_id, ids, claims = {}, None, 0, [], []
    for F in frames:
        dets = F["dets"]
        n = len(dets)
        _, hist = hsv_histograms(F["image"].reshape(FIXTURE_H, FIXTURE_W, 3), np.array([d["mask"] for d in dets], np.uint8).reshape(n, FIXTURE_H, FIXTURE_W))
        cur = dict(label=np.array([d["label"] for d in dets], np.int32), hist=hist, box=np.array([d["box"] for d in dets], f32).reshape(n, 4), obj3d=np.full(n, -1, np.int32),
                   kps=[d["kps"] for d in dets])
        two = 0
        if prev is not None:
            pre = dict(obj3d=prev["obj3d"], label=np.array([objects[int(t)]["label"] if t >= 0 else 0 for t in prev["obj3d"]], np.int32), hist=prev["hist"], box=prev["box"])
            cur["obj3d"], _, _, two = match_two_frame(dict(pre=pre, cur=cur), params)
        order = sorted(objects)       # ascending mTrackID
        objs = dict(id=np.array(order, np.int32), label=np.array([objects[t]["label"] for t in order], np.int32), obs_center=[np.array(objects[t]["center"], f32) for t in order],
                    obs_hist=[np.array(objects[t]["hist"], f32) for t in order])
        cur["obj3d"], _, _, _, by_sim, by_dist = match_map_to_frame(dict(Rwc=F["Rwc"], Ow=F["Ow"], K=FIXTURE_K, cur=cur, objs=objs), params)
        for j, d in enumerate(dets):
            t = int(cur["obj3d"][j])
            if t < 0:
                t = next_id
                next_id += 1
                objects[t] = dict(label=d["label"], center=[], hist=[])
                cur["obj3d"][j] = t
            objects[t]["center"].append(d["center"])
            objects[t]["hist"].append(hist[j])
        ids.append([int(t) for t in cur["obj3d"]])
        claims.append((two, by_sim, by_dist))
        prev = cur
    return ids, claims
