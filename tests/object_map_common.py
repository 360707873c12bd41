"""The numpy restatement of the object map maintenance (include/oslam_hip.h, "Object map maintenance"), operator by operator in the header's arithmetic, with hand
cases and seeded generators.  The connected components come from a plain union-find over the all-pairs float32 test.  Written from the header's formulas; no GPU."""
import numpy as np

f32, f64 = np.float32, np.float64
MODE_UPDATE, MODE_NEW_OBJECT = 0, 1
PATH_TEST5, PATH_TEST7, PATH_SHORTCUT = 0, 1, 2
TOL2 = f32(0.1 * 0.1)


def quiet(a):
    """every NaN becomes the quiet NaN 0x7fc00000"""
    a = np.array(a, f32)
    a[np.isnan(a)] = np.nan
    return a


def seq_sum(v):
    """the float32 sum 0 + v[0] + v[1] + ... in order"""
    return np.cumsum(np.concatenate([np.zeros(1, f32), np.asarray(v, f32)]), dtype=f32)[-1]


def norm3(v):
    """cv::norm of float32 vectors [., 3]: squares and sum in double"""
    v = np.asarray(v, f32).astype(f64).reshape(-1, 3)
    return np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])


def label_bad(cnt, total):
    cnt, total = np.asarray(cnt, np.int64), np.asarray(total, np.int64)
    with np.errstate(all="ignore"):
        prob = np.where(total == 0, f32(0), (cnt.astype(f64) / total.astype(f64)).astype(f32))
    return prob.astype(f64) < 0.5


def components(pos):
    """per point the smallest index of its connected component under d2 < (float)(0.1 * 0.1); -1 for a point with a non-finite coordinate"""
    pos = np.asarray(pos, f32).reshape(-1, 3)
    n = len(pos)
    ok = np.isfinite(pos).all(axis=1)
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    with np.errstate(all="ignore"):
        for i0 in range(0, n, 512):
            blk = pos[i0:i0 + 512]
            dx, dy, dz = blk[:, None, 0] - pos[None, :, 0], blk[:, None, 1] - pos[None, :, 1], blk[:, None, 2] - pos[None, :, 2]
            d2 = dx * dx + dy * dy + dz * dz
            assert d2.dtype == f32
            ii, jj = np.nonzero(d2 < TOL2)
            for i, j in zip((ii + i0).tolist(), jj.tolist()):
                if i < j:
                    a, b = find(i), find(j)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    return np.array([find(i) if ok[i] else -1 for i in range(n)], np.int32)


def center_and_size(pos):
    """CalculateCenterAndSize: (center [3], bbox [6] = max x, y, z, min x, y, z), or (None, None) for an empty list"""
    pos = np.asarray(pos, f32).reshape(-1, 3)
    if len(pos) == 0:
        return None, None
    with np.errstate(all="ignore"):
        center = np.array([seq_sum(pos[:, c]) / f32(len(pos)) for c in range(3)], f32)
    mx, mn = [], []
    for c in range(3):
        v = pos[:, c][~np.isnan(pos[:, c])]
        mx.append(v[np.argmax(v)] if len(v) else f32(-np.inf))   # the first of equal values, as a strict comparison leaves it
        mn.append(v[np.argmin(v)] if len(v) else f32(np.inf))
    return quiet(center), np.array(mx + mn, f32)


def reject_outliers(pos, label_cnt=None, label_sum=None, mode=MODE_UPDATE):
    pos = np.asarray(pos, f32).reshape(-1, 3)
    n = len(pos)
    bad = label_bad(label_cnt, label_sum) if mode == MODE_UPDATE else np.zeros(n, bool)
    ci = np.nonzero(~bad)[0]
    N = len(ci)
    cp = pos[ci]
    with np.errstate(all="ignore"):
        square = norm3(cp).astype(f32)
        square_sum = seq_sum(square * square)
        inv = f32(f64(1.0) / f64(N))
        cc = np.array([seq_sum(cp[:, c]) * inv for c in range(3)], f32)
        nrm = norm3(cc)[0]
        variance = f64(square_sum) / f64(N) - nrm * nrm
        std = f32(np.sqrt(variance))
        thr = f32(3.0) * std
        dist = norm3(cp - cc[None, :]).astype(f32)   # (the squares of Center - PosW are those of PosW - Center)
    keep = np.zeros(n, np.uint8)
    cluster = np.full(n, -1, np.int32)
    n_clusters = 0
    if mode == MODE_UPDATE and n > 3000:
        path = PATH_TEST5
        keep[ci] = ~(dist > thr)
    else:
        path = PATH_TEST7
        comp = components(cp)
        inc = comp >= 0
        cluster[ci[inc]] = ci[comp[inc]]
        roots, sizes = np.unique(comp[inc], return_counts=True)
        n_clusters = len(roots)
        if mode == MODE_NEW_OBJECT and n_clusters == 1 and N > 5:
            path = PATH_SHORTCUT
            keep[:] = 1
        else:
            size_of = dict(zip(roots.tolist(), sizes.tolist()))
            kc = np.ones(N, bool)
            for k in range(N):
                if not inc[k]:
                    continue
                ratio = f32(f64(size_of[int(comp[k])]) / f64(N))
                if f64(ratio) < 0.1 and N > 15:
                    kc[k] = False
                elif dist[k] > thr:
                    kc[k] = False
            keep[ci] = kc
    center, bbox = center_and_size(pos[keep != 0])
    return dict(keep=keep, cluster=cluster, n_candidates=N, n_clusters=n_clusters, n_kept=int(keep.sum()), path=path, std_dev=quiet(std)[()], candidates_center=quiet(cc),
                center=center, bbox=bbox, variance=float(variance))


def overlap_ratio(b1, b2):
    """ObjectMatcher::Compute3DOverlapRatio on boxes max x, y, z, min x, y, z, in float32"""
    b1, b2 = np.asarray(b1, f32), np.asarray(b2, f32)
    with np.errstate(all="ignore"):
        area1 = (b1[0] - b1[3]) * (b1[1] - b1[4]) * (b1[2] - b1[5])
        area2 = (b2[0] - b2[3]) * (b2[1] - b2[4]) * (b2[2] - b2[5])
        lo = [b2[3 + c] if b1[3 + c] < b2[3 + c] else b1[3 + c] for c in range(3)]   # std::max(a, b)
        hi = [b2[c] if b2[c] < b1[c] else b1[c] for c in range(3)]                  # std::min(a, b)
        if lo[0] >= hi[0] or lo[1] >= hi[1] or lo[2] >= hi[2]:
            return f32(0)
        inter = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])
        q1, q2 = inter / area1, inter / area2
        return quiet(q2 if q1 < q2 else q1)[()]


def merge_sets(label, track_id, bbox):
    """(ratio [n, n] with NaN below and on the diagonal, sets as a list of (sorted members, target))"""
    n = len(label)
    bbox = np.asarray(bbox, f32).reshape(n, 6)
    ratio = np.full((n, n), np.nan, f32)
    sets = []
    for i in range(n):
        for j in range(i + 1, n):
            ratio[i, j] = overlap_ratio(bbox[i], bbox[j])
            if label[i] == label[j] and track_id[i] != track_id[j] and f64(ratio[i, j]) > 0.4:
                inserted = False
                for s in sets:
                    if i in s or j in s:
                        s.add(i)
                        s.add(j)
                        inserted = True
                if not inserted:
                    sets.append({i, j})
    out = []
    for s in sets:
        mem = sorted(s)
        best = mem[0]
        for o in mem[1:]:
            if track_id[o] > track_id[best]:
                best = o
        out.append((mem, best))
    return ratio, out


# ------------------------------------------------------------------ hand cases ------------------------------------------------------------------

def _line(n, x0=0.0, step=0.09):
    p = np.zeros((n, 3), f32)
    p[:, 0] = (x0 + step * np.arange(n)).astype(f32)
    return p


def _case(pos, keep, mode=MODE_UPDATE, bad=(), cnt=None, total=None, **expect):
    pos = np.asarray(pos, f32).reshape(-1, 3)
    n = len(pos)
    cnt = np.full(n, 3, np.int32) if cnt is None else np.asarray(cnt, np.int32)
    total = np.full(n, 4, np.int32) if total is None else np.asarray(total, np.int32)   # probability 0.75
    for r in bad:
        cnt[r] = 1   # probability 0.25
    return dict(pos=pos, cnt=cnt, total=total, mode=mode, keep=np.asarray(keep, np.uint8), expect=expect)


def hand_cases():
    """name -> dict(pos, cnt, total, mode, keep = the answer worked out by hand, expect = further hand answers among the restatement's keys)"""
    c = {}
    c["n0"] = _case(np.zeros((0, 3)), [], n_candidates=0, n_clusters=0, n_kept=0, path=PATH_TEST7)
    # one point: Center is the point, SquareSum / 1 - |Center|^2 = 0, dist 0 > 0 is false
    c["n1"] = _case([[1, 0, 0]], [1], n_clusters=1, std_dev=f32(0))
    # 0 and 0.05: Center 0.025, variance 0.00125 - 0.000625, sigma 0.025, both at 0.025 < 0.075
    c["n2"] = _case([[0, 0, 0], [0.05, 0, 0]], [1, 1], n_clusters=1, cluster=[0, 0])
    c["every_point_bad"] = _case([[0, 0, 0], [0.01, 0, 0], [0, 0.01, 0], [0, 0, 0.01]], [0, 0, 0, 0], bad=(0, 1, 2, 3), n_candidates=0, n_kept=0, cluster=[-1] * 4)
    # row 1 has an empty label map: probability 0.  The others: Center (1/60, 1/60, 0), sigma 1/30, distances 0.024 and 0.037 < 0.1
    c["label_sum_0"] = _case([[0, 0, 0], [0.02, 0.02, 0], [0.05, 0, 0], [0, 0.05, 0]], [1, 0, 1, 1], total=[4, 0, 4, 4], n_candidates=3, cluster=[0, -1, 0, 0])
    # 14 on a line and one point 0.3 past its end: 15 candidates, the cluster rule is off (N > 15 fails); sigma 0.414, the far point at 0.826 < 1.243
    c["15_candidates_far_point_stays"] = _case(np.concatenate([_line(14), [[1.47, 0, 0]]]), [1] * 15, n_clusters=2)
    # 15 on a line and one far point: 16 candidates, ratio 1/16 < 0.1: dropped; sigma 0.439, the line within 0.688 < 1.316
    c["16_candidates_far_point_goes"] = _case(np.concatenate([_line(15), [[1.56, 0, 0]]]), [1] * 15 + [0], n_clusters=2)
    # 18 + 2: ratio = (float)0.1 = 0.100000001490116 is not < 0.1; sigma 0.554, the pair at most 1.044 < 1.663
    c["20_candidates_pair_stays"] = _case(np.concatenate([_line(18), [[1.83, 0, 0], [1.92, 0, 0]]]), [1] * 20, n_clusters=2)
    # 19 + 2: ratio 2/21 = 0.095 < 0.1: dropped
    c["21_candidates_pair_goes"] = _case(np.concatenate([_line(19), [[1.92, 0, 0], [2.01, 0, 0]]]), [1] * 19 + [0, 0], n_clusters=2)
    # 0.1f * 0.1f rounds to 0.010000000707805 > (float)0.01 = 0.009999999776483: not neighbours.  Center 0.05, sigma 0.05, both at 0.05 < 0.15
    c["gap_0.1f_not_neighbours"] = _case([[0, 0, 0], [f32(0.1), 0, 0]], [1, 1], n_clusters=2, cluster=[0, 1])
    c["gap_0.0999f_neighbours"] = _case([[0, 0, 0], [f32(0.0999), 0, 0]], [1, 1], n_clusters=1, cluster=[0, 0])
    c["duplicated_point"] = _case([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.55, 0.5, 0.5]], [1, 1, 1], n_clusters=1, cluster=[0, 0, 0])
    # a uniform line of length L: sigma L / sqrt(12), 3 sigma = 0.87 L above the half length: everything stays, one cluster whatever the order
    for name, n, seed in (("line_70_shuffled", 70, 1), ("line_300_shuffled", 300, 2)):
        p = _line(n)[np.random.default_rng(seed).permutation(n)]
        c[name] = _case(p, [1] * n, n_clusters=1, cluster=[0] * n, path=PATH_TEST7)
    # two blobs 0.16 apart and a bridge at 0.08: the bridge is within 0.0854 of every blob point; sigma 0.07, the farthest at 0.083 < 0.21
    blob = np.array([[0, 0, 0], [0, 0.03, 0], [0, 0, 0.03]], f32)
    c["two_blobs_and_a_bridge"] = _case(np.concatenate([blob, blob + f32([0.16, 0, 0]), [[0.08, 0, 0]]]), [1] * 7, n_clusters=1, cluster=[0] * 7)
    c["two_blobs_without_the_bridge"] = _case(np.concatenate([blob, blob + f32([0.16, 0, 0])]), [1] * 6, n_clusters=2, cluster=[0, 0, 0, 3, 3, 3])
    # near (1000, 1000, 1000) SquareSum is a float at 2.4e7 (spacing 2) and the true variance 0.0004: the simplified variance is rounding noise, here negative
    # (the CPU test asserts that the restatement says so): sigma NaN, no distance exceeds NaN.  One cluster of 8.
    off = f32([1000, 1000, 1000])
    cloud = np.array([[0, 0, 0], [0.03, 0, 0], [0, 0.03, 0], [0, 0, 0.03], [0.03, 0.03, 0], [0.03, 0, 0.03], [0, 0.03, 0.03], [0.03, 0.03, 0.03]], f32)
    c["negative_variance_far_from_origin"] = _case(cloud + off, [1] * 8, n_clusters=1, negative_variance=True)
    # NEW_OBJECT.  Near (100, 100, 100) the simplified sigma of a chain of true sigma 0.09 is rounding noise again: for these rows it comes out positive and
    # far too small (the CPU test asserts 3 sigma below the distance of the rows marked), so they are 3-sigma outliers.  Six points in one cluster: the shortcut
    # keeps them.  Five: no shortcut, the rule drops them.
    c["new_object_6_points_shortcut"] = _case(NEW6, [1] * 6, mode=MODE_NEW_OBJECT, n_clusters=1, path=PATH_SHORTCUT, outliers=NEW6_OUT)
    c["new_object_5_points_no_shortcut"] = _case(NEW5, NEW5_KEEP, mode=MODE_NEW_OBJECT, n_clusters=1, path=PATH_TEST7, outliers=[k for k in range(5) if not NEW5_KEEP[k]])
    # 2998 on a line and a pair 0.3 past its end, 135 from the centre with sigma 78: at n = 3000 TEST7 drops the pair as a small cluster, at n = 3001 (one more
    # line point) TEST5 knows no clusters and keeps everything
    p = np.concatenate([_line(2998), [[f32(0.09 * 2997 + 0.3), 0, 0], [f32(0.09 * 2997 + 0.39), 0, 0]]])
    perm = np.random.default_rng(3).permutation(3000)
    keep = np.ones(3000, np.uint8)
    keep[np.nonzero(perm >= 2998)[0]] = 0
    c["n3000_test7"] = _case(p[perm], keep, n_clusters=2, path=PATH_TEST7)
    p = np.concatenate([_line(2999), [[f32(0.09 * 2998 + 0.3), 0, 0], [f32(0.09 * 2998 + 0.39), 0, 0]]])
    c["n3001_test5"] = _case(p[np.random.default_rng(4).permutation(3001)], [1] * 3001, n_clusters=0, path=PATH_TEST5, cluster=[-1] * 3001)
    # a NaN coordinate: the row is a candidate and in no cluster; Center and sigma are NaN, so nothing is a 3-sigma outlier
    c["nan_coordinate"] = _case([[0, 0, 0], [0.05, 0, 0], [np.nan, 0.02, 0], [0, 0.05, 0]], [1, 1, 1, 1], n_clusters=1, cluster=[0, 0, -1, 0], n_candidates=4)
    return c


# found with this file's restatement by trying offsets; the numbers are fixed here, and what makes them cases is asserted by tests/test_object_map_cpu.py
NEW6 = _line(6) + f32([374.5, 388.75, 55.25])     # simplified sigma 0.033: rows 0, 1, 4, 5 lie beyond 0.099 from the centre
NEW6_OUT = [0, 1, 4, 5]
NEW5 = _line(5) + f32([356.25, 379.5, 141.75])    # simplified sigma 0.0327: the end points, 0.18 from the centre, lie beyond 0.098
NEW5_KEEP = [0, 1, 1, 1, 0]


def _unit_box(x, y=0.0, z=0.0, sx=1.0):
    return [x + sx, y + 1.0, z + 1.0, x, y, z]


def merge_hand_cases():
    """name -> dict(label, track_id, bbox, sets = the answer by hand as (members, target))"""
    c = {}
    # unit cubes half a side apart overlap by 0.5 > 0.4; a whole side apart they only touch
    c["chain_is_one_set"] = dict(label=[1] * 4, track_id=[10, 11, 12, 13], bbox=[_unit_box(0.5 * k) for k in range(4)], sets=[([0, 1, 2, 3], 3)])
    # a, c, d, b in the caller's order: pairs (0,3) = a-b, then (1,2) = c-d, then (1,3) = c-b, which touches both sets
    c["pair_lands_in_both_sets"] = dict(label=[1] * 4, track_id=[10, 12, 13, 11], bbox=[_unit_box(0.0), _unit_box(1.0), _unit_box(1.5), _unit_box(0.5)],
                                        sets=[([0, 1, 3], 1), ([1, 2, 3], 2)])
    c["equal_track_ids"] = dict(label=[1, 1], track_id=[4, 4], bbox=[_unit_box(0.0), _unit_box(0.5)], sets=[])
    c["label_mismatch"] = dict(label=[1, 2], track_id=[4, 5], bbox=[_unit_box(0.0), _unit_box(0.5)], sets=[])
    c["zero_volume_box"] = dict(label=[1, 1], track_id=[4, 5], bbox=[_unit_box(0.0), [1.5, 1.0, 0.5, 0.5, 0.0, 0.5]], sets=[])
    # 1 and 2 share a track id and do not merge with each other; both merge with 0: the first of the two largest ids is the target
    c["tie_for_the_largest_track_id"] = dict(label=[1] * 3, track_id=[5, 7, 7], bbox=[_unit_box(0.0), _unit_box(0.25), _unit_box(0.5)], sets=[([0, 1, 2], 1)])
    c["empty_map"] = dict(label=[], track_id=[], bbox=np.zeros((0, 6)), sets=[])
    c["one_object"] = dict(label=[1], track_id=[0], bbox=[_unit_box(0.0)], sets=[])
    return c


# ------------------------------------------------------------------ generators ------------------------------------------------------------------

def gen_points(rng, n):
    """n map points: jittered-grid blobs, a shuffled line, scattered outliers, at a world offset up to 1000; labels with bad rows and empty label maps"""
    off = f32(rng.choice([0.0, 1.0, 30.0, 300.0, 1000.0])) * (rng.uniform(0.5, 1, 3) * rng.choice([-1, 1], 3)).astype(f32)
    parts, left = [], n
    single = rng.random() < 0.3    # one blob or one line: one cluster, the case of the shortcut
    while left > 0:
        kind = rng.integers(2) if single else rng.integers(4)
        m = left if single else int(min(left, rng.integers(1, max(2, n // 2 + 1))))
        if kind == 0:      # a blob: a jittered grid of spacing 0.07, every point within 0.1 of its axis neighbours
            side = int(np.ceil(m ** (1 / 3)))
            g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(side ** 3)[:m]]
            p = g * 0.07 + rng.uniform(-0.01, 0.01, (m, 3)) + rng.uniform(-0.5, 0.5, 3)
        elif kind == 1:    # a line in a random direction
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            p = np.arange(m)[:, None] * 0.09 * d[None, :] + rng.uniform(-0.5, 0.5, 3)
        elif kind == 2:    # outliers
            m = min(m, 5)
            p = rng.uniform(-3, 3, (m, 3))
        else:              # a small far cluster
            m = min(m, 4)
            p = rng.uniform(-0.03, 0.03, (m, 3)) + rng.uniform(-2, 2, 3)
        parts.append(p)
        left -= m
    pos = (np.concatenate(parts) if parts else np.zeros((0, 3))).astype(f32)[:n]
    pos = (pos[rng.permutation(n)] + off[None, :]).astype(f32)
    total = rng.integers(0, 9, n).astype(np.int32)
    cnt = np.minimum(total, rng.integers(0, 9, n)).astype(np.int32)
    good = rng.random(n) < 0.8
    cnt[good], total[good] = 3, 4
    return pos, cnt, total


def generated(mode, count=200, seed=5):
    """`count` problems of n drawn from 0 .. 400: a list of dict(pos, cnt, total, mode)"""
    rng = np.random.default_rng(seed + mode)
    out = []
    for k in range(count):
        n = int(rng.integers(0, 401)) if k > 3 else (0, 1, 400, 257)[k]
        pos, cnt, total = gen_points(rng, n)
        out.append(dict(pos=pos, cnt=cnt, total=total, mode=mode))
    return out


def blob_3000(seed=6):
    """3000 points of a jittered 15 x 15 x 14 grid of spacing 0.07 with 150 of them taken out, so that it has gaps"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(15), np.arange(15), np.arange(14), indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.permutation(len(g))[:3000]]
    return (g * 0.07 + rng.uniform(-0.01, 0.01, (3000, 3))).astype(f32)


def gen_map(rng, n):
    """n objects: boxes around a few sites so that many overlap, few labels, track ids with repeats"""
    sites = rng.uniform(-2, 2, (max(1, n // 3), 3))
    lo = sites[rng.integers(len(sites), size=n)] + rng.uniform(-0.4, 0.4, (n, 3))
    size = rng.uniform(0.3, 1.2, (n, 3))
    size[rng.random(n) < 0.05] = 0.0
    bbox = np.concatenate([lo + size, lo], axis=1).astype(f32)
    label = rng.integers(0, 3, n).astype(np.int32)
    track = np.sort(rng.integers(0, max(1, 2 * n), n)).astype(np.int32)
    return label, track, bbox


def generated_maps(count=200, seed=8):
    rng = np.random.default_rng(seed)
    return [gen_map(rng, int(rng.integers(0, 41)) if k > 2 else (0, 1, 128)[k]) for k in range(count)]


# ------------------------------------------------------------------ the caller program's fixture ------------------------------------------------------------------

def fixture_scene():
    """(points [M, 3], frames): three frames over two overlapping blobs A and B of label 1 that become two objects, a blob C of label 2 and background points.
    A frame is dict(kps = [(point index or -1, outlier)], dets = [dict(label, obj = the track id TrackObject gave or -1, idx = keypoint indices)])."""
    rng = np.random.default_rng(12)

    def grid(nx, ny, nz, o):
        g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
        return (g * 0.07 + rng.uniform(-0.01, 0.01, (len(g), 3)) + np.asarray(o)).astype(f32)
    A, B, Cc = grid(4, 4, 4, [0, 0, 0]), grid(4, 4, 4, [0.05, 0.03, 0.02]), grid(3, 3, 4, [3, 0, 0])
    bg = (rng.uniform(-2, 2, (8, 3)) + [0, 5, 0]).astype(f32)
    points = np.concatenate([A, B, Cc, bg])
    a, b, c, g = 0, 64, 128, 164   # first indices
    frames = []

    def frame(kps, dets):
        index = {}
        for i, (p, _) in enumerate(kps):
            index.setdefault(p, i)
        frames.append(dict(kps=kps, dets=[dict(label=l, obj=o, idx=[index[p] for p in ps] + extra) for l, o, ps, extra in dets]))
    r = lambda lo, hi: list(range(lo, hi))
    # frame 0: A's first 40 points with two background points (dropped as small clusters) become object 0; 30 points of C, one cluster: the shortcut, object 1;
    # ten points of B are seen outside every detection: label -1
    kps = [(p, 0) for p in r(a, a + 40) + [g, g + 1] + r(c, c + 30) + r(b, b + 10)] + [(-1, 0), (-1, 0)]
    frame(kps, [(1, -1, r(a, a + 40) + [g, g + 1], [len(kps) - 1]), (2, -1, r(c, c + 30), [])])
    # frame 1: object 0 is updated (a background point is flagged as the frame's outlier); B[5:60] become object 2; B[0:5] are background again; four points of C: no object
    kps = [(p, 0) for p in r(a + 20, a + 64)] + [(g + 2, 1)] + [(p, 0) for p in r(b, b + 60) + r(c + 30, c + 34)]
    frame(kps, [(1, 0, r(a + 20, a + 64) + [g + 2], []), (1, -1, r(b + 5, b + 60), []), (2, -1, r(c + 30, c + 34), [])])
    # frame 2: both updated; B[0:5] carry label 1 once in three sightings: bad; a background point with label 1 is a far one-point cluster
    kps = [(p, 0) for p in r(a, a + 64) + r(b, b + 64) + [g + 3]]
    frame(kps, [(1, 0, r(a, a + 64), []), (1, 2, r(b, b + 64) + [g + 3], [])])
    return points, frames


def write_fixture(path, points, frames):
    with open(path, "w") as f:
        f.write("n_points %d\n" % len(points))
        for p in points:
            f.write(" ".join(float(v).hex() for v in p) + "\n")
        f.write("n_frames %d\n" % len(frames))
        for F in frames:
            f.write("frame %d %d\n" % (len(F["kps"]), len(F["dets"])))
            for p, o in F["kps"]:
                f.write("%d %d\n" % (p, o))
            for d in F["dets"]:
                f.write("%d %d %d %s\n" % (d["label"], d["obj"], len(d["idx"]), " ".join(str(i) for i in d["idx"])))


def run_fixture(points, frames):
    """the lines tests/adapter_object_map_program.cc prints, from the restatement"""
    label_cnt = [dict() for _ in points]
    objects, lines = {}, []
    hx = lambda v: " ".join("%08x" % int(x) for x in np.asarray(v, f32).reshape(-1).view(np.uint32))

    def counts(mps, label):
        return [label_cnt[p].get(label, 0) for p in mps], [sum(label_cnt[p].values()) for p in mps]

    def extent(o):
        center, bbox = center_and_size(points[o["mps"]])
        if center is not None:
            o["center"], o["bbox"] = center, bbox

    def reject(o):
        if not o["mps"]:
            return
        cnt, total = counts(o["mps"], o["label"])
        keep = reject_outliers(points[o["mps"]], cnt, total, MODE_UPDATE)["keep"]
        o["mps"] = [p for p, k in zip(o["mps"], keep) if k]
    for k, F in enumerate(frames):
        det_of = {}
        for j, d in enumerate(F["dets"]):
            for i in d["idx"]:
                det_of[i] = j
        for i, (p, _) in enumerate(F["kps"]):
            if p >= 0:
                lab = F["dets"][det_of[i]]["label"] if i in det_of else -1
                label_cnt[p][lab] = label_cnt[p].get(lab, 0) + 1
        for d in F["dets"]:
            if d["obj"] >= 0:
                o = objects[d["obj"]]
                o["updates"] += 1
                new = [F["kps"][i][0] for i in d["idx"] if F["kps"][i][0] >= 0 and not F["kps"][i][1] and F["kps"][i][0] not in o["mps"]]
                o["mps"] = o["mps"] + new
                reject(o)
                extent(o)
                o["obs"] += 1
                if o["updates"] > 5 and len(o["mps"]) < 5:
                    o["valid"] = 0
                continue
            cand = [F["kps"][i][0] for i in d["idx"] if F["kps"][i][0] >= 0]
            if not cand:
                continue
            r = reject_outliers(points[cand], mode=MODE_NEW_OBJECT)
            cand = [p for p, kk in zip(cand, r["keep"]) if kk]
            if r["path"] == PATH_SHORTCUT or len(cand) > 5:
                o = dict(track=len(objects), label=d["label"], updates=0, valid=1, replaced=-1, obs=1, mps=cand, center=np.zeros(3, f32), bbox=np.zeros(6, f32))
                extent(o)
                objects[o["track"]] = o
        lines.append("frame %d:" % k + "".join(" %d:%d" % (t, len(o["mps"])) for t, o in sorted(objects.items())))
    order = sorted(objects)
    _, sets = merge_sets([objects[t]["label"] for t in order], [objects[t]["track"] for t in order], np.array([objects[t]["bbox"] for t in order], f32).reshape(-1, 6))
    gone = set()
    for mem, best in sets:
        tgt = objects[order[best]]
        old = len(tgt["mps"])
        tgt["mps"] = [p for i in mem for p in objects[order[i]]["mps"]]
        tgt["obs"] = sum(objects[order[i]]["obs"] for i in mem)
        if abs(len(tgt["mps"]) - old) > 50:
            reject(tgt)
        extent(tgt)
        tgt["updates"] += 1
        for i in mem:
            if i != best:
                objects[order[i]]["replaced"] = tgt["track"]
                gone.add(order[i])
    lines.append("erased %d left %d" % (len(gone), len(objects) - len(gone)))
    for t in order:
        o = objects[t]
        lines.append("object %d label %d updates %d valid %d replaced %d obs %d n %d center %s bbox %s ids%s" % (o["track"], o["label"], o["updates"], o["valid"], o["replaced"], o["obs"],
                     len(o["mps"]), hx(o["center"]), hx(o["bbox"]), "".join(" %d" % p for p in o["mps"])))
    return lines
