"""Shared pieces of the GPU parity tests: the input generators of the single-frame tests (moved here unchanged, same arrays from the same
seeds) and the helpers of the batched-entry-point tests (tests/test_batch_entry_points_gpu.py, tests/test_batch_frame_mappoint_gpu.py): the
heterogeneous batch shape, device memory as torch tensors, a side stream, reads of handle-owned device arrays."""
import ctypes as C

import numpy as np

from object_slam_amd import KP_DTYPE, QUERY_DTYPE

SCALE = np.array([1.2 ** i for i in range(8)], np.float32)

# ---- tests/test_matcher_gpu.py ----


def rand_frame(rng, N, w=640, h=480, clustered=False):
    k = np.zeros(N, KP_DTYPE)
    if clustered:   # few distinct positions: many queries compete for the same keypoints
        cx = rng.uniform(50, w - 50, 12)
        cy = rng.uniform(50, h - 50, 12)
        sel = rng.integers(0, 12, N)
        k["x"] = (cx[sel] + rng.normal(0, 4, N)).astype(np.float32)
        k["y"] = (cy[sel] + rng.normal(0, 4, N)).astype(np.float32)
    else:
        k["x"] = rng.uniform(-5, w + 5, N).astype(np.float32)   # a few outside the grid on purpose
        k["y"] = rng.uniform(-5, h + 5, N).astype(np.float32)
    k["octave"] = rng.integers(0, 8, N)
    k["angle"] = rng.uniform(0, 360, N).astype(np.float32)
    desc = rng.integers(0, 256, (N, 32)).astype(np.uint8)
    uR = np.where(rng.random(N) < 0.7, k["x"] - rng.uniform(1, 40, N), -1).astype(np.float32)
    return k, uR, desc


def rand_queries(rng, k, uR, desc, M, noise_bits, p_block=0.8, few_desc=False):
    q = np.zeros(M, QUERY_DTYPE)
    src = rng.integers(0, len(k), M)
    q["u"] = k["x"][src] + rng.normal(0, 3, M)
    q["v"] = k["y"][src] + rng.normal(0, 3, M)
    q["ur"] = q["u"] - (k["x"][src] - uR[src]) + rng.normal(0, 2, M)
    lvl = np.clip(k["octave"][src] + rng.integers(-1, 2, M), 0, 7)
    q["radius"] = (rng.choice([2.5, 4.0], M) * rng.choice([1, 3, 7], M) * SCALE[lvl]).astype(np.float32)
    q["minLevel"] = lvl - 1
    q["maxLevel"] = lvl
    q["flags"] = (rng.random(M) < 0.95).astype(np.int32) | ((rng.random(M) < p_block).astype(np.int32) << 1)
    q["angle"] = (k["angle"][src] + rng.normal(0, 20, M)) % 360
    d = desc[src].copy()
    if few_desc:   # force Hamming ties: only a handful of distinct descriptors
        d = desc[src % 5].copy()
    flip = rng.random((M, 256)) < noise_bits
    d ^= np.packbits(flip, axis=1, bitorder="little")
    q["desc"] = d
    return q


def bow_pair(rng, N1, N2, n_nodes):
    k1, uR1, d1 = rand_frame(rng, N1)
    src = rng.integers(0, N1, N2)
    k2 = np.zeros(N2, KP_DTYPE)
    k2["x"] = k1["x"][src] - rng.uniform(2, 30, N2)
    k2["y"] = k1["y"][src] + rng.normal(0, 1.0, N2)
    k2["octave"] = np.clip(k1["octave"][src] + rng.integers(-1, 2, N2), 0, 7)
    k2["angle"] = (k1["angle"][src] + rng.normal(0, 8, N2)) % 360
    d2 = d1[src].copy()
    d2 ^= np.packbits(rng.random((N2, 256)) < 0.06, axis=1, bitorder="little")
    node1 = rng.integers(0, n_nodes, N1).astype(np.uint32)
    node2 = node1[src].copy()
    wrong = rng.random(N2) < 0.15
    node2[wrong] = rng.integers(0, n_nodes, wrong.sum())
    uR2 = np.where(rng.random(N2) < 0.6, k2["x"] - rng.uniform(1, 30, N2), -1).astype(np.float32)
    return k1, uR1, d1, node1, k2, uR2, d2, node2


# ---- tests/test_mappoint_gpu.py ----


def desc_lists(rng, P, nmax):
    base = rng.integers(0, 256, (P, 32), dtype=np.uint8)
    out = []
    for p in range(P):
        n = int(rng.integers(0, nmax + 1)) if p % 7 else (0 if p % 14 == 0 else nmax)
        d = np.repeat(base[p][None], n, 0)
        flips = rng.random((n, 256)) < 0.08          # noisy views of one descriptor: many ties in the medians
        d = np.bitwise_xor(d, np.packbits(flips, axis=1))
        out.append(d)
    return out


# ---- tests/test_triangulate_gpu.py ----

SF = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
LS2 = (SF * SF).astype(np.float32)


def tri_pose(rng, t_scale):
    a = rng.normal(0, 0.08, 3)
    th = np.linalg.norm(a)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    Tcw = np.eye(4, dtype=np.float32)
    Tcw[:3, :3] = R
    Tcw[:3, 3] = rng.normal(0, t_scale, 3)
    Twc = np.eye(4, dtype=np.float32)
    Twc[:3, :3] = Tcw[:3, :3].T
    Twc[:3, 3] = -(Tcw[:3, :3].T @ Tcw[:3, 3])
    return Tcw, Twc


def tri_make_kf(rng, X, Tcw, cam, stereo_frac, noise):
    fx, fy, cx, cy, bf = cam
    Pc = X @ Tcw[:3, :3].T.astype(np.float64) + Tcw[:3, 3]
    z = Pc[:, 2]
    N = len(X)
    k = np.zeros(N, KP_DTYPE)
    octv = rng.integers(0, 8, N)
    sig = np.sqrt(LS2[octv])
    k["x"] = fx * Pc[:, 0] / z + cx + rng.normal(0, noise, N) * sig
    k["y"] = fy * Pc[:, 1] / z + cy + rng.normal(0, noise, N) * sig
    k["octave"] = octv
    k["size"] = 31 * SF[octv]
    st = (rng.random(N) < stereo_frac) & (z > 0.1)
    depth = np.where(st, z * (1 + rng.normal(0, 0.01, N)), -1).astype(np.float32)
    ur = np.where(st, k["x"] - bf / np.maximum(depth, 1e-3), -1).astype(np.float32)
    raw = k.copy()
    raw["x"] += 0.3   # mvKeys differs from mvKeysUn (distortion); only UnprojectStereo reads it
    return k, raw, ur, depth


# ---- tests/test_frame_gpu.py ----

TUM1_K = (517.306408, 516.469215, 318.643040, 255.313989)                      # reference Examples/RGB-D/TUM1.yaml:8-11
TUM1_D = (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)                  # k1, k2, p1, p2, k3 (:13-17)


def frame_keys(rng, n, w, h):
    k = np.zeros(n, KP_DTYPE)
    k["x"] = rng.uniform(0, w - 1, n).astype(np.float32)
    k["y"] = rng.uniform(0, h - 1, n).astype(np.float32)
    k["octave"] = rng.integers(0, 8, n)
    k["angle"] = rng.uniform(0, 360, n)
    k["size"] = 31
    k["response"] = rng.integers(7, 200, n)
    k["class_id"] = -1
    return k


# ---- the batch every batched-entry-point test uses ----

B = 5


def batch_counts(stride):
    """Counts per element of the heterogeneous batch: full, small, empty, one, about half — the empty and the full element between the others."""
    return np.array([stride, 17, 0, 1, stride // 2], np.int32)


REV = np.arange(B)[::-1].copy()   # the batch order of the independence check


def dev(a):
    """Host array (structured dtypes as bytes) -> device tensor."""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        a = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    return torch.from_numpy(a.copy()).cuda()


def host(t, dtype=None, shape=None):
    """Device tensor -> host array, optionally reinterpreted as a (structured) dtype."""
    a = t.cpu().numpy()
    if dtype is not None:
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1).view(dtype)
        if shape is not None:
            a = a.reshape(shape)
    return a


def vp(t, offset_bytes=0):
    return C.c_void_p(t.data_ptr() + offset_bytes) if t is not None else None


def side_stream():
    """A non-default stream.  Inputs are uploaded on the default stream: synchronise before the first launch on it."""
    import torch
    torch.cuda.synchronize()
    return torch.cuda.Stream()


def fetch(L, d_ptr, count, dtype):
    """Synchronous read of a handle-owned device array (oslam_*_results_device pointers)."""
    out = np.zeros(count, dtype)
    if count:
        rc = L.oslam_memcpy_from_device(C.c_void_p(out.ctypes.data), d_ptr, C.c_size_t(out.nbytes))
        assert rc == 0, L.oslam_last_error()
    return out


# ---- the windowed matcher on device memory (oslam_match_*_batch_device) ----


def upload_frames(els):
    """els[b] = dict(k, uR, desc, blocked, q, nk, nq) with rows of equal length -> the [batch][stride] device arrays of a search."""
    st = lambda f: np.stack([e[f] for e in els])
    return dict(k=dev(st("k")), uR=dev(st("uR")), desc=dev(st("desc")), blocked=dev(st("blocked")), q=dev(st("q")),
                nk=dev(np.array([e["nk"] for e in els], np.int32)), nq=dev(np.array([e["nq"] for e in els], np.int32)))


def match_frames(D, row0, kp_stride, bounds, nk_const=None):
    """oslam_match_frames_t over the rows row0.. of upload_frames(); the counts from the device array, or one constant."""
    from object_slam_amd.matcher import MatchFrames
    f = MatchFrames()
    f.keysUn, f.kp_stride = D["k"].data_ptr() + row0 * kp_stride * KP_DTYPE.itemsize, kp_stride
    f.uRight, f.desc, f.blocked = D["uR"].data_ptr() + row0 * kp_stride * 4, D["desc"].data_ptr() + row0 * kp_stride * 32, D["blocked"].data_ptr() + row0 * kp_stride
    if nk_const is None:
        f.n_kps, f.n_kps_const = D["nk"].data_ptr() + row0 * 4, -1
    else:
        f.n_kps, f.n_kps_const = None, nk_const
    f.minX, f.minY, f.maxX, f.maxY = [float(v) for v in bounds]
    return f


def match_results(L, h, batch, q_stride, kp_stride):
    """Everything through oslam_match_results_device, with the strides of the search: kp_match is [batch][kp_stride], also for kp_stride < max_keypoints."""
    p = [C.c_void_p() for _ in range(6)]
    rc = L.oslam_match_results_device(h, *[C.byref(x) for x in p])
    assert rc == 0, L.oslam_last_error()
    return dict(qm=fetch(L, p[0], batch * q_stride, np.int32).reshape(batch, q_stride), qd=fetch(L, p[1], batch * q_stride, np.int32).reshape(batch, q_stride),
                km=fetch(L, p[2], batch * kp_stride, np.int32).reshape(batch, kp_stride), nm=fetch(L, p[3], batch, np.int32), d_queries=p[4], d_nq=p[5])
