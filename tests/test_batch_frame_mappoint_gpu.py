"""GPU parity of the batched device entry points whose OUTPUT arrays belong to the caller: Frame::ComputeStereoFromRGBD in its three batch forms, the
gather / copy helpers of the resident keyframe store, Frame::isInFrustum for a batch of frames (feeding the matcher, as the driver does), the MapPoint
device forms and the batched triangulation.  Same batch as tests/test_batch_entry_points_gpu.py (counts {stride, 17, 0, 1, stride / 2} from a device
array, a side stream) and the same three assertions; the third one here: every output is prefilled with a sentinel (0xFF bytes, NaN) and nothing
outside [b][0 : count_b] changes, except where include/oslam_hip.h defines a value there."""
import ctypes as C

import numpy as np
import pytest

from batch_common import (B, LS2, REV, SCALE, SF, batch_counts, desc_lists, dev, frame_keys, host, match_frames, match_results, rand_frame, side_stream, tri_make_kf,
                          tri_pose, upload_frames, vp)
from object_slam_amd import KP_DTYPE, QUERY_DTYPE, synth
from object_slam_amd._lib import check, lib

pytestmark = pytest.mark.gpu

KS, QS = 640, 1024
NAN32 = np.float32(np.nan).view(np.uint32)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _all_sentinel(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


# --------------------------------------------------------------------------------------------------------------------------------------------
# Frame::ComputeStereoFromRGBD, three batch forms
# --------------------------------------------------------------------------------------------------------------------------------------------

DW, DH, DPITCH = 320, 240, 336                  # pitch > cols
DSTRIDE = DH * DPITCH + 64                      # floats between the images of the contiguous form
MBF = 40.0
DEPTH_FACTOR = np.float32(1.0 / 5000.0)         # TUM: (float)d16 * factor is not exactly representable


def _rgbd_elements():
    rng = np.random.default_rng(91)
    n = batch_counts(KS)
    els = []
    for b in range(B):
        keys = frame_keys(rng, KS, DW, DH)
        un = keys.copy()
        un["x"] = (keys["x"] + rng.normal(0, 1.5, KS)).astype(np.float32)
        d16 = rng.integers(300, 40000, (DH, DPITCH)).astype(np.uint16)
        d16[rng.random((DH, DPITCH)) < 0.2] = 0                                            # invalid depth
        depth = (d16.astype(np.float32) * DEPTH_FACTOR).astype(np.float32)                # one float multiplication, as cvtScale does
        depthf = depth.copy()
        depthf[rng.random((DH, DPITCH)) < 0.05] = -1.0
        depthf[:, DW:] = 777.0                                                             # the padding between cols and pitch: skipped, never read
        els.append(dict(keys=keys, un=un, d16=d16, depth16f=depth, depthf=depthf, n=int(n[b])))
    return els


def test_stereo_from_rgbd_batch_forms(oracle):
    import torch
    L = lib()
    els = _rgbd_elements()
    assert float(np.float32(12345) * DEPTH_FACTOR) != 12345 / 5000.0                       # the scaled depth rounds: float arithmetic matters
    stream = side_stream()
    s = C.c_void_p(stream.cuda_stream)
    perm = np.array([3, 0, 4, 1, 2])                                                       # image b lives in slot perm[b]: a shuffled pointer table

    def up(order):
        e = [els[b] for b in order]
        D = dict(keys=dev(np.stack([x["keys"] for x in e])), un=dev(np.stack([x["un"] for x in e])), n=dev(np.array([x["n"] for x in e], np.int32)))
        cont = np.full((B, DSTRIDE), 555.0, np.float32)
        slots = np.full((B, DSTRIDE), 555.0, np.float32)
        slots16 = np.full((B, DH * DPITCH + 8), 7, np.uint16)
        for i, x in enumerate(e):
            cont[i, :DH * DPITCH] = x["depthf"].reshape(-1)
            slots[perm[i], :DH * DPITCH] = x["depthf"].reshape(-1)
            slots16[perm[i], :DH * DPITCH] = x["d16"].reshape(-1)
        D["cont"], D["slots"], D["slots16"] = dev(cont), dev(slots), dev(slots16.view(np.int16))
        D["ptrs"] = dev(np.array([D["slots"].data_ptr() + int(perm[i]) * DSTRIDE * 4 for i in range(B)], np.int64))
        D["ptrs16"] = dev(np.array([D["slots16"].data_ptr() + int(perm[i]) * (DH * DPITCH + 8) * 2 for i in range(B)], np.int64))
        return D

    def run(form, D, row0, batch, n_const=None):
        uR = torch.full((batch + 2, KS), float("nan"), dtype=torch.float32, device="cuda")  # a guard row before and behind the block
        dp = torch.full((batch + 2, KS), float("nan"), dtype=torch.float32, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        head = (vp(D["keys"], row0 * KS * 28), vp(D["un"], row0 * KS * 28), vp(D["n"], row0 * 4) if n_const is None else None, n_const or 0, KS, batch)
        tail = (C.c_float(MBF), vp(uR, KS * 4), vp(dp, KS * 4), vp(status), s)
        if form == "cont":
            check(L.oslam_frame_stereo_from_rgbd_batch_device(*head, vp(D["cont"], row0 * DSTRIDE * 4), DH, DW, DPITCH, C.c_size_t(DSTRIDE), *tail))
        elif form == "ptrs":
            check(L.oslam_frame_stereo_from_rgbd_batch_ptrs_device(*head, vp(D["ptrs"], row0 * 8), DH, DW, DPITCH, *tail))
        else:
            check(L.oslam_frame_stereo_from_rgbd_batch_ptrs_u16_device(*head, vp(D["ptrs16"], row0 * 8), DH, DW, DPITCH, C.c_float(float(DEPTH_FACTOR)), *tail))
        stream.synchronize()
        uR, dp = uR.cpu().numpy(), dp.cpu().numpy()
        assert int(status.cpu()[0]) == 0                                                   # valid input
        for a in (uR, dp):
            assert (_u32(a[0]) == NAN32).all() and (_u32(a[-1]) == NAN32).all()            # nothing before or behind [batch][stride]
        return uR[1:-1], dp[1:-1]

    D, Drev = up(range(B)), up(REV)
    for form in ("cont", "ptrs", "u16"):
        uR, dp = run(form, D, 0, B)
        ruR, rdp = run(form, Drev, 0, B)
        for b, e in enumerate(els):
            n = e["n"]
            depth = e["depth16f"] if form == "u16" else e["depthf"]
            our, odp = oracle.stereo_from_rgbd(e["keys"][:n], e["un"][:n], depth, MBF)
            assert np.array_equal(_u32(uR[b, :n]), _u32(our)) and np.array_equal(_u32(dp[b, :n]), _u32(odp)), (form, b)
            assert (uR[b, n:] == -1).all() and (dp[b, n:] == -1).all()                     # the header: -1 in the slots beyond the count
            r = int(np.where(REV == b)[0][0])
            assert np.array_equal(_u32(ruR[r]), _u32(uR[b])) and np.array_equal(_u32(rdp[r]), _u32(dp[b])), (form, b)
            auR, adp = run(form, D, b, 1)
            assert np.array_equal(_u32(auR[0]), _u32(uR[b])) and np.array_equal(_u32(adp[0]), _u32(dp[b])), (form, b)
        assert 0.1 < (dp[0] < 0).mean() < 0.4 and (dp[0] > 0).sum() > 300
        c17 = dict(D, n=dev(np.full(B, 17, np.int32)))
        a, c = run(form, c17, 0, B), run(form, D, 0, B, n_const=17)
        assert np.array_equal(_u32(a[0]), _u32(c[0])) and np.array_equal(_u32(a[1]), _u32(c[1]))


# --------------------------------------------------------------------------------------------------------------------------------------------
# gather / copy helpers: byte equality against numpy
# --------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,row_bytes,src_pitch,dst_pitch,skew", [(37, 101, 117, 128, 3), (24, 320, 336, 320, 0), (9, 50, 50, 64, 16)])
def test_gather_images_device(rows, row_bytes, src_pitch, dst_pitch, skew):
    """src_pitch != dst_pitch; rows that are 16-byte aligned on both sides (vector chunks + byte tail) and rows that are not (bytes only)."""
    import torch
    L = lib()
    rng = np.random.default_rng(rows)
    n = B
    slot = rows * src_pitch + 48
    src = rng.integers(0, 255, n * slot + 64, dtype=np.uint8)
    off = [int(p) * slot + (i % 2) * skew for i, p in enumerate(rng.permutation(n))]      # a shuffled table; every other image skewed off alignment
    dst_image_stride = rows * dst_pitch + 32
    d_src = dev(src)
    stream = side_stream()
    for order in (list(range(n)), list(range(n))[::-1]):
        d_dst = torch.full((n * dst_image_stride + 16,), 0xFF, dtype=torch.uint8, device="cuda")
        tab = dev(np.array([d_src.data_ptr() + off[i] for i in order], np.int64))
        torch.cuda.synchronize()
        check(L.oslam_frame_gather_images_device(vp(tab), n, src_pitch, row_bytes, rows, vp(d_dst), C.c_size_t(dst_image_stride), dst_pitch, C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        want = np.full(n * dst_image_stride + 16, 0xFF, np.uint8)
        for j, i in enumerate(order):
            for r in range(rows):
                want[j * dst_image_stride + r * dst_pitch: j * dst_image_stride + r * dst_pitch + row_bytes] = src[off[i] + r * src_pitch: off[i] + r * src_pitch + row_bytes]
        assert np.array_equal(d_dst.cpu().numpy(), want)                                   # the copied bytes, and 0xFF everywhere else
        assert (want != 0xFF).sum() > n * rows * row_bytes * 0.9


def test_copy_segments_device():
    """Byte counts that are no multiple of 4 (and 0), unaligned offsets, and segments aligned on both sides (16-byte chunks + tail)."""
    import torch
    L = lib()
    rng = np.random.default_rng(17)
    nbytes = [KS * 28, 17, 0, 1, 4099, 333, 4096, 15]
    src_off = [21000, 1003, 2000, 2001, 4112, 9001, 16384, 20481]                          # 4112 and 16384 are multiples of 16
    src = rng.integers(0, 255, 40000, dtype=np.uint8)
    dst_off, at = [], 5
    for i, nb in enumerate(nbytes):
        at = (at + 15) // 16 * 16 if i in (4, 6) else at | 1                               # segments 4 and 6 aligned on both sides, the others odd
        dst_off.append(at)
        at += nb + 7
    d_src = dev(src)
    stream = side_stream()
    for order in (list(range(len(nbytes))), list(range(len(nbytes)))[::-1]):
        d_dst = torch.full((at + 64,), 0xFF, dtype=torch.uint8, device="cuda")
        assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
        segs = np.zeros(len(nbytes), np.dtype([("src", "<u8"), ("dst", "<u8"), ("bytes", "<u4"), ("pad", "<u4")]))
        for j, i in enumerate(order):
            segs[j] = (d_src.data_ptr() + src_off[i], d_dst.data_ptr() + dst_off[i], nbytes[i], 0)
        d_segs = dev(segs)
        torch.cuda.synchronize()
        check(L.oslam_copy_segments_device(vp(d_segs), len(nbytes), C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        want = np.full(at + 64, 0xFF, np.uint8)
        for i, nb in enumerate(nbytes):
            want[dst_off[i]:dst_off[i] + nb] = src[src_off[i]:src_off[i] + nb]
        assert np.array_equal(d_dst.cpu().numpy(), want)
    assert (src_off[4] % 16, dst_off[4] % 16, src_off[6] % 16, dst_off[6] % 16) == (0, 0, 0, 0) and src_off[1] % 2 == 1 and dst_off[1] % 2 == 1


def test_gather_descriptors_device():
    import torch
    L = lib()
    rng = np.random.default_rng(23)
    counts = batch_counts(KS)
    arrays = [rng.integers(0, 256, (max(int(c), 1), 32), dtype=np.uint8) for c in counts]
    d_arrays = [dev(a) for a in arrays]
    n = 1003                                                                               # 32 descriptors per workgroup: a partial last one
    which = rng.choice([0, 1, 3, 4], n)                                                    # the empty array has nothing to gather
    rec = np.stack([which, [int(rng.integers(0, counts[w])) for w in which]], 1).astype(np.int32)
    tab = dev(np.array([a.data_ptr() for a in d_arrays], np.int64))
    d_rec = dev(rec)
    out = torch.full((n + 4, 32), 0xFF, dtype=torch.uint8, device="cuda")
    stream = side_stream()
    check(L.oslam_gather_descriptors_device(vp(tab), vp(d_rec), n, vp(out), C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    got = out.cpu().numpy()
    want = np.stack([arrays[w][k] for w, k in rec])
    assert np.array_equal(got[:n], want) and _all_sentinel(got[n:])
    assert set(which.tolist()) == {0, 1, 3, 4} and (rec[which == 0, 1] > 600).any()


# --------------------------------------------------------------------------------------------------------------------------------------------
# Frame::isInFrustum for a batch of frames -> SearchByProjection of the same batch
# --------------------------------------------------------------------------------------------------------------------------------------------

SIN = 1200           # stride of the resident point table; the queries use QS < SIN
K5 = np.asarray(synth.TUM_K, np.float32)
PLAIN = (0.0, 0.0, 640.0, 480.0)
LOGSF = np.float32(np.log(np.float32(1.2)))
TH = (1.0, 3.0, 1.0, 5.0, 3.0)


def _frustum_elements():
    """Frames as in the matcher tests and, per frame, map points that project near its keypoints from the frame's own pose."""
    rng = np.random.default_rng(515)
    nk, M = batch_counts(KS), batch_counts(QS)
    fx, fy, cx, cy = [float(v) for v in K5[:4]]
    els = []
    for b in range(B):
        k, uR, desc = rand_frame(rng, KS)
        n = max(int(nk[b]), 1)
        src = rng.integers(0, n, SIN)
        Tcw = synth.make_T(rng.normal(0, 0.08, 3), rng.normal(0, 0.3, 3)).astype(np.float32)
        z = rng.uniform(0.8, 6.0, SIN)
        u = k["x"][src] + rng.normal(0, 3, SIN)
        v = k["y"][src] + rng.normal(0, 3, SIN)
        u[::11] += rng.choice([-700, 700], len(u[::11]))                                   # outside the image
        Xc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
        Xc[::29, 2] *= -1                                                                  # behind the camera
        R, t = Tcw[:3, :3].astype(np.float64), Tcw[:3, 3].astype(np.float64)
        Pw = ((Xc - t) @ R).astype(np.float32)
        Ow = -R.T @ t
        dirs = Pw - Ow
        dist = np.linalg.norm(dirs, axis=1)
        Pn = dirs / dist[:, None] + rng.normal(0, 0.5, (SIN, 3))
        Pn = (Pn / np.linalg.norm(Pn, axis=1)[:, None]).astype(np.float32)
        # most points predict the level of the keypoint they came from (ceil(log(maxD / dist) / log 1.2) == octave), the rest any level or none
        ratio = np.where(rng.random(SIN) < 0.7, 1.2 ** (k["octave"][src] - rng.uniform(0.05, 0.95, SIN)), rng.uniform(0.6, 5.0, SIN))
        maxD = (dist * ratio).astype(np.float32)
        minD = (maxD / SCALE[-1]).astype(np.float32)
        mp_desc = desc[src] ^ np.packbits(rng.random((SIN, 256)) < 0.06, axis=1, bitorder="little")
        els.append(dict(k=k, uR=uR, desc=desc, blocked=(rng.random(KS) < 0.1).astype(np.uint8), q=np.zeros(QS, QUERY_DTYPE), nk=int(nk[b]), nq=int(M[b]), Tcw=Tcw, Pw=Pw, Pn=Pn,
                        maxD=maxD, minD=minD, obs=(rng.random(SIN) < 0.9).astype(np.uint8), mp_desc=mp_desc, skip=(rng.random(QS) < 0.1).astype(np.uint8), th=np.float32(TH[b])))
    return els


def _frustum_ref(oracle, e, M):
    return oracle.is_in_frustum(e["Pw"][:M], e["Pn"][:M], e["maxD"][:M], e["minD"][:M], e["obs"][:M], e["mp_desc"][:M], e["Tcw"], K5, PLAIN, 0.5, LOGSF, SCALE, float(e["th"]))


def test_is_in_frustum_batch_forms_feed_the_matcher(oracle):
    """oslam_frame_is_in_frustum_batch_resident_device (stride_out < stride_in, skip flags, a pose and a radius factor per element), its plain batch form
    and the single-frame device form on the same points; the queries of the resident form then go straight into oslam_match_search_batch_device."""
    import torch
    L = lib()
    els = _frustum_elements()
    stream = side_stream()
    s = C.c_void_p(stream.cuda_stream)
    sf = np.ascontiguousarray(SCALE)
    bnd = (C.c_float * 4)(*PLAIN)
    k5 = (C.c_float * 5)(*[float(v) for v in K5])
    m = C.c_void_p()
    check(L.oslam_matcher_create(C.byref(m), B, 2400, 4096, 0))
    inactive = np.zeros(1, QUERY_DTYPE)
    inactive["minLevel"] = inactive["maxLevel"] = -1

    def up(order):
        e = [els[b] for b in order]
        st = lambda f, dt: dev(np.stack([x[f] for x in e]).astype(dt))
        D = upload_frames(e)
        D.update(Pw=st("Pw", np.float32), Pn=st("Pn", np.float32), maxD=st("maxD", np.float32), minD=st("minD", np.float32), obs=st("obs", np.uint8), mp_desc=st("mp_desc", np.uint8),
                 skip=st("skip", np.uint8), Tcw=st("Tcw", np.float32), th=st("th", np.float32))
        return D

    def run(D, row0, batch, resident=True):
        so = QS if resident else SIN
        out = torch.full((batch + 2, so, 64), 0xFF, dtype=torch.uint8, device="cuda")
        inv = torch.full((batch + 2, so), 0xFF, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        pts = (vp(D["Pw"], row0 * SIN * 12), vp(D["Pn"], row0 * SIN * 12), vp(D["maxD"], row0 * SIN * 4), vp(D["minD"], row0 * SIN * 4), vp(D["obs"], row0 * SIN), vp(D["mp_desc"], row0 * SIN * 32))
        tail = (vp(D["Tcw"], row0 * 64), vp(D["th"], row0 * 4), k5, bnd, C.c_float(0.5), C.c_float(float(LOGSF)), C.c_void_p(sf.ctypes.data), 8, vp(out, so * 64), vp(inv, so), s)
        if resident:
            check(L.oslam_frame_is_in_frustum_batch_resident_device(batch, SIN, QS, vp(D["nq"], row0 * 4), *pts, vp(D["skip"], row0 * QS), *tail))
        else:
            check(L.oslam_frame_is_in_frustum_batch_device(batch, SIN, vp(D["nq"], row0 * 4), *pts, *tail))
        res = None
        if resident:    # the driver's next step: the queries, where they are, with the same counts
            f = match_frames(D, row0, KS, PLAIN)
            check(L.oslam_match_search_batch_device(m, C.byref(f), vp(out, so * 64), QS, vp(D["nq"], row0 * 4), 0, batch, C.c_float(0.8), 1, 0, 100, s))
            stream.synchronize()
            res = match_results(L, m, batch, QS, KS)
        stream.synchronize()
        q = host(out, QUERY_DTYPE, (batch + 2, so))
        iv = inv.cpu().numpy()
        assert _all_sentinel(q[0]) and _all_sentinel(q[-1]) and _all_sentinel(iv[0]) and _all_sentinel(iv[-1])
        return q[1:-1], iv[1:-1], res

    D, Drev = up(range(B)), up(REV)
    q, iv, res = run(D, 0, B)
    rq, riv, rres = run(Drev, 0, B)
    pq, piv, _ = run(D, 0, B, resident=False)
    seen, onms = 0, []
    for b, e in enumerate(els):
        M, nk = e["nq"], e["nk"]
        ref = _frustum_ref(oracle, e, M)
        want = ref.copy()
        sk = e["skip"][:M] != 0
        want[sk] = inactive[0]                                                             # a skipped point: an inactive query, in_view 0
        assert np.array_equal(q[b, :M].view(np.uint8), want.view(np.uint8)), b
        assert np.array_equal(iv[b, :M], (want["flags"] & 1).astype(np.uint8)), b
        assert _all_sentinel(q[b, M:]) and _all_sentinel(iv[b, M:])                        # the header: entries beyond d_M[b] are left untouched
        assert np.array_equal(pq[b, :M].view(np.uint8), ref.view(np.uint8)) and np.array_equal(piv[b, :M], (ref["flags"] & 1).astype(np.uint8)), b   # the plain batch form: no skip
        assert _all_sentinel(pq[b, M:]) and _all_sentinel(piv[b, M:])
        seen += int((want["flags"] & 1).sum())
        if M > 20:
            assert sk.any() and (ref["flags"][sk] & 1).any()                               # a skip flag really suppressed a visible point
            assert 0.2 * M < int((ref["flags"] & 1).sum()) < 0.95 * M
        # the matcher on these queries
        onm, oqm, oqd, okm = oracle.search_by_projection(e["k"][:nk], e["uR"][:nk], e["desc"][:nk], e["blocked"][:nk], PLAIN, want, 0.8, True, False)
        onms.append(onm)
        assert np.array_equal(res["qm"][b, :M], oqm) and np.array_equal(res["qd"][b, :M], oqd) and np.array_equal(res["km"][b, :nk], okm) and res["nm"][b] == onm, b
        # independence: reversed batch, element alone
        r = int(np.where(REV == b)[0][0])
        aq, aiv, ares = run(D, b, 1)
        for oq_, oiv, ores, row in ((rq, riv, rres, r), (aq, aiv, ares, 0)):
            assert np.array_equal(oq_[row].view(np.uint8), q[b].view(np.uint8)) and np.array_equal(oiv[row], iv[b])
            assert ores["nm"][row] == res["nm"][b] and np.array_equal(ores["qm"][row, :M], res["qm"][b, :M]) and np.array_equal(ores["km"][row, :nk], res["km"][b, :nk])
        # the single-frame device form: the element's points against its pose
        if M:
            one = torch.full((M + 2, 64), 0xFF, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            check(L.oslam_frame_is_in_frustum_device(M, vp(D["Pw"], b * SIN * 12), vp(D["Pn"], b * SIN * 12), vp(D["maxD"], b * SIN * 4), vp(D["minD"], b * SIN * 4), vp(D["obs"], b * SIN),
                                                     vp(D["mp_desc"], b * SIN * 32), (C.c_float * 16)(*[float(v) for v in e["Tcw"].reshape(-1)]), k5, bnd, C.c_float(0.5), C.c_float(float(LOGSF)),
                                                     C.c_void_p(sf.ctypes.data), 8, C.c_float(float(e["th"])), vp(one, 64), s))
            stream.synchronize()
            o = host(one, QUERY_DTYPE, (M + 2,))
            assert np.array_equal(o[1:-1].view(np.uint8), ref.view(np.uint8)) and _all_sentinel(o[0]) and _all_sentinel(o[-1]), b
    assert seen > 500 and onms[0] > 100 and onms[4] > 50, (seen, onms)                     # the oracle's counts: the matcher had real work on these queries
    L.oslam_matcher_destroy(m)


# --------------------------------------------------------------------------------------------------------------------------------------------
# MapPoint device forms
# --------------------------------------------------------------------------------------------------------------------------------------------

def test_mp_device_forms_match_oracle_and_host_forms(oracle):
    """oslam_mp_distinctive_descriptors_device / oslam_mp_update_normal_depth_device: points with 0, 1 and 2 observations among longer lists, more than
    one workgroup of either kernel, against the oracle and the host-pointer forms."""
    import torch
    from object_slam_amd import MapPointBatch
    L = lib()
    rng = np.random.default_rng(77)
    P, G = 261, 3
    lists = desc_lists(rng, P, 9)
    for p, n in ((1, 1), (2, 2), (3, 130)):
        lists[p] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    nobs = np.array([len(l) for l in lists])
    assert len(lists[0]) == 0 and len(lists[1]) == 1 and len(lists[2]) == 2 and nobs.max() > 128 and (nobs == 0).sum() > 5    # 0, 1, 2 and beyond the LDS chunk
    start = np.concatenate([[0], np.cumsum(nobs)]).astype(np.int32)
    flat = np.concatenate([l for l in lists if len(l)])
    ow_lists = [rng.normal(0, 3, (n, 3)).astype(np.float32) for n in nobs]
    Pos = rng.normal(0, 5, (P, 3)).astype(np.float32)
    OwRef = rng.normal(0, 3, (P, 3)).astype(np.float32)
    lsf = SF[rng.integers(0, 8, P)]
    d = dict(start=dev(start), flat=dev(flat), ow=dev(np.concatenate(ow_lists)), pos=dev(Pos), ref=dev(OwRef), lsf=dev(lsf))
    best = torch.full((P + G,), -1, dtype=torch.int32, device="cuda")                      # 0xFF bytes
    odesc = torch.full((P + G, 32), 0xFF, dtype=torch.uint8, device="cuda")
    o5 = torch.full((P + G, 5), float("nan"), dtype=torch.float32, device="cuda")
    stream = side_stream()
    s = C.c_void_p(stream.cuda_stream)
    check(L.oslam_mp_distinctive_descriptors_device(P, vp(d["start"]), vp(d["flat"]), vp(best), vp(odesc), s))
    check(L.oslam_mp_update_normal_depth_device(P, vp(d["pos"]), vp(d["start"]), vp(d["ow"]), vp(d["ref"]), vp(d["lsf"]), C.c_float(float(SF[-1])), vp(o5), s))
    stream.synchronize()
    best = best.cpu().numpy()
    odesc, o5 = odesc.cpu().numpy(), o5.cpu().numpy()
    mp = MapPointBatch()
    hbest, hdesc = mp.ComputeDistinctiveDescriptors(lists)
    h5 = mp.UpdateNormalAndDepth(Pos, ow_lists, OwRef, lsf, SF[-1])
    for p in range(P):
        ref = oracle.distinctive_descriptor(lists[p])
        assert best[p] == ref == hbest[p], (p, nobs[p], best[p], ref)
        if ref >= 0:
            assert np.array_equal(odesc[p], lists[p][ref]) and np.array_equal(odesc[p], hdesc[p])
        else:
            assert _all_sentinel(odesc[p]) and not hdesc[p].any()                          # the header: the row is left untouched (the host form zero-fills first)
        if nobs[p]:
            r5 = oracle.update_normal_depth(Pos[p], ow_lists[p], OwRef[p], lsf[p], SF[-1])
            assert np.array_equal(_u32(o5[p]), _u32(r5)), p
        else:
            assert not _u32(o5[p]).any()                                                   # the header: five zeros for a point without observations
        assert np.array_equal(_u32(o5[p]), _u32(h5[p])), p
    assert _all_sentinel(best[P:]) and _all_sentinel(odesc[P:]) and (_u32(o5[P:]) == NAN32).all()


# --------------------------------------------------------------------------------------------------------------------------------------------
# triangulation of a batch of (keyframe, neighbour) pairs
# --------------------------------------------------------------------------------------------------------------------------------------------

def test_triangulate_pairs(oracle):
    """oslam_mp_triangulate_pairs: every pair has its OWN current keyframe (pose, keypoints), match counts {300, 17, 0, 1, 150}; what
    tests/test_triangulate_gpu.py asserts (flags identical, accepted positions within 1e-5 relative, rejected positions zero), per pair."""
    from object_slam_amd.mappoint import TriKF, make_tri_kf
    L = lib()
    rng = np.random.default_rng(12)
    fx, fy, cx, cy, bf = synth.KITTI_K
    cam8 = np.array([fx, fy, cx, cy, np.float32(1) / np.float32(fx), np.float32(1) / np.float32(fy), bf, bf / fx], np.float32)
    N = 400
    nm = batch_counts(300)
    pairs = []
    for p in range(B):
        X = np.stack([rng.uniform(-15, 15, N), rng.uniform(-4, 4, N), rng.uniform(2, 60, N)], 1)
        X[:20, 2] = rng.uniform(-5, 0.5, 20)
        T1, W1 = tri_pose(rng, 0.3 * (p + 1))
        T2, W2 = tri_pose(rng, 0.5 + 0.3 * p)
        a1 = tri_make_kf(rng, X, T1, synth.KITTI_K, (0.6, 0.0, 0.6, 1.0, 0.3)[p], 0.7)
        a2 = tri_make_kf(rng, X, T2, synth.KITTI_K, (0.6, 0.0, 0.6, 1.0, 0.3)[p], 0.7)
        perm = rng.permutation(N).astype(np.int32)
        a2 = tuple(v[perm] for v in a2)
        inv = np.argsort(perm).astype(np.int32)
        m = np.sort(rng.choice(N, int(nm[p]), replace=False)).astype(np.int32)
        i2 = inv[m].copy()
        bad = rng.random(len(m)) < 0.15
        i2[bad] = rng.integers(0, N, int(bad.sum()))
        pairs.append(dict(kf1=(T1, W1, cam8) + a1, kf2=(T2, W2, cam8) + a2, i1=m, i2=i2.astype(np.int32)))
    assert [len(p["i1"]) for p in pairs] == [300, 17, 0, 1, 150]                           # one pair without matches, between the others
    ratio = np.float32(1.5) * np.float32(1.2)
    h = C.c_void_p()
    check(L.oslam_mappoint_create(C.byref(h), 0))
    G = 5

    def run(order):
        kfs = [(make_tri_kf(*pairs[p]["kf1"]), make_tri_kf(*pairs[p]["kf2"])) for p in order]     # (struct, the arrays it points into) twice per pair
        k1 = (TriKF * len(order))(*[a[0] for a, _ in kfs])
        k2 = (TriKF * len(order))(*[b[0] for _, b in kfs])
        start = np.concatenate([[0], np.cumsum([len(pairs[p]["i1"]) for p in order])]).astype(np.int32)
        M = int(start[-1])
        i1 = np.concatenate([pairs[p]["i1"] for p in order] + [np.zeros(1, np.int32)]).astype(np.int32)
        i2 = np.concatenate([pairs[p]["i2"] for p in order] + [np.zeros(1, np.int32)]).astype(np.int32)
        ok = np.full(M + G, 0xFF, np.uint8)
        x = np.full((M + G, 3), np.nan, np.float32)
        check(L.oslam_mp_triangulate_pairs(h, len(order), k1, k2, C.c_void_p(start.ctypes.data), C.c_void_p(i1.ctypes.data), C.c_void_p(i2.ctypes.data), C.c_void_p(SF.ctypes.data),
                                           C.c_void_p(LS2.ctypes.data), 8, C.c_float(float(ratio)), C.c_void_p(ok.ctypes.data), C.c_void_p(x.ctypes.data)))
        assert _all_sentinel(ok[M:]) and (_u32(x[M:]) == NAN32).all()                      # nothing behind [M]
        return [(ok[start[i]:start[i + 1]].copy(), x[start[i]:start[i + 1]].copy()) for i in range(len(order))]

    got = run(list(range(B)))
    rev = run(list(REV))
    accepted = 0
    for p, pr in enumerate(pairs):
        ok, x = got[p]
        rok, rx = oracle.triangulate(pr["kf1"], pr["kf2"], pr["i1"], pr["i2"], SF, LS2, ratio)
        assert np.array_equal(ok, rok), p
        sel = ok.astype(bool)
        if sel.any():
            rel = np.abs(x[sel] - rx[sel]).max(1) / np.maximum(np.abs(rx[sel]).max(1), 1e-3)
            assert rel.max() <= 1e-5, (p, rel.max())
        assert not x[~sel].any()
        accepted += int(sel.sum())
        r = int(np.where(REV == p)[0][0])
        (aok, ax), = run([p])
        for ook, ox in ((rev[r][0], rev[r][1]), (aok, ax)):
            assert np.array_equal(ook, ok) and np.array_equal(_u32(ox), _u32(x)), p
    assert 30 < accepted < 440, accepted
    assert 10 < int(got[0][0].sum()) < 290 and 5 < int(got[4][0].sum()) < 145, (got[0][0].sum(), got[4][0].sum())
    L.oslam_mappoint_destroy(h)
