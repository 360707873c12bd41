"""The stereo kernels (csrc/stereo.hip) against the numpy restatement of tests/stereo_common.py, to the bit, on the cases that take every decision of
Frame::ComputeStereoMatches on purpose: through the host entry point, and through oslam_stereo_match_batch_device in heterogeneous batches."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import stereo_common as sc
from batch_common import dev, fetch, side_stream
from object_slam_amd import KP_DTYPE, ORBextractor, StereoMatcher
from object_slam_amd._lib import check, lib

pytestmark = pytest.mark.gpu

SPARE_ROWS = 8          # rows behind the last image of a test-owned device buffer


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _extractor(case, max_batch=1):
    nf, sf, nl = case["cfg"]
    H, W = case["left"].shape
    return ORBextractor(nf, sf, nl, 20, 7, W, H, max_batch=max_batch)


_PYR_CHECKED = set()


def _check_pyramid(oracle, ex, case, side):
    """The extractor's pyramid of this image equals the oracle's, once per image."""
    key = hashlib.sha1(case[side].tobytes() + repr(case["cfg"]).encode()).hexdigest()
    if key in _PYR_CHECKED:
        return
    o = oracle.OrbExtractor(case["cfg"][0], case["cfg"][1], case["cfg"][2], 20, 7)
    o.extract(case[side])
    for l in range(case["cfg"][2]):
        assert np.array_equal(ex.pyramid_level(l), o.level(l)), (case["name"], side, l)
    _PYR_CHECKED.add(key)


def _host_run(oracle, sm, case):
    exL, exR = _extractor(case), _extractor(case)
    exL(case["left"])
    exR(case["right"])
    _check_pyramid(oracle, exL, case, "left")
    _check_pyramid(oracle, exR, case, "right")
    uR, dep = sm.ComputeStereoMatches(exL, exR, case["kL"], case["dL"], case["kR"], case["dR"], case["bf"], case["b"])
    exL.close(); exR.close()
    return uR, dep


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_host_entry_equals_restatement(oracle, name):
    case = sc.case_by_name(oracle, name)
    ref = sc.run_restatement(oracle, case)
    sm = StereoMatcher(max_keypoints=case["max_kps"])
    uR, dep = _host_run(oracle, sm, case)
    sm.close()
    assert np.array_equal(bits(uR), bits(ref["uRight"])), np.nonzero(bits(uR) != bits(ref["uRight"]))[0][:10]
    assert np.array_equal(bits(dep), bits(ref["depth"]))


def test_host_entry_small_after_large(oracle):
    """Two calls in a row on one handle: the results, the SADs and the best indices of the 2400-keypoint call stay in the handle's arrays behind the rows of the
    second call, which has 3 (then 1) keypoints; nothing of them may reach its median or its output."""
    sm = StereoMatcher()
    for name in ("size_2400_2400", "median_m3", "size_2049_2049", "median_m1_zero", "size_2400_2400", "clamp_single"):
        case = sc.case_by_name(oracle, name)
        ref = sc.run_restatement(oracle, case)
        uR, dep = _host_run(oracle, sm, case)
        assert np.array_equal(bits(uR), bits(ref["uRight"])) and np.array_equal(bits(dep), bits(ref["depth"])), name
    sm.close()


# ------------------------------------------------------------------------------------------------------------------------------------------
# oslam_stereo_match_batch_device
# ------------------------------------------------------------------------------------------------------------------------------------------

class Batch:
    """One stereo handle and two batch extractors for cases of one image size and extractor configuration."""

    def __init__(self, oracle, proto, max_batch, max_kps):
        self.oracle, self.L, self.max_batch, self.max_kps = oracle, lib(), max_batch, max_kps
        self.exL, self.exR = _extractor(proto, max_batch), _extractor(proto, max_batch)
        self.h = C.c_void_p()
        check(self.L.oslam_stereo_create(C.byref(self.h), max_batch, max_kps, 0))
        self.stream = side_stream()
        self.H, self.W = proto["left"].shape
        self.cfg, self.bf, self.b = proto["cfg"], proto["bf"], proto["b"]
        # rows behind an entry's count: valid keypoints that would match if a kernel read them
        fill = sc.case_by_name(oracle, "shift9")
        self.fill = (fill["kL"], fill["dL"], fill["kR"], fill["dR"])

    def close(self):
        self.L.oslam_stereo_destroy(self.h)
        self.exL.close(); self.exR.close()

    def _images(self, entries, side):
        """The images of a launch, tightly packed at the image's own width, in a buffer with spare rows behind the last one."""
        buf = np.zeros(len(entries) * self.W * self.H + SPARE_ROWS * self.W, np.uint8)
        for b, e in enumerate(entries):
            assert e[side].shape == (self.H, self.W) and e["cfg"] == self.cfg and e["bf"] == self.bf and e["b"] == self.b
            buf[b * self.W * self.H:(b + 1) * self.W * self.H] = e[side].reshape(-1)
        return dev(buf)

    def _rows(self, entries, kp_stride, alloc_rows, which):
        """[batch][kp_stride] keypoints and descriptors inside arrays of alloc_rows rows per entry; rows behind an entry's list are filled."""
        n = len(entries)
        k, d = np.zeros(n * alloc_rows, KP_DTYPE), np.zeros((n * alloc_rows, 32), np.uint8)
        fk, fd = (self.fill[0], self.fill[1]) if which == "L" else (self.fill[2], self.fill[3])
        idx = np.arange(n * alloc_rows) % len(fk)
        k[:], d[:] = fk[idx], fd[idx]
        for b, e in enumerate(entries):
            m = len(e["k" + which])
            assert m <= kp_stride
            k[b * kp_stride:b * kp_stride + m] = e["k" + which]
            d[b * kp_stride:b * kp_stride + m] = e["d" + which]
        return dev(k), dev(d)

    def run(self, entries, kp_stride, counts="device", nL=None, nR=None, alloc_rows=None):
        """One launch.  counts: "device" (arrays) or "const"; nL / nR override the entries' list lengths.  Returns uR, dep [n][kp_stride] and n_matched [n]."""
        import torch
        n = len(entries)
        assert n <= self.max_batch and kp_stride <= self.max_kps
        alloc_rows = alloc_rows or kp_stride
        dL, dR = self._images(entries, "left"), self._images(entries, "right")
        kL, deL = self._rows(entries, kp_stride, alloc_rows, "L")
        kR, deR = self._rows(entries, kp_stride, alloc_rows, "R")
        nL = np.array([len(e["kL"]) for e in entries] if nL is None else nL, np.int32)
        nR = np.array([len(e["kR"]) for e in entries] if nR is None else nR, np.int32)
        cL, cR = dev(nL), dev(nR)
        torch.cuda.synchronize()
        s = self.stream.cuda_stream
        self.exL.extract_batch_device(dL.data_ptr(), n, self.W, self.W * self.H, s)
        self.exR.extract_batch_device(dR.data_ptr(), n, self.W, self.W * self.H, s)
        if counts == "device":
            a = (C.c_void_p(cL.data_ptr()), 0, C.c_void_p(cR.data_ptr()), 0)
        else:
            assert len(set(nL.tolist())) == 1 and len(set(nR.tolist())) == 1
            a = (None, int(nL[0]), None, int(nR[0]))
        check(self.L.oslam_stereo_match_batch_device(self.h, self.exL.h, self.exR.h, n, kp_stride, C.c_void_p(kL.data_ptr()), C.c_void_p(deL.data_ptr()), a[0], a[1],
                                                     C.c_void_p(kR.data_ptr()), C.c_void_p(deR.data_ptr()), a[2], a[3], self.cfg[2], C.c_float(self.bf), C.c_float(self.b),
                                                     C.c_void_p(s)))
        self.stream.synchronize()
        pu, pd, pn = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(self.L.oslam_stereo_results_device(self.h, C.byref(pu), C.byref(pd), C.byref(pn)))
        return (fetch(self.L, pu, n * kp_stride, np.float32).reshape(n, kp_stride), fetch(self.L, pd, n * kp_stride, np.float32).reshape(n, kp_stride),
                fetch(self.L, pn, n, np.int32))

    def check(self, entries, kp_stride, counts="device", independence=True):
        """Every entry equals the restatement; with `independence`, also its result in the reversed batch and alone."""
        got = self.run(entries, kp_stride, counts)
        for b, e in enumerate(entries):
            ref = e["expect"] if "expect" in e else sc.run_restatement(self.oracle, e)
            N = len(e["kL"])
            assert got[2][b] == ref["n_before"], (e["name"], got[2][b], ref["n_before"])
            assert np.array_equal(bits(got[0][b, :N]), bits(ref["uRight"])), (e["name"], np.nonzero(bits(got[0][b, :N]) != bits(ref["uRight"]))[0][:10])
            assert np.array_equal(bits(got[1][b, :N]), bits(ref["depth"])), e["name"]
        if independence:
            rev = self.run(entries[::-1], kp_stride, counts)
            for b, e in enumerate(entries):
                N, rb = len(e["kL"]), len(entries) - 1 - b
                assert rev[2][rb] == got[2][b] and np.array_equal(bits(rev[0][rb, :N]), bits(got[0][b, :N])) and np.array_equal(bits(rev[1][rb, :N]), bits(got[1][b, :N])), e["name"]
                alone = self.run([e], kp_stride, counts)
                assert alone[2][0] == got[2][b] and np.array_equal(bits(alone[0][0, :N]), bits(got[0][b, :N])) and np.array_equal(bits(alone[1][0, :N]), bits(got[1][b, :N])), e["name"]
        return got


def _nothing(N):
    return dict(uRight=np.full(N, -1, np.float32), depth=np.full(N, -1, np.float32), n_before=0)


def _degenerate(oracle):
    """A pair without right keypoints and a pair without left keypoints (both with their images)."""
    base = sc.case_by_name(oracle, "shift9")
    empty_right = dict(base, name="empty_right", kR=base["kR"][:0], dR=base["dR"][:0], expect=_nothing(len(base["kL"])))
    n0 = dict(base, name="n0", kL=base["kL"][:0], dL=base["dL"][:0], expect=_nothing(0))
    return empty_right, n0


def test_batch_device_mixed_large(oracle):
    """One launch at kp_stride == max_keypoints: a 2400-keypoint pair, an ordinary pair, a pair without right keypoints, a pair with N = 0, the Hamming / tie
    pair — counts from device arrays."""
    g = lambda n: sc.case_by_name(oracle, n)
    empty_right, n0 = _degenerate(oracle)
    bt = Batch(oracle, g("shift9"), 5, sc.MAX_KPS)
    bt.check([g("size_2400_2400"), g("shift9"), empty_right, n0, g("hamming")], sc.MAX_KPS)
    # a small launch straight after the large one, on the same rows of the handle
    bt.check([g("median_m3"), n0, g("median_m1_zero")], sc.MAX_KPS)
    bt.close()


def test_batch_device_stride_below_capacity(oracle):
    """kp_stride = 400 on a handle of 2400: the gates, the borders (level 0 in the test's own buffer, its last row included), the alignment residues and the
    hand-made images in one launch; then equal counts as constants and as device arrays."""
    g = lambda n: sc.case_by_name(oracle, n)
    empty_right, n0 = _degenerate(oracle)
    bt = Batch(oracle, g("shift9"), 8, sc.MAX_KPS)
    bt.check([g("shift9"), g("octave_hi"), empty_right, g("borders"), g("alignment"), n0, g("corners"), g("octave_lo")], 400)
    bt.check([g("median_zero_minority"), g("median_zero_majority"), g("median_threshold"), g("parabola_single"), g("periodic5"), g("shifted5"), g("flat"), g("clamp_mixed")],
             400)
    two = [g("median_zero_minority"), g("median_threshold")]               # 5 and 5 keypoints on both sides
    a = bt.check(two, 400, counts="const")
    b = bt.check(two, 400, counts="device", independence=False)
    assert all(np.array_equal(x[:, :5].view(np.uint32), y[:, :5].view(np.uint32)) for x, y in zip(a[:2], b[:2])) and np.array_equal(a[2], b[2])
    odd = dict(g("size_1025_1025"), name="size_1025_1025_swapped", left=g("shift9")["right"], right=g("shift9")["left"])   # another pair of the same counts
    odd.pop("ref", None)
    bt.check([g("size_1025_1025"), odd], 1025, counts="const")             # an odd stride
    bt.close()


def test_batch_device_odd_image(oracle):
    """322 x 241 images tightly packed: every image after the first starts at an address that is no multiple of 4, and neither width nor height is one."""
    g = lambda n: sc.case_by_name(oracle, n)
    bt = Batch(oracle, g("shift6_odd"), 6, sc.MAX_KPS)
    # entries 1, 3 and 5 start at 2 modulo 4 (322 * 241 = 77602): there the corner case reaches the word in front of its level (tests/test_stereo_cases_cpu.py,
    # test_corner_words); in the reversed launch the same pairs are entries 0, 2 and 4
    bt.check([g("shift6_odd"), g("corners_odd"), g("borders_odd"), g("corners_odd"), g("alignment_odd"), g("shift7_odd")], 400)
    bt.close()


def test_batch_device_table_and_overflow(oracle):
    """A pair whose row table fits, one that overflows it and one that fills it to the last item but one, in one launch on a handle as large as the lists."""
    g = lambda n: sc.case_by_name(oracle, n)
    n = g("wide_table")["max_kps"]
    bt = Batch(oracle, g("wide_table"), 3, n)
    bt.check([g("wide_table"), g("wide_overflow"), g("wide_nearfull")], n)
    bt.close()


def test_batch_device_refuses_count_above_stride(oracle):
    """An entry whose device count is above kp_stride (but within the handle's capacity) owns no such rows: it reports n_matched == -1, its output rows keep
    what the previous launch left there and the other entries are untouched.  The input arrays have max_keypoints rows per entry, so whatever a kernel
    reads for that entry lies inside them."""
    g = lambda n: sc.case_by_name(oracle, n)
    entries = [g("shift9"), g("octave_hi"), g("hamming")]
    stride = 400
    bt = Batch(oracle, g("shift9"), 3, sc.MAX_KPS)
    good = bt.run(entries, stride, alloc_rows=sc.MAX_KPS)
    for which, bad_n in (("nL", 1000), ("nR", stride + 1), ("nL", sc.MAX_KPS), ("nL", -1)):
        counts = {"nL": [len(e["kL"]) for e in entries], "nR": [len(e["kR"]) for e in entries]}
        counts[which][1] = bad_n
        got = bt.run(entries, stride, alloc_rows=sc.MAX_KPS, **counts)
        assert got[2][1] == -1 and got[2][0] == good[2][0] and got[2][2] == good[2][2], (which, bad_n, got[2])
        for x, y in zip(got[:2], good[:2]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (which, bad_n)
    again = bt.run(entries, stride, alloc_rows=sc.MAX_KPS)
    assert np.array_equal(again[2], good[2]) and np.array_equal(again[0].view(np.uint32), good[0].view(np.uint32))
    bt.close()
