"""Stage parity of the HIP ORB extractor against the CPU oracle, shared by tests/test_extractor_gpu.py and tests/test_extractor_paths_gpu.py.

Everything is compared bit-exact: level sizes, pyramid bytes, blurred bytes, FAST candidates (order, x, y, score), quad-tree survivors (order),
keypoints (all 7 fields) and descriptors.  The image reaches the handle either through the host entry (ORBextractor.__call__, which stages it into
a 64-byte aligned pitch) or through extract_batch_device from a device buffer with a chosen base offset, row stride and image stride."""
import collections
import hashlib

import numpy as np

from object_slam_amd import ORBextractor

KP_FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")

# Layout of a batch in a device buffer: `base_offset` bytes after a 256-byte aligned address, `stride` bytes per row, `image_stride` bytes per image
Layout = collections.namedtuple("Layout", "base_offset stride image_stride")

_LEAD = 256        # bytes in front of the first image: the base pointer may be moved without leaving the allocation
_SLACK_ROWS = 8    # rows behind the last image: no test depends on a read at the very end of an allocation

_ref_cache = {}


def oracle_ref(oracle, cfg, img, blur_sse2=True):
    """The oracle's stage outputs for one image, computed once per (configuration, rounding, image) and shared read-only."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    key = (tuple(sorted(cfg.items())), bool(blur_sse2), img.shape, hashlib.sha1(img.tobytes()).hexdigest())
    ref = _ref_cache.get(key)
    if ref is None:
        oe = oracle.OrbExtractor(cfg["nfeatures"], cfg["scaleFactor"], cfg["nlevels"], cfg["iniThFAST"], cfg["minThFAST"])
        if not blur_sse2:
            oe.set_blur_sse2(False)
        kps, desc = oe.extract(img)
        levels = []
        for l in range(cfg["nlevels"]):
            levels.append(dict(size=oe.level_size(l), image=oe.level(l), cand=oe.candidates(l), keys=oe.level_keys(l), blurred=oe.blurred(l)))
        ref = dict(kps=kps, desc=desc, levels=levels)
        for a in [kps, desc] + [v for lv in levels for v in lv.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        _ref_cache[key] = ref
    return ref


def assert_result_parity(kps, desc, ref, what=""):
    assert len(kps) == len(ref["kps"]), "%s: %d vs %d keypoints" % (what, len(kps), len(ref["kps"]))
    for f in KP_FIELDS:
        np.testing.assert_array_equal(kps[f], ref["kps"][f], err_msg="%s %s" % (what, f))
    np.testing.assert_array_equal(desc, ref["desc"], err_msg="%s descriptors" % what)


def assert_stage_parity(ex, b, ref, kps, desc, what=""):
    """Every stage of batch element b of the handle's last batch against the oracle's record `ref`; kps / desc are the element's results."""
    for l, o in enumerate(ref["levels"]):
        assert ex.level_size(l) == o["size"]
        np.testing.assert_array_equal(ex.pyramid_level(l, b), o["image"], err_msg="%s pyramid level %d" % (what, l))
        cand = ex.debug_candidates(l, b)
        oc = o["cand"]
        assert len(cand) == len(oc), "%s level %d: %d vs %d candidates" % (what, l, len(cand), len(oc))
        np.testing.assert_array_equal(cand[:, 0], oc["x"].astype(np.int32), err_msg="%s candidates x level %d" % (what, l))
        np.testing.assert_array_equal(cand[:, 1], oc["y"].astype(np.int32), err_msg="%s candidates y level %d" % (what, l))
        np.testing.assert_array_equal(cand[:, 2], oc["response"].astype(np.int32), err_msg="%s candidates score level %d" % (what, l))
        keys = ex.debug_level_keys(l, b)
        ok = o["keys"]
        assert len(keys) == len(ok), "%s level %d: %d vs %d survivors" % (what, l, len(keys), len(ok))
        np.testing.assert_array_equal(keys[:, 0], ok["x"].astype(np.int32), err_msg="%s survivors x level %d" % (what, l))
        np.testing.assert_array_equal(keys[:, 1], ok["y"].astype(np.int32), err_msg="%s survivors y level %d" % (what, l))
        if o["blurred"] is not None:   # the oracle, like the reference, blurs only levels that kept a keypoint
            np.testing.assert_array_equal(ex.debug_blurred(l, b), o["blurred"], err_msg="%s blur level %d" % (what, l))
    assert_result_parity(kps, desc, ref, what)


def device_batch(imgs, layout, fill=0):
    """imgs [B, h, w] uint8 -> (torch uint8 tensor that owns the device buffer, address of image 0).  Every byte that is not a pixel of an image row
    (row padding, gaps between images, the margins in front and behind) holds `fill`."""
    import torch
    imgs = np.ascontiguousarray(imgs, dtype=np.uint8)
    B, h, w = imgs.shape
    assert layout.stride >= w and (B == 1 or layout.image_stride >= layout.stride * h)
    start = _LEAD + layout.base_offset
    host = np.full(start + (B - 1) * layout.image_stride + (h + _SLACK_ROWS) * layout.stride, fill, np.uint8)
    view = np.lib.stride_tricks.as_strided(host[start:], shape=(B, h, w), strides=(layout.image_stride, layout.stride, 1))
    view[...] = imgs
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 256 == 0
    return t, t.data_ptr() + start


def run_stages(oracle, cfg, imgs, elements=None, layout=None, fill=0, blur_sse2=True, max_batch=None, full=None):
    """One extraction and its parity checks.  imgs: one image [h, w] for the host entry (layout None), or a batch [B, h, w] fed through
    extract_batch_device in `layout`.  `elements`: the batch elements whose results are compared with the oracle (default: all); `full`: those
    of them that also get the comparison of every stage (default: all of `elements`).  Returns (keypoint count per element of `elements`, the
    handle's plan record, {element: (keypoints, descriptors)})."""
    imgs = np.asarray(imgs)
    host = layout is None
    batch = imgs[None] if host else imgs
    B, h, w = batch.shape
    elements = list(range(B)) if elements is None else list(elements)
    full = set(elements if full is None else full)
    ex = ORBextractor(width=w, height=h, max_batch=max_batch or B, **cfg)
    try:
        if not blur_sse2:
            ex.set_blur_rounding(0)
        if host:
            out = {0: ex(batch[0])}
        else:
            import torch
            buf, addr = device_batch(batch, layout, fill)
            ex.extract_batch_device(addr, B, layout.stride, layout.image_stride, torch.cuda.current_stream().cuda_stream)
            out = {b: ex.fetch(b) for b in elements}   # buf stays alive below: level 0 of the pyramid is read from it
        plan = ex.debug_plan()
        for b in elements:
            ref = oracle_ref(oracle, cfg, batch[b], blur_sse2)
            if b in full:
                assert_stage_parity(ex, b, ref, out[b][0], out[b][1], "element %d" % b)
            else:
                assert_result_parity(out[b][0], out[b][1], ref, "element %d" % b)
    finally:
        ex.close()
    return [len(out[b][0]) for b in elements], plan, out


def _stages(oracle, cfg, img, b=0, layout=None, fill=0, blur_sse2=True):
    """Stage parity of one batch element; returns its keypoint count.  img [h, w]: through the host entry (b = 0); img [B, h, w] with a Layout:
    through extract_batch_device, element b compared."""
    counts, _, _ = run_stages(oracle, cfg, img, elements=[b], layout=layout, fill=fill, blur_sse2=blur_sse2)
    return counts[0]
