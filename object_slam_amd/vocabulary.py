"""ctypes view of the ORB vocabulary (include/oslam_hip.h, "ORB vocabulary"): the DBoW2 tree the reference loads from ORBvoc.txt
(src/System.cc:64-76) and applies with transform(desc, BowVector, FeatureVector, 4).

`Vocabulary.load(path)` reads the text format, `Vocabulary.from_arrays(...)` takes the same tree from arrays, `save_text(path, ...)` writes
the format (tests generate their trees with it; so can users who train their own).  `transform` runs the gfx950 kernel (no CPU fallback:
it fails without a device); `transform_host` is the host descent the tracking driver uses over an operator table without a device.
"""
import ctypes as C
import os
import sys

import numpy as np

from ._lib import Handle, OslamError, check, lib, ptr

SCORING = ("L1_NORM", "L2_NORM", "CHI_SQUARE", "KL", "BHATTACHARYYA", "DOT_PRODUCT")
WEIGHTING = ("TF_IDF", "TF", "IDF", "BINARY")


def _bind(L):
    if getattr(L, "_oslam_voc_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int
    L.oslam_voc_load_text.argtypes = [C.POINTER(vp), C.c_char_p]
    L.oslam_voc_create.argtypes = [C.POINTER(vp), i32, i32, i32, i32, i32, vp, vp, vp, vp]
    L.oslam_voc_destroy.argtypes = [vp]
    L.oslam_voc_destroy.restype = None
    L.oslam_voc_info.argtypes = [vp, vp]
    L.oslam_voc_get_nodes.argtypes = [vp, vp, vp, vp, vp, vp]
    L.oslam_voc_upload.argtypes = [vp, i32]
    L.oslam_voc_transform_device.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]
    L.oslam_voc_transform.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    L.oslam_voc_transform_host.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    L.oslam_voc_vectors.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.oslam_voc_score.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp]
    L.oslam_voc_score.restype = C.c_double
    L.oslam_slam_set_vocabulary.argtypes = [vp, vp]
    L._oslam_voc_bound = True
    return L


def save_text(path, k, L, scoring, weighting, parent, is_leaf, desc, weight):
    """Writes a vocabulary in the text format of DBoW2's loadFromTextFile (ORB-SLAM2 fork): line 1 `k L scoring weighting`, then one line per
    node id 1 .. n: `parent_id is_leaf b0 .. b31 weight` (entry j of the arrays is node id j + 1; the root, id 0, has no line).  Weights are
    written with repr(), the shortest text that reads back to the same double."""
    parent, is_leaf = np.asarray(parent), np.asarray(is_leaf)
    desc = np.asarray(desc, np.uint8).reshape(len(parent), 32)
    with open(path, "w") as f:
        f.write("%d %d %d %d\n" % (k, L, scoring, weighting))
        for j in range(len(parent)):
            f.write("%d %d %s %r\n" % (int(parent[j]), 1 if is_leaf[j] else 0, " ".join(map(str, desc[j].tolist())), float(weight[j])))


class Vocabulary(Handle):
    _destroy = "oslam_voc_destroy"   # (the handle comes from one of the class methods)

    def __init__(self, handle):
        self.L = _bind(lib())
        self.h = handle

    @classmethod
    def load(cls, path):
        """ORBVocabulary::loadFromTextFile; a file that does not parse raises OslamError (OSLAM_E_INVALID, the message names the line)."""
        L = _bind(lib())
        h = C.c_void_p()
        check(L.oslam_voc_load_text(C.byref(h), str(path).encode()))
        return cls(h)

    @classmethod
    def from_arrays(cls, k, L_, scoring, weighting, parent, is_leaf, desc, weight):
        L = _bind(lib())
        parent = np.ascontiguousarray(parent, np.int32)
        is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        desc = np.ascontiguousarray(desc, np.uint8)
        weight = np.ascontiguousarray(weight, np.float64)
        n = len(parent)
        assert len(is_leaf) == n and desc.size == 32 * n and len(weight) == n
        h = C.c_void_p()
        check(L.oslam_voc_create(C.byref(h), k, L_, scoring, weighting, n, ptr(parent), ptr(is_leaf), ptr(desc), ptr(weight)))
        return cls(h)

    @property
    def info(self):
        out = np.zeros(8, np.int32)
        check(self.L.oslam_voc_info(self.h, ptr(out)))
        return dict(zip(("k", "L", "scoring", "weighting", "nodes", "words", "max_depth", "max_children"), out.tolist()))

    def nodes(self):
        """(parent, is_leaf, desc [n, 32], weight, word_id) by node id - 1, as read."""
        n = self.info["nodes"]
        parent, leaf, desc = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8)
        weight, word = np.zeros(n, np.float64), np.zeros(n, np.int32)
        check(self.L.oslam_voc_get_nodes(self.h, ptr(parent), ptr(leaf), ptr(desc), ptr(weight), ptr(word)))
        return parent, leaf, desc, weight, word

    def upload(self, device=0):
        check(self.L.oslam_voc_upload(self.h, device))

    def transform_host(self, desc, levelsup=4):
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        word, node, weight = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float64)
        check(self.L.oslam_voc_transform_host(self.h, ptr(desc), n, levelsup, ptr(word), ptr(node), ptr(weight)))
        return word, node, weight

    def transform_array(self, desc, levelsup=4):
        """One host array [N, 32] through the kernel (oslam_voc_transform: upload, launch, download)."""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        word, node, weight = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float64)
        check(self.L.oslam_voc_transform(self.h, ptr(desc), n, levelsup, ptr(word), ptr(node), ptr(weight)))
        return word, node, weight

    def transform(self, desc_batch, levelsup=4, stride=None):
        """desc_batch: one uint8 array [N, 32] or a list of them (the batch layout of oslam_voc_transform_device).  Runs the gfx950 kernel on the
        current device; returns (word, node, weight) — arrays for one input array, lists of arrays for a list."""
        import torch
        single = not isinstance(desc_batch, (list, tuple))
        arrays = [np.ascontiguousarray(a, np.uint8).reshape(-1, 32) for a in ([desc_batch] if single else desc_batch)]
        n = len(arrays)
        counts = np.array([len(a) for a in arrays], np.int32)
        stride = int(stride or max(1, counts.max()))
        assert counts.max() <= stride
        dev = torch.device("cuda", torch.cuda.current_device())
        d_arrays = [torch.from_numpy(a if len(a) else np.zeros((1, 32), np.uint8)).to(dev) for a in arrays]
        d_ptrs = torch.tensor([t.data_ptr() for t in d_arrays], dtype=torch.int64, device=dev)
        d_counts = torch.from_numpy(counts).to(dev)
        # 0xff / NaN fill: entries beyond a count are not written
        d_word = torch.full((n, stride), -1, dtype=torch.int32, device=dev)
        d_node = torch.full((n, stride), -1, dtype=torch.int32, device=dev)
        d_weight = torch.full((n, stride), float("nan"), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        check(self.L.oslam_voc_transform_device(self.h, d_ptrs.data_ptr(), d_counts.data_ptr(), n, stride, levelsup, d_word.data_ptr(), d_node.data_ptr(),
                                                d_weight.data_ptr(), None))
        torch.cuda.synchronize()
        word, node, weight = d_word.cpu().numpy().view(np.uint32), d_node.cpu().numpy().view(np.uint32), d_weight.cpu().numpy()
        self._last_full = (word, node, weight)   # (tests look at the entries beyond the counts)
        res = [(word[i, :c].copy(), node[i, :c].copy(), weight[i, :c].copy()) for i, c in enumerate(counts)]
        if single:
            return res[0]
        return [r[0] for r in res], [r[1] for r in res], [r[2] for r in res]

    def vectors(self, word, node, weight):
        """(bow_ids, bow_vals, fv_nodes, fv_start, fv_items): BowVector (word id ascending) and the FeatureVector as CSR (oslam_bow_side2_t's form)."""
        word, node = np.ascontiguousarray(word, np.uint32), np.ascontiguousarray(node, np.uint32)
        weight = np.ascontiguousarray(weight, np.float64)
        n = len(word)
        m = max(n, 1)
        bi, bv = np.zeros(m, np.uint32), np.zeros(m, np.float64)
        fn, fs, fi = np.zeros(m, np.uint32), np.zeros(m + 1, np.int32), np.zeros(m, np.int32)
        nb, nf = C.c_int32(0), C.c_int32(0)
        check(self.L.oslam_voc_vectors(self.h, n, ptr(word), ptr(node), ptr(weight), ptr(bi), ptr(bv), C.addressof(nb), ptr(fn), ptr(fs), ptr(fi), C.addressof(nf)))
        return bi[:nb.value].copy(), bv[:nb.value].copy(), fn[:nf.value].copy(), fs[:nf.value + 1].copy(), fi[:fs[nf.value]].copy()

    def score(self, a, b):
        """score of two BowVectors (ids, vals); only L1_NORM vocabularies (the reference's) are scored, others raise OslamError."""
        ia, va = np.ascontiguousarray(a[0], np.uint32), np.ascontiguousarray(a[1], np.float64)
        ib, vb = np.ascontiguousarray(b[0], np.uint32), np.ascontiguousarray(b[1], np.float64)
        rc = C.c_int(0)
        s = self.L.oslam_voc_score(self.h, len(ia), ptr(ia), ptr(va), len(ib), ptr(ib), ptr(vb), C.addressof(rc))
        check(rc.value)
        return float(s)


def load_like_system(path):
    """What System::System does with strVocFile (src/System.cc:65-76), for the dataset runners: prints the reference's messages and returns the
    Vocabulary; a file that exists but does not load -> the reference's two error lines (plus the parser's own, which names the line) and SystemExit(1).
    One departure, kept for the runs that have no vocabulary file at hand: a path that does not exist is not an error — one line says that the substitute
    vocabulary (include/oslam_slam.h) is used, and None is returned."""
    if not os.path.isfile(path):
        print("No vocabulary file at %s: using the substitute vocabulary (two-level 10 x 10 tree, include/oslam_slam.h)" % path)
        return None
    print("\nLoading ORB Vocabulary. This could take a while...")
    try:
        voc = Vocabulary.load(path)
    except OslamError as e:
        print("Wrong path to vocabulary. \nFalied to open at: %s\n(Failed to open: %s)" % (path, e), file=sys.stderr)
        raise SystemExit(1)
    i = voc.info
    print("Vocabulary loaded!  (%s: k = %d, L = %d, %d nodes, %d words, %s / %s)\n" % (path, i["k"], i["L"], i["nodes"], i["words"], WEIGHTING[i["weighting"]], SCORING[i["scoring"]]))
    return voc
