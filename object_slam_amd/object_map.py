"""ctypes view of the object map maintenance (include/oslam_hip.h, "Object map maintenance"): Object3D::RejectOutliers (src/ObjectTypes.cc:152-162) with the
new-object path of Tracking::UpdateCurrentObject (src/Tracking.cc:1113-1199), Object3D::CalculateCenterAndSize (src/ObjectTypes.cc:805-833) and the merge sets of
Map::ObjectMapRegularization (src/Map.cc:47-112), for batches of independent point lists and maps.

`ObjectMap.reject_outliers`, `.center_and_size` and `.merge_sets` are launches of the gfx950 kernels (no CPU fallback: creating an ObjectMap fails without a
device).  Map points and objects are rows of flat arrays; the `pack_*` helpers build the records that name them.  Operators: the driver does not call them, it
still takes the caller's track_id per detection and skips the rejection.
"""
import ctypes as C

import numpy as np

from ._lib import Handle, check, device_call, lib, optptr, ptr
from ._proj_common import _consecutive

MODE_UPDATE, MODE_NEW_OBJECT = 0, 1
PATH_TEST5, PATH_TEST7, PATH_SHORTCUT = 0, 1, 2
TEST5_ABOVE = 3000
MIN_CLUSTER_POINTS, MAX_CLUSTER_POINTS, MAX_OBJECTS = 3000, 4000, 128
DONE, REFUSED_RECORD, REFUSED_CAPACITY = 0, -1, -2
MIN_OBJ3DMP_NUM = 5   # include/ObjectTypes.h: an object is created when more points than this survive

PROBLEM_DTYPE = np.dtype([("off", "<i4"), ("n", "<i4"), ("mode", "<i4"), ("reserved", "<i4")])
RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_candidates", "<i4"), ("n_clusters", "<i4"), ("n_kept", "<i4"), ("path", "<i4"), ("rounds", "<i4"), ("std_dev", "<f4"),
                         ("candidates_center", "<f4", (3,)), ("center", "<f4", (3,)), ("bbox", "<f4", (6,)), ("reserved", "<i4")])
MERGE_DTYPE = np.dtype([("n", "<i4"), ("off_obj", "<i4"), ("off_pair", "<i4"), ("reserved", "<i4")])
RESULT_BBOX_OFFSET = RESULT_DTYPE.fields["bbox"][1]   # bytes; with bbox_stride = RESULT_DTYPE.itemsize // 4 the result records are merge_sets' bbox rows


def _bind(L):
    if getattr(L, "_oslam_objmap_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int
    L.oslam_objmap_create.argtypes = [C.POINTER(vp)] + [i32] * 3
    L.oslam_objmap_destroy.argtypes = [vp]
    L.oslam_objmap_destroy.restype = None
    L.oslam_objmap_reject_outliers.argtypes = [vp, i32, vp, i32] + [vp] * 6
    L.oslam_objmap_reject_outliers_device.argtypes = [vp, i32, vp, i32] + [vp] * 7
    L.oslam_objmap_center_and_size.argtypes = [vp, i32, vp, i32, vp, vp]
    L.oslam_objmap_center_and_size_device.argtypes = [vp, i32, vp, i32, vp, vp, vp]
    L.oslam_objmap_merge_sets.argtypes = [vp, i32, vp, i32, vp, vp, vp, i32, i32] + [vp] * 5
    L.oslam_objmap_merge_sets_device.argtypes = [vp, i32, vp, i32, vp, vp, vp, i32, i32] + [vp] * 6
    L.oslam_objmap_set_timing.argtypes = [vp, i32]
    L.oslam_objmap_last_kernel_ms.argtypes = [vp, vp]
    L._oslam_objmap_bound = True
    return L


def pack_problems(n, mode=MODE_UPDATE, off=None):
    """PROBLEM_DTYPE records.  mode: one value or one per problem; off defaults to consecutive rows in the order given."""
    n = np.asarray(n, np.int32).reshape(-1)
    pr = np.zeros(len(n), PROBLEM_DTYPE)
    pr["n"], pr["mode"] = n, mode
    pr["off"] = _consecutive(n) if off is None else np.asarray(off, np.int32)
    return pr


def pack_merge_problems(n, off_obj=None, off_pair=None):
    """MERGE_DTYPE records.  The offsets default to consecutive rows and n * n pair blocks."""
    n = np.asarray(n, np.int32).reshape(-1)
    pr = np.zeros(len(n), MERGE_DTYPE)
    pr["n"] = n
    pr["off_obj"] = _consecutive(n) if off_obj is None else np.asarray(off_obj, np.int32)
    pr["off_pair"] = _consecutive(n * n) if off_pair is None else np.asarray(off_pair, np.int32)
    return pr


def new_results(n, fill=0):
    """n RESULT_DTYPE records whose every byte is `fill`"""
    return np.full(n * RESULT_DTYPE.itemsize, fill, np.uint8).view(RESULT_DTYPE)


def _arr(a, dt, shape):
    a = a if isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous else np.ascontiguousarray(a, dt)
    return a.reshape(shape)


class ObjectMap(Handle):
    """A handle for calls of up to max_problems problems, clustering point lists of up to max_cluster_points (3000 .. 4000) points and maps of up to max_objects
    (<= 128) objects."""

    def __init__(self, max_problems=512, max_cluster_points=MIN_CLUSTER_POINTS, max_objects=MAX_OBJECTS):
        super().__init__(_bind(lib()), "oslam_objmap", max_problems, max_cluster_points, max_objects)

    def set_timing(self, on=True):
        check(self.L.oslam_objmap_set_timing(self.h, int(bool(on))))

    def last_kernel_ms(self):
        """milliseconds of the last call's kernel; needs set_timing()"""
        ms = np.zeros(2, np.float32)
        check(self.L.oslam_objmap_last_kernel_ms(self.h, ptr(ms)))
        return float(ms[0])

    def reject_outliers(self, problems, pos, label_cnt=None, label_sum=None, keep=None, cluster=None, results=None, device=False):
        """RejectOutliers (mode UPDATE) or the new-object rejection (mode NEW_OBJECT) of every problem.  problems: PROBLEM_DTYPE (pack_problems); pos [n_rows, 3]
        float32; label_cnt, label_sum [n_rows] int32 (not needed when every problem is NEW_OBJECT).  Returns dict(keep uint8 [n_rows], cluster int32 [n_rows],
        results RESULT_DTYPE [n_problems]); arrays given by the caller are written in place."""
        problems = np.ascontiguousarray(problems, PROBLEM_DTYPE)
        pos = _arr(pos, np.float32, (-1, 3))
        nr, n = len(pos), len(problems)
        label_cnt = None if label_cnt is None else _arr(label_cnt, np.int32, (-1,))
        label_sum = None if label_sum is None else _arr(label_sum, np.int32, (-1,))
        keep = np.zeros(nr, np.uint8) if keep is None else keep
        cluster = np.full(nr, -1, np.int32) if cluster is None else cluster
        results = new_results(n) if results is None else results
        assert keep.dtype == np.uint8 and keep.size == nr and cluster.dtype == np.int32 and cluster.size == nr and results.dtype == RESULT_DTYPE and results.size == n
        assert (label_cnt is None or label_cnt.size == nr) and (label_sum is None or label_sum.size == nr)
        if not device:
            check(self.L.oslam_objmap_reject_outliers(self.h, n, optptr(problems), nr, optptr(pos), optptr(label_cnt), optptr(label_sum), optptr(keep), optptr(cluster), optptr(results)))
        else:
            with device_call([problems, pos, label_cnt, label_sum, keep, cluster, results], outputs=(keep, cluster, results)) as (addr, stream):
                check(self.L.oslam_objmap_reject_outliers_device(self.h, n, addr(problems), nr, addr(pos), addr(label_cnt), addr(label_sum), addr(keep), addr(cluster), addr(results), stream))
        return dict(keep=keep, cluster=cluster, results=results)

    def center_and_size(self, problems, pos, results=None, device=False):
        """CalculateCenterAndSize of every problem's rows: n_kept, center and bbox (max x, y, z, min x, y, z) of results."""
        problems = np.ascontiguousarray(problems, PROBLEM_DTYPE)
        pos = _arr(pos, np.float32, (-1, 3))
        nr, n = len(pos), len(problems)
        results = new_results(n) if results is None else results
        assert results.dtype == RESULT_DTYPE and results.size == n
        if not device:
            check(self.L.oslam_objmap_center_and_size(self.h, n, optptr(problems), nr, optptr(pos), optptr(results)))
        else:
            with device_call([problems, pos, results], outputs=(results,)) as (addr, stream):
                check(self.L.oslam_objmap_center_and_size_device(self.h, n, addr(problems), nr, addr(pos), addr(results), stream))
        return dict(results=results)

    def merge_sets(self, problems, label, track_id, bbox, ratio=None, member=None, target=None, n_sets=None, status=None, n_pairs=None, device=False):
        """The merge sets of every map.  problems: MERGE_DTYPE (pack_merge_problems); label, track_id [n_rows] int32; bbox [n_rows, 6] float32 (max x, y, z, min x, y, z).
        Returns dict(ratio float32 [n_pairs], member uint8 [n_pairs], target int32 [n_rows], n_sets, status int32 [n_problems]); per problem ratio is [n, n] at
        off_pair (i < j written), member [n_sets, n] at off_pair and target [n_sets] at off_obj."""
        problems = np.ascontiguousarray(problems, MERGE_DTYPE)
        label, track_id, bbox = _arr(label, np.int32, (-1,)), _arr(track_id, np.int32, (-1,)), _arr(bbox, np.float32, (-1, 6))
        nr, n = len(label), len(problems)
        assert len(track_id) == nr and len(bbox) == nr
        if n_pairs is None:
            n_pairs = int(max([0] + [int(p["off_pair"]) + int(p["n"]) ** 2 for p in problems])) if ratio is None else ratio.size
        ratio = np.full(n_pairs, np.nan, np.float32) if ratio is None else ratio
        member = np.zeros(n_pairs, np.uint8) if member is None else member
        target = np.full(nr, -1, np.int32) if target is None else target
        n_sets = np.zeros(n, np.int32) if n_sets is None else n_sets
        status = np.zeros(n, np.int32) if status is None else status
        outs = (ratio, member, target, n_sets, status)
        if not device:
            check(self.L.oslam_objmap_merge_sets(self.h, n, optptr(problems), nr, optptr(label), optptr(track_id), optptr(bbox), 6, n_pairs, *[optptr(o) for o in outs]))
        else:
            with device_call([problems, label, track_id, bbox] + list(outs), outputs=outs) as (addr, stream):
                check(self.L.oslam_objmap_merge_sets_device(self.h, n, addr(problems), nr, addr(label), addr(track_id), addr(bbox), 6, n_pairs, *[addr(o) for o in outs], stream))
        return dict(ratio=ratio, member=member, target=target, n_sets=n_sets, status=status)


def sets_of(out, problems, b):
    """the merge sets of problem b as a list of (sorted member indices, target index)"""
    p = problems[b]
    n, ns = int(p["n"]), int(out["n_sets"][b])
    mem = out["member"][int(p["off_pair"]):int(p["off_pair"]) + ns * n].reshape(ns, n)
    return [([int(i) for i in np.nonzero(mem[s])[0]], int(out["target"][int(p["off_obj"]) + s])) for s in range(ns)]
