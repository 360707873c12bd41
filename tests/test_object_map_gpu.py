"""GPU: the object map maintenance (include/oslam_hip.h, "Object map maintenance") against the numpy restatement of tests/object_map_common.py.  Exact parity:
keep, cluster, every count and the path equal, every float bit for bit with its NaN pattern.  No tolerance anywhere: every output is a fixed sequence of IEEE
operations that the restatement repeats (the library is built without contraction)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import object_map_common as omc
from object_slam_amd import object_map as om
from object_slam_amd._lib import OSLAM_E_CAPACITY, OSLAM_E_INVALID, OslamError, check

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "object_slam_amd")
f32 = np.float32
FILL, GAP = 0xA5, 3     # the byte every output holds before a call; rows between the problems that no problem owns
HAND, MERGE = omc.hand_cases(), omc.merge_hand_cases()


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def handle():
    h = om.ObjectMap(1024, 3000, 128)
    yield h
    h.close()


def _batch(ps, gap=GAP):
    """problems with `gap` rows between them -> (records, pos, cnt, total)"""
    offs, rows = [], gap
    for p in ps:
        offs.append(rows)
        rows += len(p["pos"]) + gap
    pos, cnt, total = np.full((rows, 3), 7.25, f32), np.full(rows, 1, np.int32), np.full(rows, 1, np.int32)
    for p, o in zip(ps, offs):
        n = len(p["pos"])
        pos[o:o + n], cnt[o:o + n], total[o:o + n] = p["pos"], p["cnt"], p["total"]
    return om.pack_problems([len(p["pos"]) for p in ps], [p["mode"] for p in ps], offs), pos, cnt, total


def _filled(n, dtype):
    return np.full(n * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype)


def _run(h, ps, device=False, gap=GAP):
    pr, pos, cnt, total = _batch(ps, gap)
    return pr, h.reject_outliers(pr, pos, cnt, total, keep=_filled(len(pos), np.uint8), cluster=_filled(len(pos), np.int32), results=om.new_results(len(ps), FILL), device=device)


def _check_extent(R, want_center, want_bbox, fill_res):
    if want_center is None:   # untouched
        assert R["center"].tobytes() == fill_res["center"].tobytes() and R["bbox"].tobytes() == fill_res["bbox"].tobytes()
    else:
        assert np.array_equal(_bits(R["center"]), _bits(want_center)), (R["center"], want_center)
        assert np.array_equal(_bits(R["bbox"]), _bits(want_bbox)), (R["bbox"], want_bbox)


def _check(pr, got, ps, answers):
    fill_res = om.new_results(1, FILL)[0]
    owned = np.zeros(len(got["keep"]), bool)
    for b, (p, w) in enumerate(zip(ps, answers)):
        o, n, R = int(pr["off"][b]), int(pr["n"][b]), got["results"][b]
        owned[o:o + n] = True
        assert R["status"] == om.DONE, (b, R["status"])
        assert np.array_equal(got["keep"][o:o + n], w["keep"]), (b, np.nonzero(got["keep"][o:o + n] != w["keep"])[0][:10])
        assert np.array_equal(got["cluster"][o:o + n], w["cluster"]), (b, np.nonzero(got["cluster"][o:o + n] != w["cluster"])[0][:10])
        assert (R["n_candidates"], R["n_clusters"], R["n_kept"], R["path"]) == (w["n_candidates"], w["n_clusters"], w["n_kept"], w["path"]), b
        assert _bits(R["std_dev"]) == _bits(w["std_dev"]), (b, R["std_dev"], w["std_dev"])
        assert np.array_equal(_bits(R["candidates_center"]), _bits(w["candidates_center"])), b
        _check_extent(R, w["center"], w["bbox"], fill_res)
    assert (got["keep"][~owned] == FILL).all() and (got["cluster"][~owned].view(np.uint8) == FILL).all()


def _answers(ps):
    return [omc.reject_outliers(p["pos"], p["cnt"], p["total"], p["mode"]) for p in ps]


@pytest.fixture(scope="module")
def hand_answers():
    return _answers(list(HAND.values()))


@pytest.fixture(scope="module")
def hand_first(handle):
    return _run(handle, list(HAND.values()))


def test_hand_cases_parity_and_hand_answers(hand_first, hand_answers):
    pr, got = hand_first
    _check(pr, got, list(HAND.values()), hand_answers)
    for b, c in enumerate(HAND.values()):   # and the answers written out by hand
        o, n = int(pr["off"][b]), int(pr["n"][b])
        assert np.array_equal(got["keep"][o:o + n], c["keep"])


def test_a_line_needs_few_rounds(hand_first):
    """a chain of 2998 points in shuffled order: the component search is logarithmic in its length, where minimum-label propagation would need thousands of rounds"""
    pr, got = hand_first
    names = list(HAND)
    # on a chain a root that does not hook is a local minimum among its two neighbour components and no two neighbours are both: k roots become at most
    # ceil(k / 2) per round, so ceil(log2 n) rounds join n points and one more finds nothing to hook
    for name, n in (("line_70_shuffled", 70), ("line_300_shuffled", 300), ("n3000_test7", 3000)):
        rounds = int(got["results"][names.index(name)]["rounds"])
        print(name, rounds)
        assert 1 <= rounds <= int(np.ceil(np.log2(n))) + 1, (name, rounds)


@pytest.mark.parametrize("mode", [omc.MODE_UPDATE, omc.MODE_NEW_OBJECT])
def test_generated_problems(handle, mode):
    ps = omc.generated(mode)
    pr, got = _run(handle, ps)
    _check(pr, got, ps, _answers(ps))


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(9)
    ok = lambda n: (np.full(n, 3, np.int32), np.full(n, 4, np.int32))
    ps = [dict(HAND["n3000_test7"]), dict(pos=omc.blob_3000()[rng.permutation(3000)], mode=omc.MODE_UPDATE), dict(HAND["n3001_test5"])]
    ps[1]["cnt"], ps[1]["total"] = ok(3000)
    return ps, _answers(ps)


def test_three_large_problems_in_one_batch(handle, big):
    ps, answers = big
    pr, got = _run(handle, ps)
    _check(pr, got, ps, answers)
    assert [int(r["path"]) for r in got["results"]] == [omc.PATH_TEST7, omc.PATH_TEST7, omc.PATH_TEST5]
    # any graph: a root that does not hook is a local minimum, all of whose neighbours hook onto labels below its own, so it hooks in the next round: the roots at
    # least halve every two rounds, 2 * ceil(log2 3000) + 1 = 25
    assert got["results"][1]["rounds"] <= 25


def test_problems_are_independent_and_calls_repeat(handle, hand_first):
    pr, got = hand_first
    ps = list(HAND.values())
    again = _run(handle, ps)[1]
    assert all(again[k].tobytes() == got[k].tobytes() for k in ("keep", "cluster", "results"))
    order = list(range(len(ps)))[::-1]
    pr2, rev = _run(handle, [ps[b] for b in order], gap=1)
    for b2, b in enumerate(order):
        o, o2, n = int(pr["off"][b]), int(pr2["off"][b2]), int(pr["n"][b])
        assert rev["keep"][o2:o2 + n].tobytes() == got["keep"][o:o + n].tobytes() and rev["cluster"][o2:o2 + n].tobytes() == got["cluster"][o:o + n].tobytes()
        assert rev["results"][b2].tobytes() == got["results"][b].tobytes()
    alone = _run(handle, [ps[5]])[1]
    assert alone["results"][0].tobytes() == got["results"][5].tobytes()


def test_host_and_device_entry_points_agree(handle, hand_first):
    dev = _run(handle, list(HAND.values()), device=True)[1]
    assert all(dev[k].tobytes() == hand_first[1][k].tobytes() for k in ("keep", "cluster", "results"))


def test_center_and_size_parity(handle):
    ps = omc.generated(omc.MODE_UPDATE, seed=21) + [dict(HAND["n3001_test5"]), dict(HAND["nan_coordinate"])]
    pr, pos, _, _ = _batch(ps)
    fill = om.new_results(1, FILL)[0]
    outs = []
    for device in (False, True):
        res = handle.center_and_size(pr, pos, results=om.new_results(len(ps), FILL), device=device)["results"]
        outs.append(res.tobytes())
        for b, p in enumerate(ps):
            center, bbox = omc.center_and_size(p["pos"])
            assert res[b]["status"] == om.DONE and res[b]["n_kept"] == len(p["pos"])
            _check_extent(res[b], center, bbox, fill)
            for k in ("n_candidates", "n_clusters", "path", "rounds", "std_dev", "candidates_center"):   # not this operator's
                assert res[b][k].tobytes() == fill[k].tobytes()
    assert outs[0] == outs[1]


def _merge_batch(maps, gap=2):
    offs, rows, poff, pairs = [], gap, [], 5
    for label, track, bbox in maps:
        offs.append(rows)
        poff.append(pairs)
        rows += len(label) + gap
        pairs += len(label) ** 2 + 5
    label, track, bbox = np.zeros(rows, np.int32), np.zeros(rows, np.int32), np.zeros((rows, 6), f32)
    for (l, t, bb), o in zip(maps, offs):
        n = len(l)
        label[o:o + n], track[o:o + n], bbox[o:o + n] = l, t, np.asarray(bb, f32).reshape(n, 6)
    return om.pack_merge_problems([len(m[0]) for m in maps], offs, poff), label, track, bbox, pairs


def _run_merge(h, maps, device=False):
    pr, label, track, bbox, pairs = _merge_batch(maps)
    got = h.merge_sets(pr, label, track, bbox, ratio=_filled(pairs, f32), member=_filled(pairs, np.uint8), target=_filled(len(label), np.int32), n_sets=_filled(len(maps), np.int32),
                       status=_filled(len(maps), np.int32), device=device)
    return pr, got


def _check_merge(pr, got, maps, answers):
    fill_f = _filled(1, f32)[0]
    ratio_owned, member_owned, target_owned = np.zeros(len(got["ratio"]), bool), np.zeros(len(got["member"]), bool), np.zeros(len(got["target"]), bool)
    for b, ((label, track, bbox), (ratio, sets)) in enumerate(zip(maps, answers)):
        n, po, oo = len(label), int(pr["off_pair"][b]), int(pr["off_obj"][b])
        assert got["status"][b] == om.DONE
        assert om.sets_of(got, pr, b) == sets, (b, om.sets_of(got, pr, b), sets)
        g = got["ratio"][po:po + n * n].reshape(n, n)
        iu = np.triu_indices(n, 1)
        assert np.array_equal(_bits(g[iu]), _bits(ratio[iu])), b
        mask = np.zeros((n, n), bool)
        mask[iu] = True
        ratio_owned[po:po + n * n] = mask.reshape(-1)
        member_owned[po:po + len(sets) * n] = True
        target_owned[oo:oo + len(sets)] = True
    assert (_bits(got["ratio"][~ratio_owned]) == _bits(fill_f)).all() and (got["member"][~member_owned] == FILL).all() and (got["target"][~target_owned].view(np.uint8) == FILL).all()


def test_merge_sets_hand_cases_and_generated_maps(handle):
    hand = [(np.asarray(c["label"], np.int32), np.asarray(c["track_id"], np.int32), np.asarray(c["bbox"], f32).reshape(-1, 6)) for c in MERGE.values()]
    maps = hand + omc.generated_maps()
    answers = [omc.merge_sets(*m) for m in maps]
    pr, got = _run_merge(handle, maps)
    _check_merge(pr, got, maps, answers)
    for b, c in enumerate(MERGE.values()):
        assert om.sets_of(got, pr, b) == c["sets"]
    assert max(len(a[1]) for a in answers) >= 2
    dev = _run_merge(handle, maps, device=True)[1]
    again = _run_merge(handle, maps)[1]
    assert all(dev[k].tobytes() == got[k].tobytes() and again[k].tobytes() == got[k].tobytes() for k in got)
    alone = _run_merge(handle, [maps[1]])
    assert om.sets_of(alone[1], alone[0], 0) == answers[1][1]


def test_reject_outliers_chains_into_merge_sets_on_one_stream(handle):
    """the result records of a rejection stay on the device and their bbox members are the rows of oslam_objmap_merge_sets_device on the same stream"""
    import torch
    from object_slam_amd._lib import upload
    rng = np.random.default_rng(31)
    ps = []
    for k in range(6):   # six objects, two by two on the same site: their boxes overlap
        pos = (rng.uniform(0, 0.4, (40, 3)) + [1.5 * (k // 2), 0, 0]).astype(f32)
        ps.append(dict(pos=pos, cnt=np.full(40, 3, np.int32), total=np.full(40, 4, np.int32), mode=omc.MODE_UPDATE))
    pr, pos, cnt, total = _batch(ps, gap=0)
    host = handle.reject_outliers(pr, pos, cnt, total)
    label, track = np.ones(6, np.int32), np.arange(6, dtype=np.int32) + 3
    mp = om.pack_merge_problems([6])
    want = handle.merge_sets(mp, label, track, host["results"]["bbox"])
    assert want["n_sets"][0] == 3 and om.sets_of(want, mp, 0) == [([0, 1], 1), ([2, 3], 3), ([4, 5], 5)]
    ins = dict(pr=pr, pos=pos, cnt=cnt, total=total, keep=np.zeros(len(pos), np.uint8), cluster=np.zeros(len(pos), np.int32), res=om.new_results(6), mp=mp, label=label, track=track,
               ratio=_filled(36, f32), member=_filled(36, np.uint8), target=_filled(6, np.int32), ns=_filled(1, np.int32), st=_filled(1, np.int32))
    t = {k: upload(v) for k, v in ins.items()}
    a = lambda k, off=0: t[k].data_ptr() + off
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    stream = C.c_void_p(side.cuda_stream)
    with torch.cuda.stream(side):
        check(handle.L.oslam_objmap_reject_outliers_device(handle.h, 6, a("pr"), len(pos), a("pos"), a("cnt"), a("total"), a("keep"), a("cluster"), a("res"), stream))
        check(handle.L.oslam_objmap_merge_sets_device(handle.h, 1, a("mp"), 6, a("label"), a("track"), a("res", om.RESULT_BBOX_OFFSET), om.RESULT_DTYPE.itemsize // 4, 36, a("ratio"),
                                                      a("member"), a("target"), a("ns"), a("st"), stream))
    side.synchronize()
    back = lambda k: t[k].cpu().numpy()[:ins[k].nbytes].view(ins[k].dtype).reshape(ins[k].shape)
    assert back("res").tobytes() == host["results"].tobytes() and back("keep").tobytes() == host["keep"].tobytes()
    got = dict(ratio=back("ratio"), member=back("member"), target=back("target"), n_sets=back("ns"), status=back("st"))
    assert om.sets_of(got, mp, 0) == om.sets_of(want, mp, 0) and got["status"][0] == om.DONE
    iu = np.triu_indices(6, 1)
    assert np.array_equal(_bits(got["ratio"].reshape(6, 6)[iu]), _bits(want["ratio"].reshape(6, 6)[iu]))


def _refused(code, fn, *args, **kw):
    with pytest.raises(OslamError) as ei:
        fn(*args, **kw)
    assert ei.value.code == code, ei.value


def test_refusals_launch_nothing(handle):
    pos = np.zeros((3100, 3), f32)
    cnt, total = np.full(3100, 3, np.int32), np.full(3100, 4, np.int32)
    keep = _filled(3100, np.uint8)

    def call(pr, **kw):
        return handle.reject_outliers(pr, pos, cnt, total, keep=keep, **kw)
    _refused(OSLAM_E_CAPACITY, call, om.pack_problems([3001], om.MODE_NEW_OBJECT))           # a clustering problem above max_cluster_points
    _refused(OSLAM_E_CAPACITY, call, om.pack_problems([1] * 1025))                             # above max_problems
    _refused(OSLAM_E_INVALID, call, om.pack_problems([-1]))
    _refused(OSLAM_E_INVALID, call, om.pack_problems([4], 2))                                  # an unknown mode
    _refused(OSLAM_E_INVALID, call, om.pack_problems([4], off=[3097]))                         # rows outside the arrays
    _refused(OSLAM_E_INVALID, call, om.pack_problems([4], off=[-1]))
    assert (keep == FILL).all()
    L, h = handle.L, handle.h
    pr, res = om.pack_problems([4]), om.new_results(1)
    p = lambda x: C.c_void_p(x.__array_interface__["data"][0])
    clu = np.zeros(3100, np.int32)
    for args in ((None, 3100, p(pos), p(cnt), p(total), p(keep), p(clu), p(res)), (p(pr), 3100, None, p(cnt), p(total), p(keep), p(clu), p(res)),
                 (p(pr), 3100, p(pos), None, p(total), p(keep), p(clu), p(res)), (p(pr), 3100, p(pos), p(cnt), p(total), None, p(clu), p(res)),
                 (p(pr), 3100, p(pos), p(cnt), p(total), p(keep), p(clu), None)):
        assert L.oslam_objmap_reject_outliers(h, 1, *args) == OSLAM_E_INVALID
    assert L.oslam_objmap_reject_outliers(None, 1, p(pr), 3100, p(pos), p(cnt), p(total), p(keep), p(clu), p(res)) == OSLAM_E_INVALID
    assert L.oslam_objmap_center_and_size(h, 1, p(pr), 3100, None, p(res)) == OSLAM_E_INVALID
    assert L.oslam_objmap_reject_outliers(h, 1, p(pr), -1, p(pos), p(cnt), p(total), p(keep), p(clu), p(res)) == OSLAM_E_CAPACITY
    # mode NEW_OBJECT alone needs no label arrays
    out = handle.reject_outliers(om.pack_problems([6], om.MODE_NEW_OBJECT), omc.NEW6)
    assert out["results"][0]["path"] == om.PATH_SHORTCUT and out["keep"].tolist() == [1] * 6
    # merge sets
    label, track, bbox = np.zeros(130, np.int32), np.arange(130, dtype=np.int32), np.zeros((130, 6), f32)
    _refused(OSLAM_E_CAPACITY, handle.merge_sets, om.pack_merge_problems([129]), label, track, bbox)
    _refused(OSLAM_E_INVALID, handle.merge_sets, om.pack_merge_problems([-1]), label, track, bbox, n_pairs=4)
    _refused(OSLAM_E_INVALID, handle.merge_sets, om.pack_merge_problems([4], off_obj=[127]), label, track, bbox)
    _refused(OSLAM_E_INVALID, handle.merge_sets, om.pack_merge_problems([4]), label, track, bbox, n_pairs=15)
    for bad in ((1, 2999, 128), (1, 4001, 128), (1, 3000, 129), (0, 3000, 128)):
        _refused(OSLAM_E_INVALID, om.ObjectMap, *bad)


def test_device_entry_points_refuse_per_problem(handle):
    """the device entry points cannot read the records: a problem that does not fit gets a negative status and nothing else of it is written; its neighbours are served"""
    good = HAND["two_blobs_and_a_bridge"]
    ps = [good, dict(pos=np.zeros((3001, 3), f32), cnt=np.ones(3001, np.int32), total=np.ones(3001, np.int32), mode=omc.MODE_NEW_OBJECT), good]
    pr, pos, cnt, total = _batch(ps)
    pr = np.concatenate([pr, om.pack_problems([4, 4], [7, omc.MODE_UPDATE], [0, len(pos) - 2])])   # an unknown mode; rows past the end
    got = handle.reject_outliers(pr, pos, cnt, total, keep=_filled(len(pos), np.uint8), cluster=_filled(len(pos), np.int32), results=om.new_results(5, FILL), device=True)
    assert got["results"]["status"].tolist() == [om.DONE, om.REFUSED_CAPACITY, om.DONE, om.REFUSED_RECORD, om.REFUSED_RECORD]
    want = omc.reject_outliers(good["pos"], good["cnt"], good["total"], good["mode"])
    for b in (0, 2):
        o = int(pr["off"][b])
        assert np.array_equal(got["keep"][o:o + 7], want["keep"]) and got["results"][b]["n_kept"] == 7
    o = int(pr["off"][1])
    assert (got["keep"][o:o + 3001] == FILL).all() and (got["keep"][:GAP] == FILL).all()
    fill = om.new_results(1, FILL)[0]
    for b in (1, 3, 4):
        assert got["results"][b]["n_kept"] == fill["n_kept"] and got["results"][b]["center"].tobytes() == fill["center"].tobytes()
    label, track, bbox = np.zeros(130, np.int32), np.arange(130, dtype=np.int32), np.zeros((130, 6), f32)
    mp = om.pack_merge_problems([129, 2, 3], off_obj=[0, 0, 129], off_pair=[0, 0, 0])
    out = handle.merge_sets(mp, label, track, bbox, n_pairs=129 * 129, device=True)
    assert out["status"].tolist() == [om.REFUSED_CAPACITY, om.DONE, om.REFUSED_RECORD]


def test_timing_gives_kernel_milliseconds(handle):
    handle.set_timing(True)
    try:
        c = HAND["line_300_shuffled"]
        handle.reject_outliers(om.pack_problems([300]), c["pos"], c["cnt"], c["total"])
        assert handle.last_kernel_ms() > 0
    finally:
        handle.set_timing(False)


def test_adapter_program_matches_the_restatement(tmp_path):
    from object_slam_amd import build
    build.build_hip()
    prog = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adapter_object_map_program.cc"), "-o", prog,
                           "-L", LIBDIR, "-loslam_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    points, frames = omc.fixture_scene()
    want = omc.run_fixture(points, frames)
    path = str(tmp_path / "scene.txt")
    omc.write_fixture(path, points, frames)
    r = subprocess.run([prog, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = r.stdout.strip().split("\n")
    print("\n".join(got))
    assert got == want
