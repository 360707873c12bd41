"""CPU: the batch-of-sequences tracking + local-mapping driver (include/oslam_slam.h) run over the oracle's operator table:
control flow, map bookkeeping invariants, trajectory accuracy, determinism, independence of the sequences in a batch.
(The HIP operator table is compared with this one in tests/test_slam_driver_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest

from object_slam_amd import slam
from slam_common import H, W, ate, make_streams, oracle_ops, run


def test_create_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from object_slam_amd import OslamError
    with pytest.raises(OslamError) as ei:
        slam.System(slam.make_config(W, H, 1))
    assert "no CPU fallback" in str(ei.value)


def test_driver_tracks_and_maps(oracle):
    n = 36
    cfg = slam.make_config(W, H, 1)
    streams = make_streams(1, n)
    sysm = slam.System(cfg, oracle_ops(cfg))
    poses, states = run(sysm, streams, n)
    assert (states == slam.OK).all()
    st = sysm.stats(0)
    assert st["frames"] == n and st["lost_frames"] == 0 and st["map_violations"] == 0
    # frame 1 has no motion model yet: TrackReferenceKeyFrame (reference src/Tracking.cc:358-361); the rest use the motion model
    assert st["tracked_reference_kf"] == 1 and st["tracked_motion_model"] == n - 2
    assert st["keyframes_created"] >= 4 and st["local_bas"] >= 2 and st["points_fused"] > 0 and st["points_culled"] > 0
    a, Twc = ate(sysm, cfg, streams, 0)
    assert a < 0.01, a          # metres over a ~1.5 m path, scene at 2 m
    # fronto-parallel translation: rotation stays at identity
    assert np.abs(Twc[:, :, :3] - np.eye(3)).max() < 1e-2
    kst, kT = sysm.keyframe_trajectory(0)
    assert len(kst) == st["keyframes_in_map"]


def test_driver_is_deterministic_and_sequences_are_independent(oracle):
    n = 14
    streams = make_streams(2, n)
    cfg2 = slam.make_config(W, H, 2, host_threads=4)   # worker pool on: results must not depend on it
    s2 = slam.System(cfg2, oracle_ops(cfg2))
    p2, _ = run(s2, streams, n)
    for s in range(2):
        cfg1 = slam.make_config(W, H, 1)
        s1 = slam.System(cfg1, oracle_ops(cfg1))
        p1, _ = run(s1, [streams[s]], n)
        assert np.array_equal(p1[:, 0], p2[:, s])
        assert s1.stats(0) == s2.stats(s)


def test_local_mapping_switches(oracle):
    """Tracking only + LBA (no culling / fusion / triangulation) still tracks; the map then only grows."""
    n = 16
    cfg = slam.make_config(W, H, 1, local_mapping=0x8)
    streams = make_streams(1, n)
    sysm = slam.System(cfg, oracle_ops(cfg))
    run(sysm, streams, n)
    st = sysm.stats(0)
    assert st["points_culled"] == 0 and st["points_fused"] == 0 and st["points_triangulated"] == 0 and st["keyframes_culled"] == 0
    assert st["local_bas"] >= 1 and st["map_violations"] == 0
    a, _ = ate(sysm, cfg, streams, 0)
    assert a < 0.01


def test_stereo_driver_kitti_shape(oracle):
    """STEREO sensor on a KITTI-shaped pair stream (1241x376, 2000 features, KITTI00-02.yaml calibration): Frame::ComputeStereoMatches
    feeds the same tracking / mapping flow with the stereo thresholds (th = 7 / 1, outliers dropped in TrackLocalMap)."""
    from slam_common import ate_stereo, make_stereo_streams, run_stereo, stereo_config
    n = 10
    cfg = stereo_config(1)
    streams = make_stereo_streams(1, n)
    sysm = slam.System(cfg, oracle_ops(cfg))
    poses, states = run_stereo(sysm, streams, n)
    assert (states == slam.OK).all()
    st = sysm.stats(0)
    assert st["lost_frames"] == 0 and st["map_violations"] == 0 and st["points_created"] > 1000
    a, _ = ate_stereo(sysm, cfg, streams, 0)
    assert a < 0.05, a          # metres; plane at 12 m, 1.7 cm per pixel


def test_map_bookkeeping_unit_checks(tmp_path):
    """tests/slam_map_check.cc: covisibility weights / ordering, spanning tree, Observations() accounting, EraseObservation, Replace and
    KeyFrame::SetBadFlag of csrc/slam_map.h on a hand-built map (host C++, no GPU, no oracle)."""
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "slam_map_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(here, "slam_map_check.cc"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


@pytest.mark.parametrize("lm", [slam.LM_SYNC, slam.LM_DEFERRED], ids=["sync", "deferred"])
def test_not_initialised_lost_and_reset(oracle, lm):
    """A textureless first frame leaves the sequence NOT_INITIALIZED (StereoInitialization needs > 500 keypoints, reference
    src/Tracking.cc:592).  Losing the track with <= 5 keyframes resets the system (:553-561): the next textured frame initialises a new
    map whose ids restart at 0.  The independent restatement goes through the same states with the same poses."""
    from oracle import slam_driver_oracle as R
    cfg = slam.make_config(W, H, 1, local_mapping=lm)
    streams = make_streams(1, 12)
    blank = np.full((H, W), 90, np.uint8)
    seq = [blank] + list(streams[0][0][:6]) + [blank, blank] + list(streams[0][0][6:10])
    depth = np.full((H, W), 2.0, np.float32)
    sysm = slam.System(cfg, oracle_ops(cfg))
    ref = R.Slam(_cfg_dict(cfg))
    states = []
    for t, img in enumerate(seq):
        T, st = sysm.TrackRGBD([img], [depth], [t / 30.0])
        Tr, sr = ref.Track((img, depth), t / 30.0)
        states.append(int(st[0]))
        assert int(st[0]) == sr, t
        if Tr is not None:
            assert np.array_equal(T[0], Tr), t
    assert states[0] == slam.NOT_INITIALIZED
    assert states[1:7] == [slam.OK] * 6
    assert states[7] == slam.LOST                      # lost with <= 5 keyframes -> reset requested
    assert states[8] == slam.NOT_INITIALIZED           # reset applied, textureless frame cannot initialise
    assert states[9:] == [slam.OK] * 4                 # new map
    st = sysm.stats(0)
    assert st["lost_frames"] == 1 and st["map_violations"] == 0 and st["keyframes_in_map"] >= 1
    stamps, Twc = sysm.trajectory(0)
    assert len(stamps) == 4                            # the trajectory of the new map only (mlRelativeFramePoses was cleared)
    assert np.array_equal(Twc[0], np.eye(4, dtype=np.float32)[:3])
    tr = ref.trajectory()
    assert len(tr) == 4 and np.array_equal(Twc, np.stack([x[1] for x in tr]))


def _cfg_dict(cfg):
    return dict(width=cfg.width, height=cfg.height, fx=cfg.fx, fy=cfg.fy, cx=cfg.cx, cy=cfg.cy, bf=cfg.bf, thDepth=cfg.thDepth, fps=cfg.fps,
                nFeatures=cfg.nFeatures, scaleFactor=cfg.scaleFactor, nLevels=cfg.nLevels, iniThFAST=cfg.iniThFAST, minThFAST=cfg.minThFAST,
                sensor=cfg.sensor, local_mapping=cfg.local_mapping)


@pytest.mark.parametrize("lm", [slam.LM_SYNC, slam.LM_DEFERRED], ids=["sync", "deferred"])
def test_driver_against_independent_restatement(oracle, lm):
    """The product's driver (index-based, staged, C++) against oracle/slam_driver_oracle.py (object-style Python restatement of the
    reference's Tracking / LocalMapping flow), both over the CPU oracle operators: same states, same map statistics, same poses."""
    from oracle import slam_driver_oracle as R
    n = 26
    cfg = slam.make_config(W, H, 1, local_mapping=lm)
    streams = make_streams(1, n)
    depth = np.full((H, W), 2.0, np.float32)
    sysm = slam.System(cfg, oracle_ops(cfg))
    ref = R.Slam(_cfg_dict(cfg))
    for t in range(n):
        img = streams[0][0][t]
        T, st = sysm.TrackRGBD([img], [depth], [t / 30.0])
        Tr, sr = ref.Track((img, depth), t / 30.0)
        assert int(st[0]) == sr, t
        assert np.array_equal(T[0], Tr), (t, np.abs(T[0] - Tr).max())
        a, b = sysm.stats(0), ref.stats()
        assert all(a[k] == b[k] for k in b), (t, a, b)
    assert sysm.stats(0)["keyframes_created"] >= 4 and sysm.stats(0)["points_fused"] > 0 and sysm.stats(0)["points_triangulated"] > 0
    stamps, Twc = sysm.trajectory(0)
    tr = ref.trajectory()
    assert len(tr) == len(stamps)
    assert np.array_equal(Twc, np.stack([x[1] for x in tr]))


@pytest.mark.parametrize("lm", [slam.LM_SYNC, slam.LM_DEFERRED], ids=["sync", "deferred"])
def test_keyframe_culling_against_independent_restatement(oracle, lm):
    """A stream with foreign texture over half of every second frame makes the tracker insert keyframes in mapped territory, so
    LocalMapping::KeyFrameCulling (reference src/LocalMapping.cc:638-713) removes redundant ones: both drivers must take the same
    decisions (the culled keyframes change covisibility, the spanning tree, the local map and the trajectory anchors)."""
    from oracle import slam_driver_oracle as R
    from object_slam_amd import synth
    n = 54
    cfg = slam.make_config(W, H, 1, local_mapping=lm)
    frames, _ = synth.make_occluded_stream(n, W, H, seed=11)
    depth = np.full((H, W), 2.0, np.float32)
    sysm = slam.System(cfg, oracle_ops(cfg))
    ref = R.Slam(_cfg_dict(cfg))
    for t in range(n):
        T, st = sysm.TrackRGBD([frames[t]], [depth], [t / 30.0])
        Tr, sr = ref.Track((frames[t], depth), t / 30.0)
        assert int(st[0]) == sr, t
        assert np.array_equal(T[0], Tr), (t, np.abs(T[0] - Tr).max())
        a, b = sysm.stats(0), ref.stats()
        assert all(a[k] == b[k] for k in b), (t, a, b)
    a = sysm.stats(0)
    assert a["keyframes_culled"] >= 2 and a["keyframes_in_map"] == a["keyframes_created"] - a["keyframes_culled"] and a["map_violations"] == 0, a
    stamps, Twc = sysm.trajectory(0)
    tr = ref.trajectory()
    assert len(tr) == len(stamps) == n
    assert np.array_equal(Twc, np.stack([x[1] for x in tr]))
    sk, Tk = sysm.keyframe_trajectory(0)
    assert len(sk) == a["keyframes_in_map"]
    # observations that survive in culled keyframes are left out of ComputeDistinctiveDescriptors (src/MapPoint.cc:366) by both drivers
    assert sysm.bad_keyframe_observations() <= getattr(ref, "bad_kf_observations", 0)
    print("observations in culled keyframes skipped:", sysm.bad_keyframe_observations())


def test_stereo_driver_against_independent_restatement(oracle):
    from oracle import slam_driver_oracle as R
    from slam_common import make_stereo_streams, stereo_config
    n = 14
    cfg = stereo_config(1)
    streams = make_stereo_streams(1, n)
    sysm = slam.System(cfg, oracle_ops(cfg))
    ref = R.Slam(_cfg_dict(cfg))
    for t in range(n):
        T, st = sysm.TrackStereo([streams[0][0][t]], [streams[0][1][t]], [t / 10.0])
        Tr, sr = ref.Track((streams[0][0][t], streams[0][1][t]), t / 10.0)
        assert int(st[0]) == sr and np.array_equal(T[0], Tr), t
        a, b = sysm.stats(0), ref.stats()
        assert all(a[k] == b[k] for k in b), (t, a, b)
    assert sysm.stats(0)["keyframes_created"] >= 2


def test_semantic_tracking_against_independent_restatement(oracle):
    """BASELINE.json configs[2] shape: S1 scene with three box objects and their instance masks.  Frame::BuildObject2DsRGBD, the Object3D lists and
    ObjectOptimizer::PoseOptimization2 in TrackLocalMap (reference src/Tracking.cc:1022) — C++ driver against the Python restatement, and against a
    run without masks (the semantic edges must change the trajectory)."""
    from oracle import slam_driver_oracle as R
    from slam_common import make_scene_streams
    n = 16
    q = make_scene_streams(1, n)[0]
    cfg = slam.make_config(W, H, 1)
    sysm = slam.System(cfg, oracle_ops(cfg))
    ref = R.Slam(_cfg_dict(cfg))
    plain = slam.System(slam.make_config(W, H, 1), oracle_ops(cfg))
    diff = 0.0
    for t in range(n):
        objs = dict(masks=[q["masks"][t, o] for o in range(3)], track_ids=q["track_ids"])
        T, st = sysm.TrackRGBD([q["gray"][t]], [q["depth"][t]], [t / 30.0], objects=[objs])
        Tr, sr = ref.Track((q["gray"][t], q["depth"][t]), t / 30.0, objects=objs)
        Tp, _ = plain.TrackRGBD([q["gray"][t]], [q["depth"][t]], [t / 30.0])
        assert int(st[0]) == sr == slam.OK, t
        assert np.array_equal(T[0], Tr), (t, np.abs(T[0] - Tr).max())
        a, b = sysm.stats(0), ref.stats()
        assert all(a[k] == b[k] for k in b), (t, a, b)
        diff = max(diff, float(np.abs(T[0] - Tp[0]).max()))
    a = sysm.stats(0)
    # frames 0 (initialisation) and 1 (no Object3D yet) carry no semantic edges; every later tracked frame does
    assert a["object3ds"] == 3 and a["semantic_frames"] == n - 2 and a["semantic_frames_nonzero"] == n - 2 and a["semantic_edges"] > 100 * (n - 2), a
    assert a["object2ds"] == 3 * n
    assert diff > 1e-5, diff
    assert plain.stats(0)["semantic_edges"] == 0


def test_observations_in_culled_keyframes_against_independent_restatement(oracle):
    """MapPoint::ComputeDistinctiveDescriptors skips observations whose keyframe is bad (reference src/MapPoint.cc:366) while UpdateNormalAndDepth reads
    all of them (:441-453).  Such observations exist: two new points triangulated against the same neighbour keypoint both observe it, the keypoint's slot
    belongs to the second (src/LocalMapping.cc:440-446), and KeyFrame::SetBadFlag later erases only the observations of the keyframe's own mvpMapPoints.
    On this 3-D scene stream the case occurs from frame 103 on: the C++ driver and the independent restatement must count the same skipped observations
    and stay bit-identical through it."""
    from oracle import slam_driver_oracle as R
    from object_slam_amd import scene
    n = 108
    q = scene.make_rgbd_sequence(2, n, speed=2.0, with_masks=False)
    cfg = slam.make_config(W, H, 1)
    sysm = slam.System(cfg, oracle_ops(cfg))
    ref = R.Slam(_cfg_dict(cfg))
    for t in range(n):
        T, st = sysm.TrackRGBD([q["gray"][t]], [q["depth"][t]], [t / 30.0])
        Tr, sr = ref.Track((q["gray"][t], q["depth"][t]), t / 30.0)
        assert int(st[0]) == sr, t
        assert np.array_equal(T[0], Tr), (t, np.abs(T[0] - Tr).max())
    a, b = sysm.stats(0), ref.stats()
    assert all(a[k] == b[k] for k in b), (a, b)
    assert a["keyframes_culled"] >= 1 and a["map_violations"] == 0
    # (the driver does not repeat an update whose inputs cannot have changed within a local-mapping pass, the restatement repeats it like the reference:
    # the counts are per ComputeDistinctiveDescriptors call, so the driver's is the smaller one; the poses and statistics above are identical)
    nb, nr = sysm.bad_keyframe_observations(), getattr(ref, "bad_kf_observations", 0)
    assert 0 < nb <= nr, (nb, nr)


def test_local_ba_window_beyond_the_operator_bound_is_degraded_not_skipped(oracle):
    """The local-BA operator solves at most 128 FREE keyframes per window (the reference has no bound, src/Optimizer.cc:456-468).  A window beyond the bound is
    kept: the current keyframe and its strongest covisible keyframes stay free, the weaker local keyframes enter as fixed cameras.  OSLAM_SLAM_LBA_MAX_FREE lowers
    the bound to 3 (read when the library is loaded, hence the child process) so that the 36-frame stream reaches it: local BA still runs on every keyframe,
    the map stays consistent and the trajectory accurate, and the degraded windows are counted."""
    import os
    import subprocess
    import sys
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
from object_slam_amd import slam
from slam_common import H, W, ate, make_streams, oracle_ops, run
n = 36
cfg = slam.make_config(W, H, 1)
streams = make_streams(1, n)
sysm = slam.System(cfg, oracle_ops(cfg))
poses, states = run(sysm, streams, n)
st, w = sysm.stats(0), sysm.lba_window_stats(0)
a, _ = ate(sysm, cfg, streams, 0)
assert (states == slam.OK).all() and st["lost_frames"] == 0 and st["map_violations"] == 0, st
assert st["local_bas"] >= 2 and w["windows"] == st["local_bas"], (st, w)
assert w["lba_windows_degraded"] >= 1, w
assert a < 0.01, a
print("degraded", w["lba_windows_degraded"], "of", w["windows"], "ate", a)
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OSLAM_SLAM_LBA_MAX_FREE="3"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "degraded" in r.stdout


def test_deferred_schedule_differs_from_the_synchronous_one_only_by_when_the_ba_lands(oracle):
    """OSLAM_SLAM_LM_DEFERRED (include/oslam_slam.h head comment): local BA's write-back and KeyFrameCulling of keyframe t are applied after the tracking of
    frame t+1.  The frame that follows a keyframe therefore tracks against the un-refined map — its pose differs from the synchronous run's by what the BA
    would have moved — while the trajectory stays as accurate; the first pass (two keyframes: no BA, nothing to cull) is identical; oslam_slam_finish applies
    the last pass, so both runs end with the same number of local BAs."""
    n = 36
    streams = make_streams(1, n)
    out = {}
    for lm in (slam.LM_SYNC, slam.LM_DEFERRED):
        cfg = slam.make_config(W, H, 1, local_mapping=lm)
        sysm = slam.System(cfg, oracle_ops(cfg))
        poses, states = run(sysm, streams, n)
        assert (states == slam.OK).all()
        a, _ = ate(sysm, cfg, streams, 0)      # (trajectory() finishes the pending pass)
        out[lm] = (poses, sysm.stats(0), a)
        assert out[lm][1]["map_violations"] == 0 and a < 0.01, (lm, a)
    ps, pd = out[slam.LM_SYNC][0], out[slam.LM_DEFERRED][0]
    first_diff = next(t for t in range(n) if not np.array_equal(ps[t], pd[t]))
    assert first_diff >= 2                      # frames 0-1 never differ: the first BA needs three keyframes in the map
    assert np.abs(ps - pd).max() < 5e-3         # the same trajectory up to what one BA moves
    assert out[slam.LM_SYNC][1]["local_bas"] >= 2 and out[slam.LM_DEFERRED][1]["local_bas"] >= 2


def test_threaded_oracle_table_equals_the_plain_one_under_the_deferred_schedule(oracle):
    """bench.py's two-thread CPU baseline (oracle/slam_ops_oracle.cc oo_slam_make_ops_threaded: the local BA of keyframe t on a second thread while frame t + 1
    is tracked, the reference's LocalMapping thread, src/System.cc:95) produces the poses and statistics of the plain table under the same schedule."""
    from oracle import oracle_py as O
    n = 26
    streams = make_streams(1, n)
    out = []
    for maker in ("oo_slam_make_ops", "oo_slam_make_ops_threaded"):
        cfg = slam.make_config(W, H, 1, local_mapping=slam.LM_DEFERRED)
        ops = slam.SlamOps()
        assert getattr(O.lib(), maker)(C.byref(cfg), C.byref(ops)) == 0
        sysm = slam.System(cfg, ops)
        poses, states = run(sysm, streams, n)
        sysm.finish()
        out.append((poses, states, sysm.stats(0)))
        sysm.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    assert out[0][2]["local_bas"] >= 2


@pytest.mark.parametrize("tag,lm", [("sync", slam.LM_SYNC), ("deferred", slam.LM_DEFERRED)])
def test_golden_driver_fixture_equals_the_cpp_driver_over_the_oracle_table(oracle, tag, lm):
    """tests/golden/driver_rgbd_*.npz (oracle/slam_driver_oracle.py, the Python restatement: tests/golden/gen_driver_golden.py) is what the GPU suite compares the
    HIP path with; here the product's C++ driver over the CPU oracle's operators must reproduce it bit for bit — the fixture is current and the two drivers agree."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "driver_rgbd_%s.npz" % tag))
    n = int(g["n"])
    streams = make_streams(1, n)
    depth = np.full((H, W), 2.0, np.float32)
    cfg = slam.make_config(W, H, 1, local_mapping=lm)
    sysm = slam.System(cfg, oracle_ops(cfg))
    keys = [str(k) for k in g["stat_keys"]]
    for t in range(n):
        T, st = sysm.TrackRGBD([streams[0][0][t]], [depth], [t / 30.0])
        assert int(st[0]) == int(g["states"][t]) and np.array_equal(T[0], g["poses"][t]), t
        s = sysm.stats(0)
        assert [int(s[k]) for k in keys] == [int(v) for v in g["stats"][t]], t
    sysm.finish()
    _, Twc = sysm.trajectory(0)
    assert np.array_equal(Twc, g["trajectory"])


def test_create_new_map_points_in_one_batch_equals_the_neighbour_rounds(oracle, monkeypatch):
    """CPU twin of the test of the same name in tests/test_slam_driver_gpu.py, over the oracle's operator table: CreateNewMapPoints as one batch over all neighbours
    (skip test at application time) and as one lockstep round per neighbour (OSLAM_SLAM_CNMP_ROUNDS=1, read per pass) build their jobs and apply their points through
    the same code and must give the same points in the same order.  9 frames is the shortest make_scene_streams length at which both sequences have triangulated
    (4 and 12 points; at 8 frames sequence 0 has none)."""
    from slam_common import make_scene_streams, run_scene
    n, S = 9, 2
    seqs = make_scene_streams(S, n)
    cfg = slam.make_config(W, H, S)
    a = slam.System(cfg, oracle_ops(cfg))
    pa, sa = run_scene(a, seqs, n)
    monkeypatch.setenv("OSLAM_SLAM_CNMP_ROUNDS", "1")
    b = slam.System(cfg, oracle_ops(cfg))
    pb, sb = run_scene(b, seqs, n)
    assert np.array_equal(sa, sb) and np.array_equal(pa, pb)
    for q in range(S):
        st = a.stats(q)
        assert st == b.stats(q) and st["points_triangulated"] > 0, st


def test_tracking_entry_points_refuse_bad_calls_with_their_codes_and_messages(oracle):
    """Every refusal of the six oslam_slam_track_* entry points (include/oslam_slam.h), by return code and oslam_last_error() text: NULL handle or image arrays,
    the wrong sensor kind, a table without frames_stereo / frames_rgbd_raw16, the mask_stride rules and the one-bit-mask rule of raw16 — in the order the checks
    are made — on one RGB-D and one STEREO handle with S = 1 and no frame tracked.  The oracle's table has no frames_rgbd_raw16: the raw16 rules behind that
    check are reached through a copy of the table whose entry is set (the refusals return before anything is called through it).  The refusals raised inside a
    step (too many detections, detections without masks, a table without semantic operators) take one frame of the smallest scene, of which the handles
    (a quarter of the scenes' image size, to keep Frame::Frame short) see the top left corner."""
    from object_slam_amd import scene
    L = slam.lib()
    INVALID = -1
    w2, h2 = W // 2, H // 2

    def table(sensor, **entries):
        cfg = slam.make_config(w2, h2, 1, sensor=sensor)
        ops = oracle_ops(cfg)
        for k, v in entries.items():
            setattr(ops, k, v)
        return slam.System(cfg, ops)

    rgbd, stereo = table(slam.RGBD), table(slam.STEREO)
    assert not oracle_ops(rgbd.cfg).frames_rgbd_raw16
    raw = table(slam.RGBD, frames_rgbd_raw16=oracle_ops(rgbd.cfg).frames_rgbd)
    no_stereo = table(slam.STEREO, frames_stereo=None)
    img = (C.c_void_p * 1)(1)   # a non-NULL image table: no refusal below reads through it
    objs = (slam.SlamObjects * 1)()
    out = (slam.ptr(rgbd.Tcw), slam.ptr(rgbd.state))
    i, f = C.c_int, C.c_float

    def refused(text, fn, *args):
        assert getattr(L, fn)(*args, *out) == INVALID, (fn, text)
        assert L.oslam_last_error().decode() == text, (fn, L.oslam_last_error())

    for h, a, b in ((None, img, img), (rgbd.h, None, img), (rgbd.h, img, None), (stereo.h, None, img)):   # (bad arguments come before the sensor kind)
        refused("oslam_slam_track_rgbd: bad argument", "oslam_slam_track_rgbd", h, a, i(W), b, i(W), i(0), None)
        refused("oslam_slam_track_rgbd_objects: bad argument", "oslam_slam_track_rgbd_objects", h, a, i(W), b, i(W), i(0), None, None, i(0))
        refused("oslam_slam_track_rgbd_raw16: bad argument", "oslam_slam_track_rgbd_raw16", h, a, i(W), b, i(W), f(5000), i(0), None, None, i(0))
    for h, a, b in ((None, img, img), (stereo.h, None, img), (stereo.h, img, None), (rgbd.h, img, None)):
        refused("oslam_slam_track_stereo: bad argument", "oslam_slam_track_stereo", h, a, b, i(W), i(0), None)
        refused("oslam_slam_track_stereo_objects: bad argument", "oslam_slam_track_stereo_objects", h, a, b, i(W), i(0), None, None, i(0))
    # the wrong sensor kind (before the table's entries and the mask rules), and a STEREO handle over a table without frames_stereo
    refused("oslam_slam_track_rgbd on a STEREO handle", "oslam_slam_track_rgbd", stereo.h, img, i(W), img, i(W), i(0), None)
    refused("oslam_slam_track_rgbd_objects on a STEREO handle", "oslam_slam_track_rgbd_objects", stereo.h, img, i(W), img, i(W), i(0), None, objs, i(0))
    refused("oslam_slam_track_rgbd_raw16 on a STEREO handle", "oslam_slam_track_rgbd_raw16", stereo.h, img, i(W), img, i(W), f(5000), i(0), None, objs, i(1))
    for h in (rgbd.h, no_stereo.h):
        refused("oslam_slam_track_stereo needs cfg.sensor = 1 (STEREO) and a stereo-capable operator table", "oslam_slam_track_stereo", h, img, img, i(W), i(0), None)
        refused("oslam_slam_track_stereo_objects needs cfg.sensor = 1 (STEREO) and a stereo-capable operator table", "oslam_slam_track_stereo_objects",
                h, img, img, i(W), i(0), None, objs, i(0))
    # mask_stride < width counts as soon as detections are passed, whatever their number
    refused("oslam_slam_track_rgbd_objects: mask_stride < width", "oslam_slam_track_rgbd_objects", rgbd.h, img, i(W), img, i(W), i(0), None, objs, i(w2 - 1))
    refused("oslam_slam_track_stereo_objects: mask_stride < width", "oslam_slam_track_stereo_objects", stereo.h, img, img, i(W), i(0), None, objs, i(w2 - 1))
    # raw16: the table's entry first, then mask_stride 0 (bitmaps) or >= width, then one-bit masks on the device only
    refused("oslam_slam_track_rgbd_raw16: the operator table has no frames_rgbd_raw16", "oslam_slam_track_rgbd_raw16",
            rgbd.h, img, i(W), img, i(W), f(5000), i(0), None, objs, i(1))
    for ms in (1, w2 - 1, -1):
        refused("oslam_slam_track_rgbd_raw16: mask_stride must be 0 (bitmaps) or >= width", "oslam_slam_track_rgbd_raw16",
                raw.h, img, i(W), img, i(W), f(5000), i(0), None, objs, i(ms))
    refused("oslam_slam_track_rgbd_raw16: one-bit masks must be device-accessible (on_device != 0)", "oslam_slam_track_rgbd_raw16",
            raw.h, img, i(W), img, i(W), f(5000), i(0), None, objs, i(0))
    # inside a step, after Frame::Frame: the detections of sequence 0
    q = scene.make_rgbd_sequence(0, 1, speed=2.0, with_masks=False)   # frame 0 of slam_common.make_scene_streams(1, 1); its masks are not rendered: none is read
    gp, dp = (C.c_void_p * 1)(slam.ptr(q["gray"][0]).value), (C.c_void_p * 1)(slam.ptr(q["depth"][0]).value)
    masks = (C.c_void_p * 9)(*[gp[0]] * 9)
    many, bare = (slam.SlamObjects * 1)(), (slam.SlamObjects * 1)()
    many[0].n, many[0].masks = 9, C.cast(masks, C.POINTER(C.c_void_p))
    bare[0].n = 1
    step = (gp, i(W), dp, i(W), i(0), None)
    refused("track: sequence 0 has 9 detections (max 8) or no masks", "oslam_slam_track_rgbd_objects", rgbd.h, *step, many, i(W))
    refused("track: sequence 0 has 1 detections (max 8) or no masks", "oslam_slam_track_rgbd_objects", rgbd.h, *step, bare, i(W))
    many[0].n = 8
    plain = table(slam.RGBD, object_kps=None)
    refused("track: this operator table has no semantic operators", "oslam_slam_track_rgbd_objects", plain.h, *step, many, i(W))
    assert rgbd.stats(0)["frames"] == 2 and raw.stats(0)["frames"] == 0 and stereo.stats(0)["frames"] == 0   # only the refusals inside a step began a frame
