"""CPU: the case tables of tests/mirror_common.py against the restatements of the reference's loops, a census of the gates they reach, and the model's change sets
against the driver's own (tests/slam_map_check.cc replays the same script over csrc/slam_map.h and prints Map::journal_changes's arrays) — the journals
test_mirror_cases_gpu.py feeds the device mirror are the journals the driver sends."""
import os
import subprocess

import pytest

import mirror_common as M

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def F0():
    return M.synthetic_fixtures()


@pytest.mark.parametrize("name", sorted(M.CULL_CASES))
def test_culling_case_restatement_equals_table(F0, name):
    build, gate, _ = M.CULL_CASES[name]
    m, F = M.MapModel(0), F0.fresh()
    info = build(m, F)
    want = M.cull_want(name, info)
    assert len(want) == len(info["kf"])
    for kf, w in zip(info["kf"], want):
        if w is None:
            assert kf in info["none"], (name, gate)
            continue
        assert M.cull_expected(m, kf) == w, (name, gate, kf)
        # the mirror's answer and the reference's own count differ exactly by the ambiguous points the reference counted
        usable, nMPs, nRed, red = M.cull_reference(m, kf)
        assert (usable, nMPs) == w[:2] and nRed == w[2] + len(red & M.cull_ambiguous(m, kf))


@pytest.mark.parametrize("name", sorted(M.JOURNAL_CASES))
def test_journal_case_restatement_equals_table(F0, name):
    m, F = M.MapModel(0), F0.fresh()
    sets, info = M.run_script(M.JOURNAL_CASES[name], m, F)
    assert sets
    for kf, w in zip(info["kf"], info["want"]):
        if w is not None:
            assert M.cull_expected(m, kf) == w, (name, kf)
    for kfs, w in info["lists"]:
        assert M.local_points(m, kfs) == w, (name, kfs)


@pytest.mark.parametrize("name", sorted(M.LIST_CASES))
def test_list_case_restatement_equals_table(F0, name):
    m, F = M.MapModel(0), F0.fresh()
    info = M.LIST_CASES[name](m, F)
    got = M.local_points(m, info["kfs"])
    if info["want"] is None:
        assert len(got) == info["n"] > M.STRIDE
    else:
        assert got == info["want"]
        assert len(set(got)) == len(got)


def test_first_occurrence_cases_decide_the_key_order(F0):
    """the two hand-built first-occurrence cases give ANOTHER list when the first occurrence is taken in (cell, keyframe) order instead of (keyframe, cell) order —
    `t` and `i` swapped in the key of k_fusecur_mark —, so the GPU comparison of these small lists catches that slip by itself"""
    m, F = M.MapModel(0), F0.fresh()
    info = M.LIST_CASES["first_occurrence"](m, F)
    assert M.first_occurrence_by_key(m, info["kfs"]) == info["want"] == M.local_points(m, info["kfs"])
    assert M.first_occurrence_by_key(m, info["kfs"], swapped=True) != info["want"]
    m, F = M.MapModel(0), F0.fresh()
    info = M.FUSE_CASES["basic"](m, F)
    assert M.first_occurrence_by_key(m, info["targets"]) == info["want_ids"]
    assert M.first_occurrence_by_key(m, info["targets"], swapped=True) != info["want_ids"]


@pytest.mark.parametrize("name", sorted(M.FUSE_CASES))
def test_fuse_case_restatement_equals_table(F0, name):
    m, F = M.MapModel(0), F0.fresh()
    info = M.FUSE_CASES[name](m, F)
    assert M.fuse_candidates(m, info["cur"], info["targets"]) == (info["want_ids"], info["want_excl"])


def test_census_every_gate_has_both_sides(F0):
    """every decision of the counting loop is taken both ways somewhere in the table, at every own octave the issue names, and the journal cases end on every
    (cell, holder) combination"""
    seen = set()
    own_octaves = set()
    for name, (build, _, _) in M.CULL_CASES.items():
        m, F = M.MapModel(0), F0.fresh()
        info = build(m, F)
        for kf in info["kf"]:
            if kf in info.get("none", []):
                seen.add("no_record")
                continue
            k = m.kfs[kf]
            amb = M.cull_ambiguous(m, kf)
            red = M.cull_reference(m, kf)[3]
            if all(p < 0 for p in k.mp):
                seen.add("empty_keyframe")
            for i, p in enumerate(k.mp):
                seen.add("cell_empty" if p < 0 else "cell_full")
                if p < 0:
                    continue
                seen.add("depth_usable" if k.good[i] else "depth_unusable")
                if not k.good[i]:
                    continue
                seen.add("bad" if m.isbad[p] else "not_bad")
                if m.isbad[p]:
                    continue
                seen.add("obs_gt3" if m.observations(p) > 3 else "obs_le3")
                if m.observations(p) == 3: seen.add("obs_eq3")
                if m.observations(p) == 4: seen.add("obs_eq4")
                if m.observations(p) <= 3:
                    continue
                octs = [m.kfs[a].octave[b] for a, b in m.obs[p].items() if a != kf]
                for o in octs:
                    d = o - k.octave[i]
                    seen.add("other_le" if d <= 1 else "other_gt")
                    if d == 1: seen.add(("plus1", k.octave[i]))
                    if d == 2: seen.add(("plus2", k.octave[i]))
                tot = sum(1 for a, b in m.obs[p].items() if m.kfs[a].octave[b] <= k.octave[i] + 1)
                seen.add(("total", min(tot, 4)))
                own_octaves.add(k.octave[i])
                if i in amb: seen.add("ambiguous_redundant" if i in red else "ambiguous_not_redundant")
                if tot == 3 and i not in amb: seen.add("three_own_held")
                h = m.histogram(p)
                for o in range(7):   # two full neighbouring bytes: the level mask ends between them, or behind both
                    if h[o] == 254 and h[o + 1] == 254 and k.octave[i] + 1 >= o: seen.add(("bytes_254", k.octave[i] + 1 > o))
            seen.update(("lane", i % 64) for i, p in enumerate(k.mp) if p >= 0 and k.good[i] and name == "lanes")
            if name == "lanes":
                assert {0, 63, 64, k.N - 1} <= {i for i, p in enumerate(k.mp) if p >= 0}
    need = {"no_record", "empty_keyframe", "cell_empty", "cell_full", "depth_usable", "depth_unusable", "bad", "not_bad", "obs_gt3", "obs_le3", "obs_eq3", "obs_eq4",
            "other_le", "other_gt", ("plus1", 0), ("plus2", 0), ("plus1", 5), ("plus2", 5), ("plus1", 6), ("total", 2), ("total", 3), ("total", 4),
            "ambiguous_redundant", "ambiguous_not_redundant", "three_own_held", ("bytes_254", True), ("bytes_254", False)}
    assert need <= seen, need - seen
    assert {0, 5, 6, 7} <= own_octaves
    assert {s[1] for s in seen if isinstance(s, tuple) and s[0] == "lane"} == set(range(64))   # (cells with a usable depth: every lane adds to the counts)
    ends = set()
    for name, build in M.JOURNAL_CASES.items():
        m, F = M.MapModel(0), F0.fresh()
        sets, info = M.run_script(build, m, F)
        k = m.kfs[1]
        for i, p in enumerate(k.mp):
            if p >= 0:
                h = m.holder.get((1, i), -1)
                ends.add("held_by_cell_point" if h == p else ("held_by_nobody" if h < 0 else "held_by_another"))
        if any(ch["reset"] for ch in sets): ends.add("reset")
        if max(len(ch["events"]) for ch in sets) > 256: ends.add("over_256_events")
        if len(m.obs) > 100000: ends.add("point_block_grows")
    assert {"held_by_cell_point", "held_by_nobody", "reset", "over_256_events", "point_block_grows"} <= ends, ends
    # the displaced claim: held by another point while the cell's point keeps its observation
    m, F = M.MapModel(0), F0.fresh()
    M.CULL_CASES["total_3_displaced"][0](m, F)
    assert any(m.holder.get((1, i), -1) not in (-1, p) and 1 in m.obs[p] for i, p in enumerate(m.kfs[1].mp) if p >= 0)
    m, F = M.MapModel(0), F0.fresh()
    info = M.FUSE_CASES["displaced_claim_on_current"](m, F)
    a = info["want_ids"][1]
    assert m.is_in_keyframe(a, 1) and a not in m.kfs[1].mp


def _build_map_check(tmp_path, flags, tag):
    exe = str(tmp_path / ("slam_map_check_" + tag))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + flags + [os.path.join(HERE, "slam_map_check.cc"), "-o", exe])
    return exe


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DOSLAM_ARENA_PASSTHROUGH"]], ids=["plain", "asan_ubsan"])
def test_model_change_sets_equal_the_drivers(tmp_path, flags):
    """the same scripted operations through csrc/slam_map.h (Map::journal_changes) and through the Python model: equal change sets, flush by flush — events in
    order, dirty cells and points (current values) up to order.  Once more under AddressSanitizer + UBSan (the map's arena forwarding every block to malloc, so
    that the sanitizer sees the observation lists' bounds): the program is host code with its own main."""
    exe = _build_map_check(tmp_path, flags, "san" if flags else "plain")
    script = tmp_path / "script.txt"
    script.write_text(M.REPLAY_SCRIPT)
    out = subprocess.check_output([exe, "replay", str(script)], text=True)
    theirs = M.parse_replay_output(out)
    mine = M.replay_model()
    assert len(theirs) == len(mine) == M.REPLAY_SCRIPT.count("\nF")
    for q, (a, b) in enumerate(zip(mine, theirs)):
        assert a == b, "flush %d" % q
    kinds = set()
    for c in mine:
        kinds.update(k for k in ("new", "cells", "events", "points") if c[k])
        if c["reset"]: kinds.add("reset")
        kinds.update("set" if e[1] >> 31 else "clear" for e in c["events"])
        kinds.update("bad_point" for p in c["points"] if p[2])
    assert kinds == {"new", "cells", "events", "points", "reset", "set", "clear", "bad_point"}
    assert subprocess.check_output([exe], text=True).strip().endswith("slam_map_check ok")   # (the hand-built checks of the same program)
