"""Shared by test_mirror_cases_cpu.py / test_mirror_cases_gpu.py: the operator table's device mirror of the observation graph (csrc/slam_ops_hip.hip: map_journal,
kf_culling_counts / _collect, local_points_list, fuse_into_current) pinned case by case.

  * ctypes mirrors of the structs that cross the table (MIRRORS: compared with gcc's sizeof by test_capi_cpu.py);
  * MapModel: the reference's bookkeeping (MapPoint::AddObservation / EraseObservation / SetBadFlag / Replace, src/MapPoint.cc:196-318; KeyFrame::AddMapPoint /
    EraseMapPointMatch / ReplaceMapPointMatch / SetBadFlag, src/KeyFrame.cc:201-230, :441-509; Tracking::Reset) over explicit containers — mObservations per point,
    mvpMapPoints per keyframe — which notes what it changes and emits change sets in the form include/oslam_slam.h states for oslam_map_changes_t;
  * three restatements over the model's explicit lists (never over the histogram): KeyFrameCulling's counting loop (src/LocalMapping.cc:646-692) with the header's
    `ambiguous` rule beside it, Tracking::UpdateLocalPoints (src/Tracking.cc:1470-1493) and the candidate list of SearchInNeighbors' second direction
    (src/LocalMapping.cc:497-513) with ORBmatcher::Fuse's exclusion `isBad() || IsInKeyFrame(pKF)`;
  * hand-built case tables: every case names its deciding gate and carries its answer written by hand.

A case is a function build(m, F): m a fresh MapModel, F a `Fixtures` — the keyframes a case may use (keypoint count, octaves, stereo flags and depths of their
keypoints).  On the CPU the fixtures are synthetic (synthetic_fixtures), on the GPU they are the frames the table extracted: cases pick keypoint indices BY OCTAVE
through F.pick, so the same table serves both.
"""
import ctypes as C

import numpy as np

# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# ctypes mirrors (include/oslam_slam.h)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
_P = C.c_void_p


class Frame(C.Structure):
    _fields_ = [("N", C.c_int32), ("keys", _P), ("keysUn", _P), ("desc", _P), ("uRight", _P), ("depth", _P)]


class MapNewKf(C.Structure):
    _fields_ = [("kf", C.c_int32), ("N", C.c_int32), ("mp", _P), ("good", _P)]


class MapChanges(C.Structure):
    _fields_ = [("slot", C.c_int32), ("reset", C.c_int32), ("n_new", C.c_int32), ("new_kfs", C.POINTER(MapNewKf)), ("n_cells", C.c_int32), ("cells", _P),
                ("n_events", C.c_int32), ("events", _P), ("n_points", C.c_int32), ("points", _P)]


class JobCull(C.Structure):
    _fields_ = [("slot", C.c_int32), ("n", C.c_int32), ("kf_ids", _P), ("out", _P)]


class JobFuseCur(C.Structure):
    _fields_ = [("slot", C.c_int32), ("kf", C.c_int32), ("n_targets", C.c_int32), ("targets", _P), ("Tcw", C.c_float * 16), ("Ow", C.c_float * 3), ("th", C.c_float),
                ("max_pairs", C.c_int32), ("pairs", _P), ("n_pairs", C.c_int32), ("n_candidates", C.c_int32), ("overflow", C.c_int32),
                ("dbg_cap", C.c_int32), ("dbg_ids", _P), ("dbg_excl", _P)]


class JobLocalList(C.Structure):
    _fields_ = [("slot", C.c_int32), ("n_kfs", C.c_int32), ("kfs", _P), ("cap", C.c_int32), ("ids", _P), ("n_ids", C.c_int32), ("overflow", C.c_int32)]


class JobMpUpdate(C.Structure):
    _fields_ = [("P", C.c_int32), ("obs_start", _P), ("obs_desc", _P), ("obs_Ow", _P), ("Pos", _P), ("OwRef", _P), ("levelScaleFactor", _P),
                ("do_desc", C.c_int32), ("do_normal", C.c_int32), ("items", _P), ("desc_start", _P), ("best_idx", _P), ("out_desc", _P), ("out5", _P)]


class JobFusePts(C.Structure):
    _fields_ = [("slot", C.c_int32), ("kf", C.c_int32), ("N", C.c_int32), ("M", C.c_int32), ("ids", _P), ("excl", _P), ("Tcw", C.c_float * 16), ("Ow", C.c_float * 3),
                ("th", C.c_float), ("q_match", _P)]


MIRRORS = [("oslam_slam_frame_t", Frame), ("oslam_map_new_kf_t", MapNewKf), ("oslam_map_changes_t", MapChanges), ("oslam_job_cull_t", JobCull),
           ("oslam_job_fuse_cur_t", JobFuseCur), ("oslam_job_local_list_t", JobLocalList), ("oslam_job_mp_update_t", JobMpUpdate), ("oslam_job_fuse_pts_t", JobFusePts)]

# the bounds of the HIP table (HipOps::kFuseCurStride / kFuseCurPairs, csrc/slam_ops_hip.hip): candidates / matches per job beyond which a job reports overflow
STRIDE, MAX_PAIRS = 16384, 2048


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the map model
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
class KF:
    def __init__(self, kf, octave, stereo, depth, th_depth):
        self.id, self.N = kf, len(octave)
        self.octave = [int(o) for o in octave]           # mvKeysUn[i].octave
        self.stereo = [bool(s) for s in stereo]          # mvuRight[i] >= 0
        # LocalMapping.cc:661: `if(pKF->mvDepth[i]>pKF->mThDepth || pKF->mvDepth[i]<0) continue;` — the usable-depth bit is its negation
        self.good = [not (d > th_depth or d < 0) for d in depth]
        self.mp = [-1] * self.N                          # mvpMapPoints
        self.bad = False


class MapModel:
    """One sequence's map.  mObservations is a std::map<KeyFrame*, size_t>: iterated by keyframe id here (include/oslam_slam.h, normalisations)."""

    def __init__(self, slot=0):
        self.slot = slot
        self._clear()
        self.n_reset = 0

    def _clear(self):
        self.kfs, self.obs, self.nobs, self.isbad = {}, [], [], []
        self.holder = {}   # (kf, idx) -> the point whose AddObservation was the last event on it (header: "the LAST one decides", an erase clears it whoever held it)
        self.j_new, self.j_cells, self.j_events, self.j_pts, self.j_ptset = [], [], [], [], set()

    # -- Tracking::Reset: the map is cleared, ids restart
    def reset(self):
        self._clear()
        self.n_reset = 1

    def new_keyframe(self, kf, octave, stereo, depth, th_depth, mp=None):
        k = KF(kf, octave, stereo, depth, th_depth)
        if mp is not None:   # KeyFrame::KeyFrame copies Frame::mvpMapPoints
            k.mp = list(mp)
        self.kfs[kf] = k
        self.j_new.append(kf)
        return k

    def new_point(self):
        self.obs.append({}); self.nobs.append(0); self.isbad.append(False)
        return len(self.obs) - 1

    def _dirty(self, p):
        if p not in self.j_ptset:
            self.j_ptset.add(p)
            self.j_pts.append(p)

    # -- MapPoint (src/MapPoint.cc)
    def add_observation(self, p, kf, idx):               # :201-212
        if kf in self.obs[p]:
            return
        self.obs[p][kf] = idx
        self.nobs[p] += 2 if self.kfs[kf].stereo[idx] else 1
        self.j_events.append((kf, idx, 1, p)); self.holder[(kf, idx)] = p
        self._dirty(p)

    def erase_observation(self, p, kf):                  # :214-240
        bad = False
        if kf in self.obs[p]:
            idx = self.obs[p][kf]
            self.nobs[p] -= 2 if self.kfs[kf].stereo[idx] else 1
            del self.obs[p][kf]
            self.j_events.append((kf, idx, 0, p)); self.holder.pop((kf, idx), None)
            self._dirty(p)
            if self.nobs[p] <= 2:
                bad = True
        if bad:
            self.set_bad_flag(p)

    def set_bad_flag(self, p):                           # :254-271
        self.isbad[p] = True
        obs, self.obs[p] = self.obs[p], {}
        for kf in sorted(obs):
            self.kf_erase_match(kf, obs[kf])
            self.j_events.append((kf, obs[kf], 0, p)); self.holder.pop((kf, obs[kf]), None)
        self._dirty(p)

    def replace(self, p, q):                             # :280-318
        if p == q:
            return
        obs, self.obs[p] = self.obs[p], {}
        self.isbad[p] = True
        for kf in sorted(obs):
            idx = obs[kf]
            self.j_events.append((kf, idx, 0, p)); self.holder.pop((kf, idx), None)   # (p lost the observation: noted where the loop reaches it)
            if kf not in self.obs[q]:                    # !pMP->IsInKeyFrame(pKF)
                self.kf_replace_match(kf, idx, q)
                self.add_observation(q, kf, idx)
            else:
                self.kf_erase_match(kf, idx)
        self._dirty(p)

    def observations(self, p):
        return self.nobs[p]

    def is_in_keyframe(self, p, kf):
        return kf in self.obs[p]

    # -- KeyFrame (src/KeyFrame.cc)
    def kf_add_map_point(self, kf, p, idx):              # :201-205
        self.kfs[kf].mp[idx] = p
        self.j_cells.append((kf, idx))

    def kf_erase_match(self, kf, idx):                   # :207-211
        self.kfs[kf].mp[idx] = -1
        self.j_cells.append((kf, idx))

    def kf_replace_match(self, kf, idx, p):              # :221-224
        self.kfs[kf].mp[idx] = p
        self.j_cells.append((kf, idx))

    def kf_set_bad_flag(self, kf):                       # :441-509, the part that touches observations (:468-470)
        if kf == 0:
            return
        k = self.kfs[kf]
        for i in range(k.N):
            if k.mp[i] >= 0:
                self.erase_observation(k.mp[i], kf)
        k.bad = True

    # -- a claim as the reference makes it (CreateNewMapPoints, LocalMapping.cc:440-446; ORBmatcher::Fuse, ORBmatcher.cc:939-943): observation, then the cell
    def claim(self, p, kf, idx):
        self.add_observation(p, kf, idx)
        self.kf_add_map_point(kf, p, idx)

    def histogram(self, p):
        h = [0] * 8
        for kf, idx in self.obs[p].items():
            h[self.kfs[kf].octave[idx]] += 1
        assert max(h) <= 255
        return h

    # -- the change set since the last flush (include/oslam_slam.h:236-251)
    def flush(self):
        new = []
        for kf in self.j_new:
            k = self.kfs[kf]
            good = np.zeros((k.N + 31) // 32, np.uint32)
            for i in range(k.N):
                if k.good[i]:
                    good[i >> 5] |= np.uint32(1 << (i & 31))
            new.append((kf, k.N, np.array(k.mp, np.int32).reshape(-1), good))
        cells = np.array([(kf, idx, self.kfs[kf].mp[idx]) for kf, idx in self.j_cells], np.int32).reshape(-1, 3)
        events = np.array([(kf, idx | (s << 31), p) for kf, idx, s, p in self.j_events], np.uint32).reshape(-1, 3)
        pts = []
        for p in self.j_pts:
            h = self.histogram(p)
            pts.append((p, self.nobs[p] & 0xFFFFFFFF, int(self.isbad[p]), sum(h[o] << (8 * o) for o in range(4)), sum(h[o + 4] << (8 * o) for o in range(4))))
        ch = dict(slot=self.slot, reset=self.n_reset, new=new, cells=cells, events=events, points=np.array(pts, np.uint32).reshape(-1, 5))
        self.n_reset = 0
        self.j_new, self.j_cells, self.j_events, self.j_pts, self.j_ptset = [], [], [], [], set()
        return ch


def canonical(ch):
    """A change set up to what the header leaves open: dirty cells and dirty points carry CURRENT values, so their order (and repeats) do not matter; events stay
    in program order."""
    return dict(reset=int(ch["reset"]), new=[(int(kf), int(N), [int(x) for x in mp], [int(x) for x in good]) for kf, N, mp, good in ch["new"]],
                cells=sorted(set(tuple(int(x) for x in r) for r in ch["cells"])), events=[tuple(int(x) for x in r) for r in ch["events"]],
                points=sorted(set(tuple(int(x) for x in r) for r in ch["points"])))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# restatements over the explicit lists
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def cull_reference(m, kf):
    """LocalMapping::KeyFrameCulling's loop body for one keyframe (src/LocalMapping.cc:646-692, stereo / RGB-D: mbMonocular false).  Returns (slots with a point at a
    usable depth — the header's out[0], which the reference does not compute: a point, bad or not, in a cell whose depth passes :661 —, nMPs, nRedundantObservations,
    the set of cells counted redundant)."""
    k = m.kfs[kf]
    usable = nMPs = 0
    red = set()
    thObs = 3
    for i, p in enumerate(k.mp):
        if p < 0:
            continue
        if k.good[i]:
            usable += 1
        if m.isbad[p]:
            continue
        if not k.good[i]:
            continue
        nMPs += 1
        if m.observations(p) > thObs:
            level = k.octave[i]
            n = 0
            for kfi in sorted(m.obs[p]):
                if kfi == kf:
                    continue
                if m.kfs[kfi].octave[m.obs[p][kfi]] <= level + 1:
                    n += 1
                    if n >= thObs:
                        break
            if n >= thObs:
                red.add(i)
    return usable, nMPs, len(red), red


def cull_ambiguous(m, kf):
    """include/oslam_slam.h, kf_culling_counts out[4 q + 3]: the cells whose point (counted in nMPs, Observations() > 3) has EXACTLY three observations at octave
    <= level + 1 — its own included, if it has one — while the observation (kf, i) is not held by that point (the last event on (kf, i) was not its AddObservation)."""
    k = m.kfs[kf]
    amb = set()
    for i, p in enumerate(k.mp):
        if p < 0 or m.isbad[p] or not k.good[i] or m.observations(p) <= 3:
            continue
        n = sum(1 for kfi, idx in m.obs[p].items() if m.kfs[kfi].octave[idx] <= k.octave[i] + 1)
        if n == 3 and m.holder.get((kf, i), -1) != p:
            amb.add(i)
    return amb


def cull_expected(m, kf):
    """What the table must return for a resident keyframe: the reference's counts, with the ambiguous points reported and left out of nRedundantObservations."""
    usable, nMPs, _, red = cull_reference(m, kf)
    amb = cull_ambiguous(m, kf)
    return (usable, nMPs, len(red - amb), len(amb))


def local_points(m, kfs):
    """Tracking::UpdateLocalPoints (src/Tracking.cc:1470-1493): mnTrackReferenceForFrame is the `seen` set."""
    out, seen = [], set()
    for kf in kfs:
        for p in m.kfs[kf].mp:
            if p < 0:
                continue
            if p in seen:
                continue
            if not m.isbad[p]:
                out.append(p)
                seen.add(p)
    return out


def first_occurrence_by_key(m, kfs, swapped=False):
    """The mark-and-list rule of k_fusecur_mark / k_fusecur_list restated: every (position t in the list, cell i) proposes a key for its good point, the smallest key
    names the point's first occurrence, the list is walked in (t, i) order and keeps the occurrences whose key stayed.  swapped = True orders the key by (i, t) — the
    slip a case on first occurrences has to catch: test_mirror_cases_cpu.py shows that the hand-built cases give another list under it."""
    best = {}
    for t, kf in enumerate(kfs):
        if kf not in m.kfs:
            continue
        for i, p in enumerate(m.kfs[kf].mp):
            if p >= 0 and not m.isbad[p]:
                key = (i, t) if swapped else (t, i)
                if p not in best or key < best[p]:
                    best[p] = key
    out = []
    for t, kf in enumerate(kfs):
        if kf not in m.kfs:
            continue
        for i, p in enumerate(m.kfs[kf].mp):
            if p >= 0 and not m.isbad[p] and best[p] == ((i, t) if swapped else (t, i)):
                out.append(p)
    return out


def fuse_candidates(m, cur, targets):
    """vpFuseCandidates (src/LocalMapping.cc:497-513; mnFuseCandidateForKF is the `seen` set) and, per candidate, ORBmatcher::Fuse's exclusion
    `pMP->isBad() || pMP->IsInKeyFrame(pKF)` (src/ORBmatcher.cc:849) from mObservations."""
    ids, seen = [], set()
    for kf in targets:
        for p in m.kfs[kf].mp:
            if p < 0:
                continue
            if m.isbad[p] or p in seen:
                continue
            seen.add(p)
            ids.append(p)
    return ids, [1 if (m.isbad[p] or m.is_in_keyframe(p, cur)) else 0 for p in ids]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# fixtures: the keyframes the cases are built on
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
TH_DEPTH = 40.0 * 40.0 / 520.908620   # mThDepth = bf * ThDepth / fx of the TUM2 settings the GPU table is created with (src/Tracking.cc:159)


class Fixtures:
    """frames[f] = (octave[N], stereo[N], depth[N]) of image f.  keyframe(m, kf, f) adds keyframe `kf` with image f's keypoints; pick() chooses keypoint indices by
    octave / depth class ('near': stereo and usable, 'far': stereo beyond mThDepth, 'mono': no depth) and never returns an index twice per (image, class, octave)."""

    def __init__(self, frames, cap):
        self.frames, self.cap = frames, cap
        self.kf_frame = {}
        self._used = {}
        self.pending = []   # (slot, keyframe, image) in creation order: the GPU test registers them with the table before the change set that names them

    def keyframe(self, m, kf, f=0, N=None, mp=None):
        octave, stereo, depth = self.frames[f]
        if N is not None:   # (the mirror takes N from the change set: a keyframe may be journalled shorter or — up to cap — longer than its frame)
            n0 = len(octave)
            # (keypoints beyond the frame's: usable depth, so that the tail of the usable-depth words is set; their octave is never read on the device as long
            # as the points in those cells have Observations() <= 3 — the record holds no keypoint there)
            octave = [octave[i] if i < n0 else 0 for i in range(N)]; stereo = [stereo[i] if i < n0 else True for i in range(N)]
            depth = [depth[i] if i < n0 else 2.0 for i in range(N)]
        self.kf_frame[(m.slot, kf)] = f
        self.pending.append((m.slot, kf, f))
        return m.new_keyframe(kf, octave, stereo, depth, TH_DEPTH, mp)

    def klass(self, f, i):
        octave, stereo, depth = self.frames[f]
        return "mono" if not stereo[i] else ("far" if depth[i] > TH_DEPTH else "near")

    def pick(self, f, octave, klass="near", n=1, lo=0):
        oc = self.frames[f][0]
        used = self._used.setdefault(f, set())
        octaves = octave if isinstance(octave, tuple) else (octave,)
        out = [i for i in range(lo, len(oc)) if oc[i] in octaves and self.klass(f, i) == klass and i not in used][:n]
        assert len(out) == n, "image %d has fewer than %d unused %s keypoints at octave %s" % (f, n, klass, octave)
        used.update(out)
        return out if n > 1 else out[0]

    def reserve(self, f, idxs):
        self._used.setdefault(f, set()).update(idxs)

    def fresh(self):
        g = Fixtures(self.frames, self.cap)
        return g


def synthetic_fixtures(n_images=3, N=1100, cap=1400):
    """CPU stand-in for the extracted frames: every octave and every depth class at every residue, deterministic."""
    frames = []
    for f in range(n_images):
        n = N + 37 * f
        octave = [(i + f) % 8 for i in range(n)]
        klass = [((i // 8) + f) % 5 for i in range(n)]   # 0, 1, 2: near; 3: far; 4: mono
        stereo = [c != 4 for c in klass]
        depth = [2.0 if c < 3 else (100.0 if c == 3 else -1.0) for c in klass]
        frames.append((octave, stereo, depth))
    return Fixtures(frames, cap)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# culling cases.  build(m, F) -> dict(kf=[candidate ids], want=[(usable, nMPs, nRedundant, ambiguous) or None = "no record": (0, 0, 0, != 0)], release=[...])
# Keyframe ids: 1 = the candidate K (image 0); 2 .. = observers (images 1, 2, 0, ...); virtual keyframes (never registered with the table) from 100.
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _observers(m, F, n, first=2):
    kfs = []
    for q in range(n):
        F.keyframe(m, first + q, f=(1 + q) % len(F.frames))
        kfs.append(first + q)
    return kfs


def _point_seen(m, F, K, i, others):
    """a point in cell (K, i) with the claim of the reference, observed by `others` = [(kf, octave, class)]"""
    p = m.new_point()
    m.claim(p, K, i)
    for kf, o, c in others:
        m.claim(p, kf, F.pick(F.kf_frame[(m.slot, kf)], o, c))
    return p


def _octave_case(o, d, n_other):
    """own cell at octave o; n_other further observations at octave min(o + d, 7)"""
    def build(m, F):
        F.keyframe(m, 1, 0)
        ob = _observers(m, F, n_other)
        i = F.pick(0, o)
        _point_seen(m, F, 1, i, [(kf, o + d, "near") for kf in ob])
        return dict(kf=[1])
    return build


def c_empty(m, F):
    F.keyframe(m, 1, 0)
    return dict(kf=[1])


def c_far_depth(m, F):
    """usable-depth bit 0 (depth beyond mThDepth, and no depth at all): not counted anywhere, though the points are fully redundant"""
    F.keyframe(m, 1, 0); ob = _observers(m, F, 4)
    _point_seen(m, F, 1, F.pick(0, 0, "far"), [(kf, 0, "near") for kf in ob])
    _point_seen(m, F, 1, F.pick(0, 0, "mono"), [(kf, 0, "near") for kf in ob])
    return dict(kf=[1])


def _kf_with_twin(F, m, kf, f, c, i, j):
    """keyframe kf arrives with point c at TWO keypoints i < j (a frame can match one point twice, and KeyFrame::KeyFrame copies mvpMapPoints); ProcessNewKeyFrame
    adds the observation at the first (LocalMapping.cc:141-147: IsInKeyFrame is true at the second).  When c goes bad later, SetBadFlag clears the cell of its
    observation, i; cell j keeps the bad point — this is how a keyframe's list comes to hold one."""
    mp = [-1] * len(F.frames[f][0]); mp[i] = c; mp[j] = c
    F.keyframe(m, kf, f, mp=mp)
    m.add_observation(c, kf, i)


def c_bad_point(m, F):
    c = m.new_point()
    i, j = F.pick(0, 1, n=2)
    _kf_with_twin(F, m, 1, 0, c, i, j); ob = _observers(m, F, 4)
    for kf in ob:
        m.claim(c, kf, F.pick(F.kf_frame[(m.slot, kf)], 0))
    m.set_bad_flag(c)
    return dict(kf=[1])


def c_obs3(m, F):
    """Observations() == 3 (own stereo + one mono): the `> thObs` gate is closed"""
    F.keyframe(m, 1, 0); ob = _observers(m, F, 1)
    _point_seen(m, F, 1, F.pick(0, 0), [(ob[0], 0, "mono")])
    return dict(kf=[1])


def c_obs4(m, F):
    """Observations() == 4 (own stereo + one stereo): the gate is open, one other observation is not three"""
    F.keyframe(m, 1, 0); ob = _observers(m, F, 1)
    _point_seen(m, F, 1, F.pick(0, 0), [(ob[0], 0, "near")])
    return dict(kf=[1])


def c_total2(m, F):
    """qualifying total 2 (own + one at octave <= o + 1), two more observations too coarse"""
    F.keyframe(m, 1, 0); ob = _observers(m, F, 3)
    _point_seen(m, F, 1, F.pick(0, 0), [(ob[0], 1, "near"), (ob[1], 2, "near"), (ob[2], 3, "near")])
    return dict(kf=[1])


def c_total3_own(m, F):
    """qualifying total 3 with K's own observation among them: two others -> not redundant, and not ambiguous"""
    F.keyframe(m, 1, 0); ob = _observers(m, F, 3)
    _point_seen(m, F, 1, F.pick(0, 0), [(ob[0], 1, "near"), (ob[1], 0, "near"), (ob[2], 3, "near")])
    return dict(kf=[1])


def c_total3_displaced(m, F):
    """qualifying total 3, and the observation (K, i) was last claimed by ANOTHER point q that has not taken the cell (the state between the AddObservation and the
    AddMapPoint calls of LocalMapping.cc:440-446): the mirror cannot vouch for p's own observation -> ambiguous.  By the lists p has two others: not redundant."""
    F.keyframe(m, 1, 0); ob = _observers(m, F, 3)
    i = F.pick(0, 0)
    _point_seen(m, F, 1, i, [(ob[0], 1, "near"), (ob[1], 0, "near"), (ob[2], 3, "near")])
    q = m.new_point()
    m.add_observation(q, 1, i)
    return dict(kf=[1])


def c_total3_foreign(m, F):
    """the cell (K, i) holds p, p does not observe K (AddMapPoint without AddObservation) and has exactly three observations elsewhere at a fine enough octave: the
    reference counts it redundant; the mirror reports it ambiguous and leaves it out of the count"""
    F.keyframe(m, 1, 0); ob = _observers(m, F, 3)
    i = F.pick(0, 0)
    p = m.new_point()
    for kf in ob:
        m.claim(p, kf, F.pick(F.kf_frame[(m.slot, kf)], 1))
    m.kf_add_map_point(1, p, i)
    return dict(kf=[1])


def c_total4(m, F):
    F.keyframe(m, 1, 0); ob = _observers(m, F, 3)
    _point_seen(m, F, 1, F.pick(0, 0), [(ob[0], 1, "near"), (ob[1], 0, "near"), (ob[2], 1, "near")])
    return dict(kf=[1])


def _c_254(own_octave):
    def build(m, F):
        """254 observations at octave 2 and 254 at octave 3 (virtual keyframes: the histogram travels with the dirty point).  Own cell at octave 1: only octave 2
        counts; at octave 2: both, 16-bit partial sums 254 + 254 + 1 without a carry into the neighbour"""
        F.keyframe(m, 1, 0)
        p = m.new_point()
        m.claim(p, 1, F.pick(0, own_octave))
        n2 = 254 - (1 if own_octave == 2 else 0)   # (the own observation is one of the 254 at octave 2)
        for q in range(n2 + 254):
            m.new_keyframe(100 + q, [2 if q < n2 else 3], [True], [2.0], TH_DEPTH)
            m.claim(p, 100 + q, 0)
        return dict(kf=[1])
    return build


def c_lanes(m, F):
    """redundant points at keypoints 0, 63, 64, N - 1 (whatever their depth) and, for every lane l of the wavefront, at the first keypoint i = l mod 64 behind
    keypoint 64 with a usable depth: every one of the 64 lanes adds to all three counts.  Four others at octave 0 or 1, which is fine enough for any own octave."""
    K = F.keyframe(m, 1, 0); ob = _observers(m, F, 4)
    per_lane = [min(i for i in range(65, K.N - 1) if i % 64 == l and F.klass(0, i) == "near") for l in range(64)]
    idx = sorted(set([0, 63, 64, K.N - 1] + per_lane))
    near = [i for i in idx if F.klass(0, i) == "near"]
    assert set(i % 64 for i in near) == set(range(64))
    o_idx = {kf: F.pick(F.kf_frame[(m.slot, kf)], (0, 1), "near", n=len(idx)) for kf in ob}
    for n, i in enumerate(idx):
        p = m.new_point()
        m.claim(p, 1, i)
        for kf in ob:
            m.claim(p, kf, o_idx[kf][n])
    return dict(kf=[1], near=len(near), total=len(idx))


def c_released(m, F):
    """candidate 1 resident, 2 released after its journal, 9 never registered; and an empty job's worth of nothing in between (the GPU test adds the n = 0 job)"""
    F.keyframe(m, 1, 0); ob = _observers(m, F, 4)
    _point_seen(m, F, 1, F.pick(0, 0), [(kf, 0, "near") for kf in ob])
    return dict(kf=[1, 2, 9, 1], release=[2], none=[2, 9])


CULL_CASES = {
    # name: (build, deciding gate, hand-written answer per candidate: (usable, nMPs, nRedundant, ambiguous); None = no record)
    "empty":            (c_empty,              "pMP != NULL",                         [(0, 0, 0, 0)]),
    "depth_bit_0":      (c_far_depth,          "mvDepth > mThDepth || mvDepth < 0",   [(0, 0, 0, 0)]),
    "bad_point":        (c_bad_point,          "pMP->isBad()",                        [(1, 0, 0, 0)]),
    "observations_3":   (c_obs3,               "Observations() > thObs (closed)",     [(1, 1, 0, 0)]),
    "observations_4":   (c_obs4,               "Observations() > thObs (open)",       [(1, 1, 0, 0)]),
    "o0_plus1":         (_octave_case(0, 1, 3), "scaleLeveli <= scaleLevel + 1 (=)",   [(1, 1, 1, 0)]),
    "o0_plus2":         (_octave_case(0, 2, 3), "scaleLeveli <= scaleLevel + 1 (>)",   [(1, 1, 0, 0)]),
    "o5_plus1":         (_octave_case(5, 1, 3), "octave 6 against level 5",            [(1, 1, 1, 0)]),
    "o5_plus2":         (_octave_case(5, 2, 3), "octave 7 against level 5",            [(1, 1, 0, 0)]),
    "o6_plus1":         (_octave_case(6, 1, 3), "octave 7 against level 6: the whole histogram", [(1, 1, 1, 0)]),
    "o7_same":          (_octave_case(7, 0, 3), "octave 7 against level 7: the whole histogram", [(1, 1, 1, 0)]),
    "total_2":          (c_total2,             "nObs >= thObs: 1 other",              [(1, 1, 0, 0)]),
    "total_3_own":      (c_total3_own,         "nObs >= thObs: 2 others, own held",   [(1, 1, 0, 0)]),
    "total_3_displaced": (c_total3_displaced,  "ambiguous: own observation displaced", [(1, 1, 0, 1)]),
    "total_3_foreign":  (c_total3_foreign,     "ambiguous: 3 others, no own",         [(1, 1, 0, 1)]),
    "total_4":          (c_total4,             "nObs >= thObs: 3 others",             [(1, 1, 1, 0)]),
    "bytes_254_own1":   (_c_254(1),            "histogram bytes 254 | 254, mask between them", [(1, 1, 1, 0)]),
    "bytes_254_own2":   (_c_254(2),            "histogram bytes 254 | 254, both summed",       [(1, 1, 1, 0)]),
    "lanes":            (c_lanes,              "every lane, keypoints 0 / 63 / 64 / N - 1",    None),   # (answer from the fixture: (near, near, near, 0))
    "released":         (c_released,           "no resident record",                  [(1, 1, 1, 0), None, None, (1, 1, 1, 0)]),
}


def cull_want(name, info):
    want = CULL_CASES[name][2]
    if name == "lanes":
        return [(info["near"], info["near"], info["near"], 0)]
    return want


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# journal cases: scripts of flushes.  build(m, F) is a generator: a bare `yield` is a flush (map_journal), `yield ("release", [kf, ..])` a release_keyframes
# call; it returns dict(kf=[candidates], want=[hand-written counts or None], lists=[(keyframes, hand-written UpdateLocalPoints list)]).  After the last flush the
# mirror is read back through its consumers: the `ambiguous` count shows who holds an observation, the lists show the cells.
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def j_N0(m, F):
    F.keyframe(m, 1, 0, N=0)
    yield
    return dict(kf=[1], want=[(0, 0, 0, 0)], lists=[([1], [])])


def j_N33(m, F):
    """N not a multiple of 32, the last keypoint with a usable depth and a point: the tail word of the usable-depth bits and the tail of the point list"""
    i = min(k for k in range(32, len(F.frames[0][0])) if F.klass(0, k) == "near" and (k + 1) % 32 != 0)
    F.reserve(0, [i])
    F.keyframe(m, 1, 0, N=i + 1)
    p = m.new_point(); m.claim(p, 1, i)
    yield
    return dict(kf=[1], want=[(1, 1, 0, 0)], lists=[([1], [p])])


def j_Ncap(m, F):
    """N = cap: the last cell (beyond the frame's keypoints, usable depth) and the first usable cell hold a point each"""
    F.keyframe(m, 1, 0, N=F.cap)
    assert F.cap > len(F.frames[0][0])
    p, q = m.new_point(), m.new_point()
    m.claim(q, 1, F.cap - 1); m.claim(p, 1, F.pick(0, (0, 1, 2, 3, 4, 5, 6, 7)))
    yield
    return dict(kf=[1], want=[(2, 2, 0, 0)], lists=[([1], [p, q])])


def j_bulk_and_cell(m, F):
    """the keyframe arrives with point p in its list (bulk record, CURRENT values) and, in the same flush, q takes another cell and p's is erased (p goes bad:
    Observations() <= 2)"""
    p, q = m.new_point(), m.new_point()
    i, j = F.pick(0, 0, n=2)
    mp = [-1] * len(F.frames[0][0]); mp[i] = p
    F.keyframe(m, 1, 0, mp=mp)
    m.add_observation(p, 1, i)
    m.claim(q, 1, j)
    m.kf_erase_match(1, i); m.erase_observation(p, 1)
    yield
    return dict(kf=[1], want=[(1, 1, 0, 0)], lists=[([1], [q])])


def _raced(m, F):
    """keyframe 1 with the raced cell i (octave 0, usable depth), observers 2, 3, 4; p and q each observed by 2 and 3 at octave 0: with keyframe 1's observation a
    point has exactly three qualifying observations, so the culling count shows whether the mirror holds the observation (1, i) for it"""
    F.keyframe(m, 1, 0); ob = _observers(m, F, 3)
    p, q = m.new_point(), m.new_point()
    for x in (p, q):
        for kf in ob[:2]:
            m.claim(x, kf, F.pick(F.kf_frame[(m.slot, kf)], 0))
    return p, q, ob, F.pick(0, 0)


def _expose_nobody(m, F, p, ob, i):
    """after the last event on (1, i) was an erase: p gets a third observation elsewhere and the cell (1, i) WITHOUT the observation.  Nobody holds (1, i): ambiguous.
    A mirror that still believed p held it would count p's three observations as own + 2: not ambiguous."""
    m.claim(p, ob[2], F.pick(F.kf_frame[(m.slot, ob[2])], 0))
    m.kf_add_map_point(1, p, i)


def _orders(kind, split):
    def build(m, F):
        p, q, ob, i = _raced(m, F)
        if split:
            yield
        if kind == "set_set":
            m.claim(p, 1, i)
            if split:
                yield
            m.claim(q, 1, i)
            yield
            return dict(kf=[1], want=[(1, 1, 0, 0)], lists=[([1], [q])])
        if kind == "set_clear":
            m.claim(p, 1, i)
            if split:
                yield
            m.erase_observation(p, 1); m.kf_erase_match(1, i)
            _expose_nobody(m, F, p, ob, i)
            yield
            return dict(kf=[1], want=[(1, 1, 0, 1)], lists=[([1], [p])])
        m.claim(p, 1, i); m.erase_observation(p, 1); m.kf_erase_match(1, i)
        if split:
            yield
        m.claim(q, 1, i)
        yield
        return dict(kf=[1], want=[(1, 1, 0, 0)], lists=[([1], [q])])
    return build


def j_many_events(m, F):
    """on each of 8 cells, interleaved, 2 x 150 events + 2 in ONE flush (2416 events: ten workgroups of k_mirror_ops race on every cell): 150 x (claim p, erase p),
    then claim p, then q's displacing claim.  The last event decides: q holds every one of them."""
    F.keyframe(m, 1, 0); ob = _observers(m, F, 3)
    cells = F.pick(0, 0, n=8)
    P, Q = [], []
    for i in cells:
        p, q = m.new_point(), m.new_point()
        for x in (p, q):
            for kf in ob[:2]:
                m.claim(x, kf, F.pick(F.kf_frame[(m.slot, kf)], 0))
        P.append(p); Q.append(q)
    yield
    for _ in range(150):
        for p, i in zip(P, cells):
            m.claim(p, 1, i)
        for p, i in zip(P, cells):
            m.erase_observation(p, 1); m.kf_erase_match(1, i)
    for p, i in zip(P, cells):
        m.claim(p, 1, i)
    for q, i in zip(Q, cells):
        m.claim(q, 1, i)
    yield
    return dict(kf=[1], want=[(8, 8, 0, 0)], lists=[([1], Q)])


def j_many_events_clear(m, F):
    """the same race ending in an erase on every cell: "nobody", although 151 set events with smaller numbers are in flight beside each erase"""
    F.keyframe(m, 1, 0); ob = _observers(m, F, 3)
    cells = F.pick(0, 0, n=8)
    P = []
    for i in cells:
        p = m.new_point()
        for kf in ob[:2]:
            m.claim(p, kf, F.pick(F.kf_frame[(m.slot, kf)], 0))
        P.append(p)
    yield
    for _ in range(151):
        for p, i in zip(P, cells):
            m.claim(p, 1, i)
        for p, i in zip(P, cells):
            m.erase_observation(p, 1); m.kf_erase_match(1, i)
    for p, i in zip(P, cells):
        _expose_nobody(m, F, p, ob, i)
    yield
    return dict(kf=[1], want=[(8, 8, 0, 8)], lists=[([1], P)])


def j_released_kf(m, F):
    """events and cells that name keyframe 2 after its record went back (release_keyframes): skipped, nothing else disturbed"""
    F.keyframe(m, 1, 0); ob = _observers(m, F, 3)
    p, q = m.new_point(), m.new_point()
    ip, iq = F.pick(0, 0, n=2)
    m.claim(p, 1, ip)
    for kf in ob:
        m.claim(p, kf, F.pick(F.kf_frame[(m.slot, kf)], 0))
    yield
    yield ("release", [2])
    m.claim(q, 2, F.pick(F.kf_frame[(m.slot, 2)], 0)); m.claim(q, 1, iq)
    for kf in ob[1:]:
        m.claim(q, kf, F.pick(F.kf_frame[(m.slot, kf)], 0))
    yield
    return dict(kf=[1], want=[(2, 2, 2, 0)], lists=[([1, 2, 3], [p, q])])


def j_grow_points(m, F):
    """point ids 0 .. 2 first, then id 300000: the per-point block is reallocated; the earlier records must survive (three redundant points stay redundant)"""
    F.keyframe(m, 1, 0); ob = _observers(m, F, 3)
    pts = [m.new_point() for _ in range(3)]
    for x in pts:
        m.claim(x, 1, F.pick(0, 0))
        for kf in ob:
            m.claim(x, kf, F.pick(F.kf_frame[(m.slot, kf)], 0))
    yield
    while len(m.obs) < 300000:
        m.new_point()
    z = m.new_point()
    m.claim(z, 1, F.pick(0, 0)); m.claim(z, 2, F.pick(F.kf_frame[(m.slot, 2)], 0))
    yield
    return dict(kf=[1], want=[(4, 4, 3, 0)], lists=[([1], pts + [z])])


def j_reset_smaller(m, F):
    """a full map, Tracking::Reset, then keyframes 0 and 1 with a SMALLER N on reused records (register_keyframes with id 0 frees the slot's records): no cell, claim
    or usable-depth bit of the old map may show.  Point ids restart: id 0 of the new map is a fresh point, and the change set says reset = 1."""
    n0 = len(F.frames[0][0])
    F.keyframe(m, 0, 0); F.keyframe(m, 1, 0)
    for i in range(n0):
        p = m.new_point(); m.claim(p, 0, i); m.claim(p, 1, i)
    yield
    m.reset()
    F.keyframe(m, 0, 0, N=40); F.keyframe(m, 1, 0, N=40)
    i = F.pick(0, 0)
    assert i < 40
    p = m.new_point()   # id 0 again: the old id 0 sat in cell 0 of both keyframes
    assert p == 0
    m.claim(p, 0, i); m.claim(p, 1, i)
    yield
    return dict(kf=[1], want=[(1, 1, 0, 0)], lists=[([0, 1], [p])])


JOURNAL_CASES = {
    "N_0": j_N0, "N_not_multiple_of_32": j_N33, "N_cap": j_Ncap, "bulk_and_cell": j_bulk_and_cell,
    "set_set": _orders("set_set", False), "set_clear": _orders("set_clear", False), "clear_set": _orders("clear_set", False),
    "set_set_split": _orders("set_set", True), "set_clear_split": _orders("set_clear", True), "clear_set_split": _orders("clear_set", True),
    "many_events": j_many_events, "many_events_clear": j_many_events_clear, "released_kf": j_released_kf, "grow_points": j_grow_points,
    "reset_smaller_N": j_reset_smaller,
}


def run_script(build, m, F, on_flush=None, on_action=None):
    """drives a journal case: on_flush(change set) at every bare yield, on_action(kind, arg) for the table-side actions; returns (change sets, the case's answer)"""
    out = []
    g = build(m, F)
    while True:
        try:
            step = next(g)
        except StopIteration as e:
            return out, e.value
        if step is not None:
            if on_action:
                on_action(*step)
            continue
        ch = m.flush(); out.append(ch)
        if on_flush:
            on_flush(ch)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# list cases (local_points_list and the candidate half of fuse_into_current).  build(m, F) -> dict(kfs=[...], cap=None | int); hand-written answers beside them.
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def l_first_occurrence(m, F):
    """point a sits at cell 900 of keyframe 1 and at cell 2 of keyframe 2: its first occurrence in (keyframe, cell) order is the LATER cell of the EARLIER keyframe.
    x is only in keyframe 2, at cell 1, below a's cell there: an order by (cell, keyframe) would move a behind x.  b at cell 3 of keyframe 1 and cell 4 of keyframe
    2; c is bad and still in cell 6 of keyframe 2; d only in keyframe 2; keyframe 1 is listed twice.  UpdateLocalPoints over (1, 2, 1): b, a, x, d."""
    a, b, c, d, x = (m.new_point() for _ in range(5))
    F.keyframe(m, 1, 0); _kf_with_twin(F, m, 2, 1, c, 0, 6)
    m.claim(a, 1, 900); m.claim(a, 2, 2)
    m.claim(b, 1, 3); m.claim(b, 2, 4)
    m.claim(x, 2, 1)
    m.claim(d, 2, 5)
    m.set_bad_flag(c)
    return dict(kfs=[1, 2, 1], want=[b, a, x, d])


def l_full(m, F):
    """every slot of two keyframes filled, N > 1024: keyframe 1 holds points 0 .. N1 - 1 in REVERSED order, keyframe 2 repeats every other point of keyframe 1 and adds
    new ones: the list crosses the 1024-thread tile and all 16 wavefronts of k_fusecur_list"""
    K1 = F.keyframe(m, 1, 0); K2 = F.keyframe(m, 2, 1)
    assert K1.N > 1024 and K2.N > 1024
    for i in range(K1.N):
        p = m.new_point(); m.claim(p, 1, K1.N - 1 - i)
    for i in range(K2.N):
        if i % 2 == 0 and i < K1.N:
            m.claim(i, 2, i)
        else:
            p = m.new_point(); m.claim(p, 2, i)
    n_new = sum(1 for i in range(K2.N) if not (i % 2 == 0 and i < K1.N))
    want = list(range(K1.N - 1, -1, -1)) + list(range(K1.N, K1.N + n_new))
    return dict(kfs=[1, 2], want=want)


def l_too_many(m, F):
    """more than 16384 distinct points over 16 keyframes with every slot filled: overflow"""
    n = 0
    for q in range(16):
        K = F.keyframe(m, 1 + q, q % len(F.frames))
        for i in range(K.N):
            p = m.new_point(); m.claim(p, 1 + q, i); n += 1
    assert n > STRIDE
    return dict(kfs=list(range(1, 17)), want=None, n=n)


LIST_CASES = {"first_occurrence": l_first_occurrence, "full_over_1024": l_full, "too_many": l_too_many}


# fuse cases: build(m, F) -> dict(cur=kf, targets=[...], want_ids=[...], want_excl=[...])
def f_basic(m, F):
    """current keyframe 1, targets 2, 3.  a: in 2 and in the current keyframe -> candidate, excluded.  b: only in 2 -> candidate.  c: bad, still in cell 9 of 2 ->
    absent.  d: in 2 at a late cell (700) and in 3 at cell 5 -> once, at its place in keyframe 2's list.  e: only in 3, at cell 0, below d's cell there: an order by
    (cell, keyframe) would put d behind e."""
    a, b, c, d, e = (m.new_point() for _ in range(5))
    F.keyframe(m, 1, 0); _kf_with_twin(F, m, 2, 1, c, 3, 9); F.keyframe(m, 3, 2)
    m.claim(a, 2, 4); m.claim(a, 1, 8)
    m.claim(b, 2, 2)
    m.claim(d, 3, 5); m.claim(d, 2, 700)
    m.claim(e, 3, 0)
    m.set_bad_flag(c)
    return dict(cur=1, targets=[2, 3], want_ids=[b, a, d, e], want_excl=[0, 1, 0, 0])


def f_displaced(m, F):
    """a claimed keypoint 8 of the current keyframe, then z claimed the same keypoint (LocalMapping.cc:440-446 twice): z holds the cell, a keeps its observation.
    a is in target 2's list: MapPoint::IsInKeyFrame(current) is true -> the reference excludes it (ORBmatcher.cc:849)."""
    F.keyframe(m, 1, 0); F.keyframe(m, 2, 1)
    a, b, z = m.new_point(), m.new_point(), m.new_point()
    m.claim(a, 2, 4); m.claim(a, 1, 8)
    m.claim(z, 1, 8)
    m.claim(b, 2, 2)
    return dict(cur=1, targets=[2], want_ids=[b, a], want_excl=[0, 1])


FUSE_CASES = {"basic": f_basic, "displaced_claim_on_current": f_displaced}


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the replay script shared with tests/slam_map_check.cc (`slam_map_check replay <file>`): one operation per line, the same bookkeeping on both sides.
# Keypoint i of a replayed keyframe: octave i % 8, class (i / 8) % 5 as in synthetic_fixtures (image 0).
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
REPLAY_N = 64
REPLAY_SCRIPT = """K 0
K 1
K 2
K 3
P
P
P
P
P
A 0 0 0
M 0 0 0
A 0 1 0
M 1 0 0
A 0 2 1
M 2 1 0
A 1 1 5
M 1 5 1
A 1 2 5
M 2 5 1
A 1 0 6
M 0 6 1
F
A 2 1 5
M 1 5 2
A 2 3 9
M 3 9 2
A 2 2 32
M 2 32 2
A 3 0 33
M 0 33 3
A 3 3 33
M 3 33 3
F
R 1 2
E 0 2
M 2 1 -1
F
A 4 3 40
M 3 40 4
A 4 1 32
M 1 32 4
E 4 3
B 3
X 2
F
Z
K 0
P
A 0 0 3
M 0 3 0
F
"""


def replay_model(script=REPLAY_SCRIPT, th_depth=TH_DEPTH):
    """The model's side of the replay: the list of canonical change sets, one per F line."""
    F = synthetic_fixtures(1, REPLAY_N, REPLAY_N)
    m = MapModel(0)
    out = []
    for line in script.split("\n"):
        t = line.split()
        if not t:
            continue
        a = [int(x) for x in t[1:]]
        if t[0] == "K":
            F.keyframe(m, a[0], 0)
        elif t[0] == "P":
            m.new_point()
        elif t[0] == "A":
            m.add_observation(a[0], a[1], a[2])
        elif t[0] == "M":
            m.kf_add_map_point(a[0], a[2], a[1]) if a[2] >= 0 else m.kf_erase_match(a[0], a[1])
        elif t[0] == "E":
            m.erase_observation(a[0], a[1])
        elif t[0] == "B":
            m.set_bad_flag(a[0])
        elif t[0] == "R":
            m.replace(a[0], a[1])
        elif t[0] == "X":
            m.kf_set_bad_flag(a[0])
        elif t[0] == "Z":
            m.reset()
        elif t[0] == "F":
            out.append(canonical(m.flush()))
        else:
            raise ValueError(line)
    return out


def parse_replay_output(text):
    """what `slam_map_check replay` prints: per flush `flush reset=R`, then `new kf N : mp.. : good..`, `cell kf idx p`, `event kf word p`, `point p nobs bad lo hi`"""
    out, cur = [], None
    for line in text.split("\n"):
        t = line.split()
        if not t:
            continue
        if t[0] == "flush":
            cur = dict(reset=int(t[1].split("=")[1]), new=[], cells=[], events=[], points=[])
            out.append(cur)
        elif t[0] == "new":
            rest = " ".join(t[3:]).split(":")
            cur["new"].append((int(t[1]), int(t[2]), [int(x) for x in rest[1].split()], [int(x) for x in rest[2].split()]))
        elif t[0] == "cell":
            cur["cells"].append(tuple(int(x) for x in t[1:]))
        elif t[0] == "event":
            cur["events"].append(tuple(int(x) for x in t[1:]))
        elif t[0] == "point":
            cur["points"].append(tuple(int(x) for x in t[1:]))
    for c in out:
        c["cells"] = sorted(set(c["cells"])); c["points"] = sorted(set(c["points"]))
    return out
