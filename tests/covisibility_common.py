"""A literal Python restatement of the covisibility bookkeeping the covisibility graph (include/oslam_hip.h, "Covisibility graph") keeps on the device:
dicts and lists, the reference's loops (src/KeyFrame.cc:123-208, :289-398, :553-567; src/MapPoint.cc:201-271; src/Tracking.cc:1496-1604;
src/LoopClosing.cc:547-565) and ONE normalisation: wherever the reference walks a std::map<KeyFrame*, ...> or std::set<KeyFrame*> in pointer order, ids
ascend (sorted(...) below).  Plus the seeded keyframe stream and the hand-built cases the CPU and GPU tests share.  Nothing here imports the product."""
import collections
import functools

import numpy as np

OBS_ADD, OBS_ERASE, POINT_BAD, CONN_ADD, CONN_ERASE, KF_BAD, PARENT_SET = range(7)   # the event types of oslam_covis_event_t
TH = 15            # src/KeyFrame.cc:330
LOCAL_LIMIT = 80   # src/Tracking.cc:1550
OK, EMPTY, OVERFLOW = 0, 1, -3


class Graph:
    """One map: MapPoint::mObservations / mbBad per point id, KeyFrame's covisibility members per keyframe id.  `cap` is the product's bound on an
    observation list (normalisation 3 of the header): an add that meets a full list sets the point's overflow mark and changes nothing else."""

    def __init__(self, cap=64):
        self.cap = cap
        self.obs = collections.defaultdict(dict)        # mObservations: {keyframe: idx}
        self.pbad, self.povf = set(), set()
        self.conn = collections.defaultdict(dict)       # mConnectedKeyFrameWeights
        self.ordered = collections.defaultdict(list)    # mvpOrderedConnectedKeyFrames
        self.ordered_w = collections.defaultdict(list)  # mvOrderedWeights
        self.first = collections.defaultdict(lambda: True)   # mbFirstConnection
        self.parent = {}                                # mpParent
        self.kbad = set()
        self.ev = collections.Counter()

    # ---- MapPoint (src/MapPoint.cc) ----
    def add_observation(self, p, kf, idx):              # :201-212
        if kf in self.obs[p]:
            return 0
        if len(self.obs[p]) >= self.cap:
            self.povf.add(p)
            return 1
        self.obs[p][kf] = idx
        self.ev["longest_obs"] = max(self.ev["longest_obs"], len(self.obs[p]))
        return 0

    def erase_observation(self, p, kf):                 # :214-240 (SetBadFlag at nObs <= 2 is the caller's POINT_BAD)
        if kf in self.obs[p]:
            del self.obs[p][kf]

    def set_point_bad(self, p):                         # :254-263
        self.pbad.add(p)
        self.obs[p].clear()
        self.povf.discard(p)

    # ---- KeyFrame (src/KeyFrame.cc) ----
    def add_connection(self, k, other, w):              # :123-136
        if other not in self.conn[k]:
            self.conn[k][other] = w
        elif self.conn[k][other] != w:
            self.conn[k][other] = w
        else:
            self.ev["add_connection_no_change"] += 1
            return
        self.update_best_covisibles(k)

    def update_best_covisibles(self, k):                # :138-157
        v_pairs = []
        for other in sorted(self.conn[k]):
            v_pairs.append((self.conn[k][other], other))
        v_pairs.sort()
        l_kfs, l_ws = [], []
        for w, other in v_pairs:
            l_kfs.insert(0, other)
            l_ws.insert(0, w)
        self.ordered[k], self.ordered_w[k] = l_kfs, l_ws

    def erase_connection(self, k, other):               # :553-567
        b_update = False
        if other in self.conn[k]:
            del self.conn[k][other]
            b_update = True
        if b_update:
            self.update_best_covisibles(k)

    def change_parent(self, k, parent):                 # :393-398 (children are derived: normalisation 2 of the header)
        self.parent[k] = parent

    def get_connected_keyframes(self, k):               # :159-166
        return sorted(self.conn[k])

    def get_vector_covisible_keyframes(self, k):        # :168-172
        return list(self.ordered[k])

    def get_best_covisibility_keyframes(self, k, n):    # :174-182
        if len(self.ordered[k]) < n:
            return list(self.ordered[k])
        return list(self.ordered[k][:n])

    def get_covisibles_by_weight(self, k, w):           # :184-199
        if not self.ordered[k]:
            return []
        ws = self.ordered_w[k]
        it = len(ws)                                    # upper_bound(begin, end, w, weightComp), weightComp(a, b) = a > b: the first weight with w > weight
        for i, x in enumerate(ws):
            if w > x:
                it = i
                break
        if it == len(ws):
            if ws:
                self.ev["by_weight_quirk"] += 1
            return []
        return list(self.ordered[k][:it])

    def get_weight(self, k, other):                     # :201-208
        return self.conn[k].get(other, 0)

    def get_childs(self, k):
        return sorted(c for c, p in self.parent.items() if p == k)

    def update_connections(self, k, vp_mp):             # :289-379
        if any(p >= 0 and p not in self.pbad and p in self.povf for p in vp_mp):
            return OVERFLOW                             # the product's refusal: a list that lost observations was read
        counter = {}
        for p in vp_mp:
            if p < 0:
                continue
            if p in self.pbad:
                continue
            for kf in sorted(self.obs[p]):
                if kf == k:
                    continue
                counter[kf] = counter.get(kf, 0) + 1
        if not counter:
            self.ev["empty_counter"] += 1
            return EMPTY
        nmax, kf_max = 0, None
        v_pairs = []
        for kf in sorted(counter):
            if counter[kf] > nmax:
                nmax, kf_max = counter[kf], kf
            if counter[kf] >= TH:
                v_pairs.append((counter[kf], kf))
                self.add_connection(kf, k, counter[kf])
        if not v_pairs:
            v_pairs.append((nmax, kf_max))
            self.add_connection(kf_max, k, nmax)
            self.ev["max_fallback"] += 1
            self.ev["max_fallback_tie"] += sum(c == nmax for c in counter.values()) > 1
        v_pairs.sort()
        l_kfs, l_ws = [], []
        for w, kf in v_pairs:
            l_kfs.insert(0, kf)
            l_ws.insert(0, w)
        self.ev["ordered_tie"] += len(set(l_ws)) < len(l_ws)
        self.ev["row_below_th"] += any(c < TH for c in counter.values())
        self.conn[k] = dict(counter)
        self.ordered[k], self.ordered_w[k] = l_kfs, l_ws
        if self.first[k] and k != 0:
            self.parent[k] = l_kfs[0]
            self.first[k] = False
            self.ev["front_is_highest_id_of_a_tie"] += len(l_ws) > 1 and l_ws[0] == l_ws[1]
        return OK

    # ---- Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1496-1604) ----
    def update_local_keyframes(self, points):
        """dict(list, ref_kf, null), n = -1 for an empty vote, -3 when an overflowed list was read"""
        null = [0] * len(points)
        counter = {}
        ovf = False
        for i, p in enumerate(points):
            if p >= 0:
                if p not in self.pbad:
                    ovf = ovf or p in self.povf
                    for kf in sorted(self.obs[p]):
                        counter[kf] = counter.get(kf, 0) + 1
                else:
                    null[i] = 1
        if ovf:
            return dict(n=OVERFLOW, null=null)
        if not counter:
            self.ev["local_empty"] += 1
            return dict(n=-1, null=null)
        mx, kf_max = 0, None
        local = []
        track_ref = set()                               # mnTrackReferenceForFrame == mCurrentFrame.mnId
        for kf in sorted(counter):
            if kf in self.kbad:
                self.ev["local_bad_voter"] += 1
                continue
            if counter[kf] > mx:
                mx, kf_max = counter[kf], kf
            local.append(kf)
            track_ref.add(kf)
        for kf in list(local):                          # (itEndKF is the end before anything was pushed; reserve() keeps it valid)
            if len(local) > LOCAL_LIMIT:
                self.ev["local_limit"] += 1
                break
            for neigh in self.get_best_covisibility_keyframes(kf, 10):
                if neigh not in self.kbad:
                    if neigh not in track_ref:
                        local.append(neigh)
                        track_ref.add(neigh)
                        self.ev["local_neighbour"] += 1
                        break
                else:
                    self.ev["local_bad_neighbour"] += 1
            for child in self.get_childs(kf):
                if child not in self.kbad:
                    if child not in track_ref:
                        local.append(child)
                        track_ref.add(child)
                        self.ev["local_child"] += 1
                        break
                else:
                    self.ev["local_bad_child"] += 1
            parent = self.parent.get(kf)
            if parent is not None:
                if parent not in track_ref:
                    local.append(parent)
                    track_ref.add(parent)
                    self.ev["local_parent_break"] += 1
                    self.ev["local_parent_break_with_voters_left"] += kf != [v for v in sorted(counter) if v not in self.kbad][-1]
                    break
        return dict(n=len(local), list=local, ref_kf=-1 if kf_max is None else kf_max, null=null)

    # ---- LoopClosing::CorrectLoop (src/LoopClosing.cc:547-565) ----
    def loop_connections(self, connected, points_of):
        loop_connections = {}
        for kfi in connected:
            previous = self.get_vector_covisible_keyframes(kfi)
            self.update_connections(kfi, points_of[kfi])
            loop_connections[kfi] = set(self.get_connected_keyframes(kfi))
            for prev in previous:
                loop_connections[kfi].discard(prev)
            for kf2 in connected:
                loop_connections[kfi].discard(kf2)
        return loop_connections

    # ---- what one record of oslam_covis_update_connections answers ----
    def update_record(self, k, points, exclude):
        before = self.get_vector_covisible_keyframes(k)
        status = self.update_connections(k, points)
        if status == OVERFLOW:
            return dict(status=status, ordered=[], weights=[], parent=self.parent.get(k, -1), new_links=[])
        links = sorted(set(self.conn[k]) - set(before) - set(exclude))   # the set form of :556-564
        return dict(status=status, ordered=list(self.ordered[k]), weights=list(self.ordered_w[k]), parent=self.parent.get(k, -1), new_links=links)

    def apply(self, events):
        n_overflow = 0
        for e in events:
            t, a, b, c = (tuple(e) + (0, 0, 0))[:4]
            if t == OBS_ADD:
                n_overflow += self.add_observation(a, b, c)
            elif t == OBS_ERASE:
                self.erase_observation(a, b)
            elif t == POINT_BAD:
                self.set_point_bad(a)
            elif t == CONN_ADD:
                self.add_connection(a, b, c)
            elif t == CONN_ERASE:
                self.erase_connection(a, b)
            elif t == KF_BAD:
                self.kbad.add(a)
            elif t == PARENT_SET:
                self.change_parent(a, b)
            else:
                raise ValueError(t)
        return n_overflow

    def all_entries_rows(self):
        """the keyframes whose ordered list holds entries an UpdateConnections of their own would have left out"""
        return sum(1 for k in self.conn if self.ordered[k] and any(w < TH for w in self.ordered_w[k]) and len(self.ordered[k]) > 1)


# the (max_n, min_w) of every covisibles query of a snapshot, K standing for max_keyframes: GetVectorCovisibleKeyFrames, GetBestCovisibilityKeyFrames(10),
# GetCovisiblesByWeight(15), (100) and (1) — at 1 every weight passes, which is the quirk of :191-193
def query_params(K):
    return [(K, 0), (10, 0), (K, 15), (K, 100), (K, 1)]


def snapshot(g, K, kfs, points):
    """What the device must hold after an operation, for the keyframes and points named: dense weights, parents, flags, observation lists, and the answer
    of every query of query_params for every keyframe."""
    w = np.zeros((K, K), np.int32)
    for k, row in g.conn.items():
        for o, x in row.items():
            w[k, o] = x
    parents = np.full(K, -1, np.int32)
    for k, p in g.parent.items():
        parents[k] = p
    cov = {}
    for k in kfs:
        for max_n, min_w in query_params(K):
            ids = g.get_covisibles_by_weight(k, min_w) if min_w > 0 else g.get_vector_covisible_keyframes(k)
            ids = ids[:max_n]
            cov[(k, max_n, min_w)] = (ids, [g.conn[k][o] for o in ids])
    return dict(weights=w, parents=parents, bad=sorted(g.kbad), connected_once=sorted(k for k, f in g.first.items() if not f),
                observations={p: sorted(g.obs[p].items()) for p in points}, point_flags={p: (1 if p in g.pbad else 0) | (2 if p in g.povf else 0) for p in points},
                covisibles=cov, connected={k: g.get_connected_keyframes(k) for k in kfs})


def run(ops, K, cap=64, kfs=None, points=None, snapshots=True):
    """Replays a script — [("apply", events), ("update", [(keyframe, points, exclude)]), ("local", points)] — and returns (expected, graph): per
    operation dict(out=..., snap=snapshot after it)."""
    g = Graph(cap)
    expected = []
    kfs, points = kfs or [], points or []
    for kind, arg in ops:
        if kind == "apply":
            out = g.apply(arg)
        elif kind == "update":
            out = [g.update_record(k, pts, excl) for k, pts, excl in arg]
        elif kind == "local":
            out = g.update_local_keyframes(arg)
        else:
            raise ValueError(kind)
        expected.append(dict(out=out, snap=snapshot(g, K, kfs, points) if snapshots else None))
    return expected, g


# ---- the stream ------------------------------------------------------------------------------------------------------------------------------------
N_KF, N_PTS, N_OUT, REACH, MAX_PER_KF, P_SEE = 40, 900, 26, 70, 48, 0.55
BAD_POINTS = (900, 901, 902)   # three more slots that are bad from the start: what local_keyframes' input is salted with
N_SLOTS = N_PTS + len(BAD_POINTS)


@functools.lru_cache(maxsize=None)
def stream(seed, ids=None, n_kf=N_KF, n_out=N_OUT, density=1):
    """One graph of 40 keyframes over 900 points on a line: the camera goes 26 keyframes out (30 apart) and 14 back, so that the return leg re-observes
    the outbound points.  Each keyframe takes at most 48 of the points within 70 of its jittered position, each with probability 0.55; every observation
    is an OBS_ADD; UpdateConnections runs after each keyframe and again on keyframe k - 2 (leaving k - 1 and k out of its new_links) whenever
    k % 7 == 3; UpdateLocalKeyFrames runs after every step on the newest keyframe's points salted with bad points and empty slots.
    `ids` renames keyframe j to ids[j].  tools/covisibility_bench.py scales it: n_kf keyframes of which n_out go out, and `density` points per unit of
    length, each keyframe taking at most 48 * density of them; the three bad slots then follow the stream_slots(n_out, density) - 3 points.
    Returns (ops, keyframe ids, mvpMapPoints per keyframe id)."""
    rng = np.random.RandomState(1000 + seed)
    ids = list(range(n_kf)) if ids is None else list(ids)
    n_pts = stream_slots(n_out, density) - len(BAD_POINTS)
    bad_points = tuple(range(n_pts, n_pts + len(BAD_POINTS)))
    ops = [("apply", [(POINT_BAD, p) for p in bad_points])]
    mp = {}
    for j in range(n_kf):
        k = ids[j]
        x = 35 + 30 * (j if j < n_out else 2 * (n_out - 1) - j) + rng.randint(-5, 6)
        lo, hi = max(0, (x - REACH) * density), min(n_pts, (x + REACH) * density + 1)
        near = (lo + np.flatnonzero(rng.rand(hi - lo) < P_SEE)).tolist()
        if len(near) > MAX_PER_KF * density:
            near = sorted(rng.choice(near, MAX_PER_KF * density, replace=False).tolist())
        slots = list(rng.permutation(near).tolist())
        for at in sorted(rng.randint(0, len(slots) + 1, 3).tolist()):
            slots.insert(at, -1)
        mp[k] = slots
        ops.append(("apply", [(OBS_ADD, p, k, i) for i, p in enumerate(slots) if p >= 0]))
        upd = [(k, slots, [])]
        if j % 7 == 3:
            upd.append((ids[j - 2], mp[ids[j - 2]], [ids[j - 1], k]))
        ops.append(("update", upd))
        ops.append(("local", slots[:20] + [bad_points[j % 3], -1] + slots[20:] + [bad_points[(j + 1) % 3]]))
    return ops, ids, mp


def stream_slots(n_out=N_OUT, density=1):
    """the point slots of a stream: the line as far as the farthest keyframe sees, and the three bad slots (903 for the test stream)"""
    return (35 + 30 * (n_out - 1) + REACH + 5 + 40) * density + len(BAD_POINTS)


def spread_ids():
    """the 40 keyframes of the stream renamed to ids spread up to 2047 (0 stays 0: mnId != 0 guards the first parent)"""
    return tuple([0] + [53 * j - 20 for j in range(1, N_KF - 1)] + [2047])


# ---- hand-built cases ------------------------------------------------------------------------------------------------------------------------------
HAND_K, HAND_P, HAND_C = 128, 400, 16


def hand_cases():
    """{name: ops} at K = 128, P = 400, C = 16"""
    cases = {}
    # AddConnection / EraseConnection against a list that the keyframe's own UpdateConnections cut: points 0..15 are seen by keyframes 1 and 5, 16..18 by
    # 2 and 5, so UpdateConnections(5) keeps row {1: 16, 2: 3} and ordered [1]
    ev = [(OBS_ADD, p, 1, p) for p in range(16)] + [(OBS_ADD, p, 5, p) for p in range(19)] + [(OBS_ADD, p, 2, p - 16) for p in range(16, 19)]
    pts5 = list(range(19))
    cases["connections"] = [
        ("apply", ev),
        ("update", [(5, pts5, [])]),
        ("apply", [(CONN_ADD, 5, 2, 3)]),                  # an equal weight: the early return, the list stays cut
        ("apply", [(CONN_ERASE, 5, 7)]),                   # an absent id: nothing
        ("apply", [(CONN_ADD, 5, 2, 4)]),                  # a changed weight: UpdateBestCovisibles, every entry
        ("apply", [(CONN_ADD, 5, 3, 4), (CONN_ADD, 5, 9, 4)]),   # ties: descending id
        ("apply", [(CONN_ERASE, 5, 1)]),
        ("update", [(5, pts5 + [0, 0, -1, 3, 17], [2])]),  # duplicates count once per occurrence: {1: 19, 2: 4}; cut again; exclude
        ("apply", [(OBS_ERASE, 16, 2), (OBS_ERASE, 16, 2), (OBS_ADD, 16, 3, 7), (OBS_ADD, 16, 3, 9), (POINT_BAD, 17)]),
        ("update", [(5, pts5, []), (2, [16, 17, 18], []), (1, list(range(16)), [5])]),
        ("apply", [(PARENT_SET, 2, 5), (PARENT_SET, 3, 5), (PARENT_SET, 5, 9), (KF_BAD, 2)]),
        ("local", [0, 1, 16, 18, -1, 17]),
        ("apply", [(KF_BAD, 1), (KF_BAD, 9)]),
        ("local", [0, 1, 16, 18, -1, 17]),
        ("local", [-1, 17, -1]),                           # an empty vote
    ]
    # Tracking::UpdateLocalKeyFrames at its 80-entry limit: points 200..209 are seen by ten keyframes each (10..109), 210 by 110..116; voters 10, 11 and 12
    # each have a neighbour and a child that do not vote, and no parent
    ev = [(OBS_ADD, 200 + i, 10 + 10 * i + j, j) for i in range(10) for j in range(10)] + [(OBS_ADD, 210, 110 + j, j) for j in range(7)]
    ev += [(CONN_ADD, 10, 120, 30), (CONN_ADD, 10, 11, 40), (CONN_ADD, 11, 121, 30), (CONN_ADD, 12, 122, 30)]
    ev += [(PARENT_SET, 123, 10), (PARENT_SET, 124, 11), (PARENT_SET, 125, 12), (PARENT_SET, 20, 10)]
    cases["limit"] = [
        ("apply", ev),
        ("local", list(range(200, 210))),                  # 100 voters: the loop ends before its first neighbour
        ("local", list(range(200, 207)) + [210]),          # 77: voter 10 makes 79, voter 11 makes 81, voter 12 is not reached
        ("local", list(range(200, 207)) + [210, 207]),     # 87
        ("local", list(range(200, 203))),                  # 30: every voter is walked
        ("apply", [(PARENT_SET, 11, 126)]),
        ("local", list(range(200, 203))),                  # voter 11 adds its parent and ends the OUTER loop: voter 12 adds nothing
        ("apply", [(OBS_ADD, 300, 127, 0), (KF_BAD, 127)]),
        ("local", [300]),                                  # a vote, but no voter that is not bad: an empty list, no reference keyframe
    ]
    return cases


def hand_kfs():
    return list(range(HAND_K))


def hand_points():
    return list(range(0, 20)) + list(range(198, 212)) + [300, 399]


def overflow_case():
    """C = 4: point 0 is seen by five keyframes (the fifth add overflows), point 1 by four (full, no overflow)"""
    ev = [(OBS_ADD, 0, k, k) for k in (3, 1, 2, 4)] + [(OBS_ADD, 1, k, 0) for k in (1, 2, 3, 4)] + [(OBS_ADD, 0, 5, 1), (OBS_ADD, 0, 6, 1), (OBS_ADD, 0, 3, 9)]
    return [
        ("apply", ev),
        ("update", [(1, [1], []), (1, [0, 1], []), (2, [1, 1], [])]),   # the second record reads the overflowed list: -3 and nothing changes
        ("local", [0, 1]),
        ("local", [1]),
        ("apply", [(POINT_BAD, 0)]),
        ("update", [(1, [0, 1], [])]),
        ("local", [0, 1]),
        ("apply", [(OBS_ADD, 0, 7, 2)]),                   # AddObservation does not look at mbBad
    ]
