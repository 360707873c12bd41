"""Shared by tests/test_loop_detect_cpu.py and tests/test_loop_detect_gpu.py: the YARDSTICK — a literal Python restatement of LoopClosing::DetectLoop
(reference src/LoopClosing.cc:104-230) over Python sets of keyframe ids and a list of (set, int) for mvConsistentGroups, with the RefDatabase of
tests/keyframe_db_common.py for the query and np.float32 wherever the reference has `float` — and the generators of its inputs.  Nothing below calls into
the library.

The normalisations of include/oslam_hip.h ("LoopClosing::DetectLoop") are here too: a connected keyframe counts as !isBad() when it is in the database, and
a consistency update whose list would exceed max_groups is refused and changes nothing."""
import collections
import functools

import numpy as np

import keyframe_db_common as kc

F32 = np.float32
REFUSED_CAPACITY = -3


def update_consistency_nested(prev, cands, connected, th):
    """:153-212, the nested loops as they stand.  prev: mvConsistentGroups, [(set, int)]; cands: vpCandidateKFs (ids); connected(id): the set
    GetConnectedKeyFrames() returns.  Returns (vCurrentConsistentGroups, mvpEnoughConsistentCandidates, events)."""
    ev = collections.Counter()
    mvpEnoughConsistentCandidates = []
    vCurrentConsistentGroups = []
    vbConsistentGroup = [False] * len(prev)
    met = [0] * len(prev)
    for pCandidateKF in cands:
        spCandidateGroup = set(connected(pCandidateKF))
        spCandidateGroup.add(pCandidateKF)
        bEnoughConsistent = False
        bConsistentForSomeGroup = False
        n_met = 0
        for iG in range(len(prev)):
            sPreviousGroup = prev[iG][0]
            bConsistent = False
            for sit in sorted(spCandidateGroup):
                if sit in sPreviousGroup:
                    bConsistent = True
                    bConsistentForSomeGroup = True
                    break
            if bConsistent:
                n_met += 1
                met[iG] += 1
                nPreviousConsistency = prev[iG][1]
                nCurrentConsistency = nPreviousConsistency + 1
                if not vbConsistentGroup[iG]:
                    vCurrentConsistentGroups.append((set(spCandidateGroup), nCurrentConsistency))
                    vbConsistentGroup[iG] = True
                if nCurrentConsistency >= th and not bEnoughConsistent:
                    mvpEnoughConsistentCandidates.append(pCandidateKF)
                    bEnoughConsistent = True
        if not bConsistentForSomeGroup:
            vCurrentConsistentGroups.append((set(spCandidateGroup), 0))
            ev["fresh"] += 1
        ev["candidate_meets_two_groups"] += n_met >= 2
        ev["only_overlap_is_itself"] += n_met >= 1 and not any(connected(pCandidateKF) & g for g, _ in prev)
    ev["group_met_by_two_candidates"] += sum(m >= 2 for m in met)
    ev["enough_nonempty"] += len(mvpEnoughConsistentCandidates) >= 1
    ev["enough_two_or_more"] += len(mvpEnoughConsistentCandidates) >= 2
    return vCurrentConsistentGroups, mvpEnoughConsistentCandidates, ev


def update_consistency_sets(prev, cands, connected, th):
    """The same as steps 1-5 of include/oslam_hip.h: what the kernel computes.  Returns (groups, enough)."""
    group = [set(connected(c)) | {c} for c in cands]                                          # 1
    C = [[bool(group[i] & prev[g][0]) for g in range(len(prev))] for i in range(len(cands))]  # 2
    first = [min([i for i in range(len(cands)) if C[i][g]], default=None) for g in range(len(prev))]   # 3
    new, enough = [], []
    for i in range(len(cands)):
        for g in range(len(prev)):                                                            # 4
            if first[g] == i:
                new.append((set(group[i]), prev[g][1] + 1))
        if not any(C[i]):
            new.append((set(group[i]), 0))
        if any(C[i][g] and prev[g][1] + 1 >= th for g in range(len(prev))):                   # 5
            enough.append(cands[i])
    return new, enough


class RefLoopClosing:
    """What LoopClosing keeps for DetectLoop of one sequence: the database, the connections of the keyframes, mvConsistentGroups, mLastLoopKFid."""

    def __init__(self, th=3, max_groups=64):
        self.db = kc.RefDatabase()
        self.connected = {}                 # id -> set of ids: GetConnectedKeyFrames(), whether or not those keyframes are in the database
        self.mvConsistentGroups = []
        self.mLastLoopKFid = 0
        self.mnCovisibilityConsistencyTh = th
        self.max_groups = max_groups
        self.events = collections.Counter()

    def conn_of(self, k):
        return self.connected.get(k, set())

    def update_consistency(self, cands):
        """:144-226 given the candidates.  Returns (n_enough or REFUSED_CAPACITY, enough)."""
        if not cands:
            self.mvConsistentGroups = []
            self.events["cleared"] += 1
            return 0, []
        new, enough, ev = update_consistency_nested(self.mvConsistentGroups, cands, self.conn_of, self.mnCovisibilityConsistencyTh)
        if len(new) > self.max_groups:      # the operator's refusal: nothing changes
            return REFUSED_CAPACITY, []
        self.events.update(ev)
        self.mvConsistentGroups = new
        self.events["max_groups"] = max(self.events["max_groups"], len(new))
        return len(enough), enough

    def detect(self, ids, vals, conn):
        """:122-226 without the add: minScore, the query, the consistency update."""
        minScore = F32(1)
        for c in conn:
            if c not in self.db.kfs:        # pKF->isBad()
                continue
            score = F32(kc.score_l1(np.asarray(ids, np.uint32), np.asarray(vals, np.float64), self.db.kfs[c].ids, self.db.kfs[c].vals))
            if score < minScore:
                minScore = score
        r = self.db.detect_loop_candidates(ids, vals, minScore, conn)
        r["log"] = self.db.log
        r["min_score"] = minScore
        r["n_enough"], r["enough"] = self.update_consistency(r["cand"])
        r["groups"] = self.groups()
        return r

    def DetectLoop(self, mnId, ids, vals, conn):
        """:104-230; returns the result dict with `ret` (the reference's bool) and `gated`."""
        if mnId < self.mLastLoopKFid + 10:
            self.db.add(mnId, ids, vals)
            return dict(gated=True, ret=False, enough=[], groups=self.groups())
        r = self.detect(ids, vals, conn)
        self.db.add(mnId, ids, vals)
        r["gated"], r["ret"] = False, len(r["enough"]) > 0
        return r

    def groups(self):
        return [(sorted(g), n) for g, n in self.mvConsistentGroups]


# ---- the keyframe stream ----
VISITS = ((0, 14), (1, 10), (0, 12), (2, 6), (1, 8))   # (scene, keyframes): 50 keyframes, scenes 0 and 1 are seen again
N_STREAM = sum(n for _, n in VISITS)


def revisit_script(seed):
    """One sequence: 50 keyframes over three 110-word scenes of a 300-word vocabulary.  Per keyframe a dict: kf, ids, vals, conn (the connected ids when it
    is detected, ascending), rows [(keyframe, connected ids)] and covis [(keyframe, list)] to apply before the detection (the keyframe's new connections
    seen from both sides; the lists of keyframes that are in the database), covis_after (the keyframe's own list, set once it has been added)."""
    rng = np.random.default_rng(seed)
    scenes = [rng.choice(300, 110, replace=False) for _ in range(3)]
    steps, connected, k = [], {}, 0
    newest10 = lambda s: sorted(s, reverse=True)[:10]   # noqa: E731
    for scene, n in VISITS:
        visit = []
        for _ in range(n):
            ids, vals = kc.scene_vector(rng, scenes[scene], 300, 40, 100)
            prev = visit[-6:]
            connected[k] = set(prev)
            for p in prev:
                connected[p].add(k)
            steps.append(dict(kf=k, ids=ids, vals=vals, conn=sorted(connected[k]), rows=[(x, sorted(connected[x])) for x in [k] + prev],
                              covis=[(p, newest10(connected[p])) for p in prev], covis_after=(k, newest10(connected[k]))))
            visit.append(k)
            k += 1
    return steps


def run_revisit(steps, th=3, last_loop_at=None):
    """The restatement over one stream: (per keyframe the result of DetectLoop, the RefLoopClosing).  last_loop_at = (keyframe, value): mLastLoopKFid is set
    to value before that keyframe is processed (what CorrectLoop does, :585)."""
    lc = RefLoopClosing(th)
    out = []
    for s in steps:
        if last_loop_at and s["kf"] == last_loop_at[0]:
            lc.mLastLoopKFid = last_loop_at[1]
        for kf, l in s["rows"]:
            lc.connected[kf] = set(l)
        for kf, l in s["covis"]:
            lc.db.set_covisibility(kf, l)
        out.append(lc.DetectLoop(s["kf"], s["ids"], s["vals"], s["conn"]))
        lc.db.set_covisibility(*s["covis_after"])
    return out, lc


@functools.lru_cache(maxsize=None)
def revisit_fixture(seed):
    """(steps, expected, events) of revisit_script(seed), computed once and shared by the tests; nobody changes it."""
    steps = revisit_script(seed)
    expected, lc = run_revisit(steps)
    return steps, expected, lc.events


# ---- consistency cases: sequences of (row updates, candidates) that do not depend on any score ----
def consistency_cases(K, seed=3):
    """[dict(name, K, max_groups, th, steps)] for keyframe ids 0 .. K - 1 (K >= 40): steps = [(rows {keyframe: connected ids}, candidates)], replayed from
    empty rows and groups.  case_triples() gives the (rows, previous groups, candidates) triple of every step and what the restatement makes of it."""
    A = dict(name="branches", K=K, max_groups=64, th=3, steps=[
        ({0: [1, 2], 1: [0, 2], 2: [0, 1], 10: [11], 11: [10], 20: [], K - 1: [K - 2], K - 2: [K - 1]}, [0, 10]),   # two fresh groups
        ({}, [1, 11, 20]),         # each of the first two meets one group; 20 is fresh
        ({}, [2, 0, 10]),          # group 0 is met by two candidates and pushed once; the group of 20 is dropped
        ({}, [1, 2, 11]),          # counters reach 3: three enough candidates, two of them through one group
        ({30: [0, 10]}, [30]),     # one candidate meets two groups: pushed twice, enough once
        ({}, [30, 30]),            # a repeated id: two candidates
        ({30: []}, [30]),          # its only overlap with the previous groups is itself
        ({}, [K - 1, 33]),         # ids in the last (partial) word, fresh
        ({}, [K - 2, 33]),         # ... and met through a row; 33 through itself
        ({}, []),                  # no candidate: cleared
        ({}, [K - 1]),             # and fresh again at 0
    ])
    B = dict(name="capacity", K=K, max_groups=4, th=3, steps=[
        ({}, [0, 1, 2, 3]),        # exactly max_groups groups
        ({}, [0, 1, 2, 3, 4]),     # max_groups + 1: refused, nothing changes
        ({}, [3, 2]),              # the state the refusal left
        ({5: [2, 3]}, [5, 6, 7]),  # 5 meets two groups, two fresh: 4 again
        ({}, [5, 5, 6, 7, 8]),     # 5 pushes twice, 6, 7 once, 8 fresh: 5 groups, refused
        ({}, [6]),
    ])
    rng = np.random.default_rng(seed + K)
    pool = rng.choice(K, 14, replace=False).tolist() + [K - 1]
    rows0 = {}
    for a in pool:
        rows0[a] = sorted(set(rng.choice(pool, int(rng.integers(0, 4))).tolist() + rng.integers(0, K, int(rng.integers(0, 3))).tolist()) - {a})
    steps = [(rows0, rng.choice(pool, 3).tolist())]
    for it in range(14):
        upd = {}
        if it % 4 == 3:
            a = pool[int(rng.integers(len(pool)))]
            upd[a] = sorted(set(rng.choice(pool, 3).tolist()) - {a})
        n = int(rng.integers(0, 7)) if it != 9 else 0
        steps.append((upd, rng.choice(pool, n).tolist() if n else []))   # (with replacement: ids repeat)
    R = dict(name="random", K=K, max_groups=64, th=2, steps=steps)
    return [A, B, R]


def run_case(case):
    """The restatement over one case: per step dict(rows, prev, cands, n_enough, enough, groups, events)."""
    lc = RefLoopClosing(case["th"], case["max_groups"])
    out = []
    for upd, cands in case["steps"]:
        for kf, l in upd.items():
            lc.connected[kf] = set(l)
        prev = [(set(g), n) for g, n in lc.mvConsistentGroups]
        n_enough, enough = lc.update_consistency(list(cands))
        out.append(dict(rows={k: set(v) for k, v in lc.connected.items()}, prev=prev, cands=list(cands), n_enough=n_enough, enough=enough, groups=lc.groups()))
    return out, lc.events


@functools.lru_cache(maxsize=None)
def case_fixture(K):
    cases = consistency_cases(K)
    return cases, [run_case(c) for c in cases]
