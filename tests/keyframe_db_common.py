"""Shared by tests/test_keyframe_db_cpu.py and tests/test_keyframe_db_gpu.py: the YARDSTICK — a literal Python restatement of ORB_SLAM2::KeyFrameDatabase
(reference src/KeyFrameDatabase.cc:33-309) with a real inverted file (per-word lists with push_back and erase), the mnLoopQuery / mnLoopWords / mLoopScore /
mnRelocQuery / mnRelocWords / mRelocScore fields on keyframe objects, and np.float32 wherever the reference has `float` — and the seeded generator of
databases, queries and whole scripts of operations.  Nothing below calls into the library.

The two normalisations of include/oslam_hip.h ("KeyFrameDatabase") are here too: mRelocScore is 0 at add, and every query carries a fresh id."""
import functools

import numpy as np

F32 = np.float32
MAX_WORDS = 2400


def score_l1(qi, qv, ki, kv):
    """DBoW2 L1Scoring::score walking both vectors (the loop of oslam_voc_score), fp64."""
    s, i, j = 0.0, 0, 0
    while i < len(qi) and j < len(ki):
        if qi[i] == ki[j]:
            a, b = float(qv[i]), float(kv[j])
            s += abs(a - b) - abs(a) - abs(b)
            i += 1; j += 1
        elif qi[i] < ki[j]:
            i += 1
        else:
            j += 1
    return -0.5 * s


class RefKeyFrame:
    def __init__(self, mnId, ids, vals):
        self.mnId, self.ids, self.vals = mnId, np.asarray(ids, np.uint32), np.asarray(vals, np.float64)
        self.mnLoopQuery = self.mnRelocQuery = 0   # (queries are stamped from 1)
        self.mnLoopWords = self.mnRelocWords = 0
        self.mLoopScore = F32(0)
        self.mRelocScore = F32(0)                  # normalisation 1: the reference leaves it uninitialised
        self.covis = []                            # ids, GetBestCovisibilityKeyFrames(10)


class RefDatabase:
    """One KeyFrameDatabase.  `log` of the last query holds every comparison of scores it made: (kind, lhs, rhs)."""

    def __init__(self):
        self.mvInvertedFile = {}   # word id -> list of RefKeyFrame (std::list<KeyFrame*>)
        self.kfs = {}              # the keyframes that are in the database, by id
        self.stamp = 0             # normalisation 2: a fresh id per query
        self.serial = 0
        self.log = []

    def add(self, mnId, ids, vals):
        assert mnId not in self.kfs
        kf = RefKeyFrame(mnId, ids, vals)
        kf.serial = self.serial    # (only the order test reads it)
        self.serial += 1
        self.kfs[mnId] = kf
        for w in kf.ids.tolist():
            self.mvInvertedFile.setdefault(w, []).append(kf)

    def erase(self, mnId):
        kf = self.kfs.pop(mnId, None)
        if kf is None:
            return
        for w in kf.ids.tolist():
            lKFs = self.mvInvertedFile[w]
            for i, x in enumerate(lKFs):
                if x is kf:
                    del lKFs[i]
                    break

    def clear(self):
        self.mvInvertedFile = {}
        self.kfs = {}

    def set_covisibility(self, mnId, ids):
        assert len(ids) <= 10
        self.kfs[mnId].covis = [int(i) for i in ids]

    def _neighbours(self, kf):
        return [self.kfs[i] for i in kf.covis if i in self.kfs]   # normalisation 4: ids that are not in the database are skipped

    def _finish(self, lAccScoreAndMatch, bestAccScore, out):
        minScoreToRetain = F32(0.75) * bestAccScore
        spAlreadyAddedKF, cand, acc = set(), [], []
        for accScore, pKFi in lAccScoreAndMatch:
            self.log.append(("retain", accScore, minScoreToRetain))
            if accScore > minScoreToRetain and pKFi.mnId not in spAlreadyAddedKF:
                cand.append(pKFi.mnId); acc.append(accScore)
                spAlreadyAddedKF.add(pKFi.mnId)
        out.update(cand=cand, acc=acc)
        return out

    def detect_loop_candidates(self, ids, vals, minScore, connected):
        ids, vals, minScore = np.asarray(ids, np.uint32), np.asarray(vals, np.float64), F32(minScore)
        self.stamp += 1
        mnId = self.stamp
        self.log = []
        out = dict(cand=[], acc=[], sharing=[], scores={})
        out["conn_score"] = [F32(score_l1(ids, vals, self.kfs[c].ids, self.kfs[c].vals)) if c in self.kfs else F32(-1) for c in connected]
        spConnectedKeyFrames = set(int(c) for c in connected)
        lKFsSharingWords = []
        for w in ids.tolist():
            for pKFi in self.mvInvertedFile.get(w, []):
                if pKFi.mnLoopQuery != mnId:
                    pKFi.mnLoopWords = 0
                    if pKFi.mnId not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = mnId
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1
        out["sharing"] = [k.mnId for k in lKFsSharingWords]
        out["diag"] = [len(lKFsSharingWords), 0, 0, 0, 0]
        if not lKFsSharingWords:
            return out
        maxCommonWords = max(k.mnLoopWords for k in lKFsSharingWords)
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        nscores = 0
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                nscores += 1
                si = F32(score_l1(ids, vals, pKFi.ids, pKFi.vals))
                pKFi.mLoopScore = si
                out["scores"][pKFi.mnId] = si
                self.log.append(("minScore", si, minScore))
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
        out["diag"] = [len(lKFsSharingWords), maxCommonWords, minCommonWords, nscores, len(lScoreAndMatch)]
        if not lScoreAndMatch:
            return out
        lAccScoreAndMatch = []
        bestAccScore = minScore
        for si, pKFi in lScoreAndMatch:
            bestScore, accScore, pBestKF = si, si, pKFi
            for pKF2 in self._neighbours(pKFi):
                if pKF2.mnLoopQuery == mnId and pKF2.mnLoopWords > minCommonWords:
                    accScore = F32(accScore + pKF2.mLoopScore)
                    self.log.append(("best", pKF2.mLoopScore, bestScore))
                    if pKF2.mLoopScore > bestScore:
                        pBestKF, bestScore = pKF2, pKF2.mLoopScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return self._finish(lAccScoreAndMatch, bestAccScore, out)

    def detect_relocalization_candidates(self, ids, vals):
        ids, vals = np.asarray(ids, np.uint32), np.asarray(vals, np.float64)
        self.stamp += 1
        mnId = self.stamp
        self.log = []
        out = dict(cand=[], acc=[], sharing=[], scores={})
        lKFsSharingWords = []
        for w in ids.tolist():
            for pKFi in self.mvInvertedFile.get(w, []):
                if pKFi.mnRelocQuery != mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = mnId
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        out["sharing"] = [k.mnId for k in lKFsSharingWords]
        out["diag"] = [len(lKFsSharingWords), 0, 0, 0, 0]
        if not lKFsSharingWords:
            return out
        maxCommonWords = max(k.mnRelocWords for k in lKFsSharingWords)
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        nscores = 0
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                nscores += 1
                si = F32(score_l1(ids, vals, pKFi.ids, pKFi.vals))
                pKFi.mRelocScore = si
                out["scores"][pKFi.mnId] = si
                lScoreAndMatch.append((si, pKFi))
        out["diag"] = [len(lKFsSharingWords), maxCommonWords, minCommonWords, nscores, len(lScoreAndMatch)]
        if not lScoreAndMatch:
            return out
        lAccScoreAndMatch = []
        bestAccScore = F32(0)
        for si, pKFi in lScoreAndMatch:
            bestScore, accScore, pBestKF = si, si, pKFi
            for pKF2 in self._neighbours(pKFi):
                if pKF2.mnRelocQuery != mnId:
                    continue
                accScore = F32(accScore + pKF2.mRelocScore)
                self.log.append(("best", pKF2.mRelocScore, bestScore))
                if pKF2.mRelocScore > bestScore:
                    pBestKF, bestScore = pKF2, pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return self._finish(lAccScoreAndMatch, bestAccScore, out)


def margin_violations(log, rel=1e-5):
    """The comparisons of a query's log whose sides lie within `rel` relative of each other.  Equal sides are allowed only where identical vectors make them
    so (the `best` comparison of two keyframes' scores): minScore and 0.75f * best are not any keyframe's score."""
    bad = []
    for kind, a, b in log:
        a, b = float(a), float(b)
        if kind == "best" and a == b:
            continue
        if abs(a - b) <= rel * max(abs(a), abs(b)):
            bad.append((kind, a, b))
    return bad


# ---- the generator ----
def l1_vector(rng, words, n):
    """n distinct word ids out of `words` (ascending) with positive values that sum to 1"""
    ids = np.sort(rng.choice(np.asarray(words), n, replace=False)).astype(np.uint32)
    v = rng.random(n) + 0.05
    return ids, (v / v.sum() if n else v).astype(np.float64)


def scene_vector(rng, scene, vocab, lo=30, hi=90, noise=0.2):
    """A vector drawn mostly from the words of `scene`, the rest from anywhere in the vocabulary: keyframes of one scene share many words, others a few."""
    n = int(rng.integers(lo, hi + 1))
    n_sc = min(len(scene), int(round(n * (1.0 - noise))))
    own = rng.choice(scene, n_sc, replace=False)
    rest = np.setdiff1d(np.arange(vocab), own)
    ids = np.sort(np.concatenate([own, rng.choice(rest, n - n_sc, replace=False)])).astype(np.uint32)
    v = rng.random(n) + 0.05
    return ids, v / v.sum()


def make_database(rng, n_kf, vocab=300, n_scenes=3, p_twin=0.15, first_id=0):
    """[(id, ids, vals)] of n_kf keyframes over `n_scenes` scenes of a small vocabulary, some with the very vector of an earlier one (ties), and a
    covisibility list per keyframe (ids of the same database, a few beyond it)."""
    scenes = [rng.choice(vocab, 110, replace=False) for _ in range(n_scenes)]
    kfs = []
    for k in range(n_kf):
        if kfs and rng.random() < p_twin:
            ids, vals = kfs[int(rng.integers(len(kfs)))][1:]
        else:
            ids, vals = scene_vector(rng, scenes[int(rng.integers(n_scenes))], vocab)
        kfs.append((first_id + k, ids, vals))
    covis = []
    for k in range(n_kf):
        m = int(rng.integers(0, 11))
        covis.append((first_id + k, rng.integers(first_id, first_id + n_kf + 3, m).tolist()))
    return kfs, covis, scenes


# ---- scripts: lists of operations that the restatement and the device replay alike ----
# ("add", [(db, kf, ids, vals)]), ("erase", [(db, kf)]), ("clear", [db]), ("covis", [(db, kf, list)]),
# ("reloc", [(db, ids, vals)]), ("loop", [(db, ids, vals, min_score, connected)])
def run_reference(script, dbs=None):
    """Replays `script` on RefDatabases; returns (per operation: None, or one result dict per query, with its log), the databases."""
    dbs = {} if dbs is None else dbs
    out = []
    for op, recs in script:
        res = None
        if op == "add":
            for d, k, ids, vals in recs:
                dbs.setdefault(d, RefDatabase()).add(k, ids, vals)
        elif op == "erase":
            for d, k in recs:
                dbs.setdefault(d, RefDatabase()).erase(k)
        elif op == "clear":
            for d in recs:
                dbs.setdefault(d, RefDatabase()).clear()
        elif op == "covis":
            for d, k, l in recs:
                dbs[d].set_covisibility(k, l)
        elif op == "reloc":
            res = []
            for d, ids, vals in recs:
                db = dbs.setdefault(d, RefDatabase())
                r = db.detect_relocalization_candidates(ids, vals)
                r["log"] = db.log
                res.append(r)
        elif op == "loop":
            res = []
            for d, ids, vals, ms, conn in recs:
                db = dbs.setdefault(d, RefDatabase())
                r = db.detect_loop_candidates(ids, vals, ms, conn)
                r["log"] = db.log
                res.append(r)
        else:
            raise ValueError(op)
        out.append(res)
    return out, dbs


KF_COUNTS = (0, 1, 15, 16, 17, 65)
VEC_SIZES = (0, 1, 15, 16, 17, 255, 256, 257, MAX_WORDS)
N_DATABASES, MAX_KEYFRAMES = 14, 70
BIG_VOCAB = 3000


def fixture_script(seed=20240611):
    """The parity fixture: databases of 0, 1, 15, 16, 17 and 65 keyframes over a 300-word vocabulary (2, 5 and 11 stay unused), database 8 with vectors of 0, 1,
    15, 16, 17, 255, 256, 257 and 2400 words over a 3000-word one, database 9 whose query shares no word, database 10 with an empty query; one batch of reloc
    queries, one of loop queries, then a second batch of reloc queries that meets the scores the first one left."""
    rng = np.random.default_rng(seed)
    db_of = dict(zip(KF_COUNTS, (0, 1, 3, 4, 6, 7)))
    adds, covis, scenes = [], [], {}
    for n_kf, d in db_of.items():
        kfs, cv, sc = make_database(rng, n_kf)
        adds += [(d, k, i, v) for k, i, v in kfs]
        covis += [(d, k, l) for k, l in cv]
        scenes[d] = sc
    big = np.arange(BIG_VOCAB)
    core = rng.choice(BIG_VOCAB, 1200, replace=False)   # what the large vectors of database 8 have in common
    for k, n in enumerate(VEC_SIZES):
        words = core if 0 < n <= len(core) and n >= 255 else big
        ids, vals = l1_vector(rng, words, n)
        adds.append((8, k, ids, vals))
    adds += [(8, len(VEC_SIZES) + j, *l1_vector(rng, core, 900 + 50 * j)) for j in range(3)]
    covis += [(8, k, rng.integers(0, len(VEC_SIZES) + 3, 6).tolist()) for k in range(len(VEC_SIZES) + 3)]
    for d in (9, 10):
        kfs, cv, sc = make_database(rng, 20)
        adds += [(d, k, i, v) for k, i, v in kfs]
        covis += [(d, k, l) for k, l in cv]
        scenes[d] = sc

    def queries(sizes):
        q = []
        for d in (0, 1, 3, 4, 6, 7):
            sc = scenes[d]
            q.append((d,) + tuple(scene_vector(rng, sc[int(rng.integers(len(sc)))], 300, 40, 100)))
        q.append((8,) + l1_vector(rng, np.concatenate([core, np.setdiff1d(big, core)[:sizes - len(core)]]) if sizes > len(core) else core, sizes))
        q.append((9,) + l1_vector(rng, np.arange(1000, 1100), 60))   # beyond the 300 words database 9 uses
        q.append((10,) + l1_vector(rng, big, 0))
        return q

    def with_loop_fields(q):
        out = []
        for d, ids, vals in q:
            n = {0: 0, 1: 1, 3: 15, 4: 16, 6: 17, 7: 65, 8: len(VEC_SIZES) + 3, 9: 20, 10: 20}[d]
            conn = rng.choice(n + 2, min(n + 2, int(rng.integers(0, 6))), replace=False).tolist()   # (some of them not present)
            out.append((d, ids, vals, float(rng.uniform(0.3, 0.42)), conn))
        return out

    return [("add", adds), ("covis", covis), ("reloc", queries(MAX_WORDS)), ("loop", with_loop_fields(queries(1000))), ("reloc", queries(257))]


@functools.lru_cache(maxsize=None)
def fixture():
    """(script, expected) of the parity fixture, computed once and shared by the tests; nobody changes it."""
    script = fixture_script()
    expected, _ = run_reference(script)
    return script, expected


def state_script(seed=77):
    """add / erase / clear / set_covisibility interleaved with queries on three databases; the reloc queries come in consecutive calls so that a keyframe that
    is reached but not scored contributes what an earlier call left in it; keyframes are erased and added again under the same id."""
    rng = np.random.default_rng(seed)
    script = []
    scenes = {}
    for d in (0, 2, 3):
        kfs, cv, scenes[d] = make_database(rng, 24)
        script.append(("add", [(d, k, i, v) for k, i, v in kfs]))
        script.append(("covis", [(d, k, l) for k, l in cv]))

    def q(d):
        sc = scenes[d]
        return (d,) + tuple(scene_vector(rng, sc[int(rng.integers(len(sc)))], 300, 40, 100))

    for it in range(4):
        script.append(("reloc", [q(0), q(2), q(3)]))
        script.append(("loop", [q(d) + (float(rng.uniform(0.28, 0.42)), rng.choice(26, 3, replace=False).tolist()) for d in (3, 0)]))
        gone = rng.choice(24, 5, replace=False).tolist()
        script.append(("erase", [(0, k) for k in gone] + [(2, gone[0])]))
        script.append(("reloc", [q(0), q(2)]))
        back = [(0, k) + tuple(scene_vector(rng, scenes[0][int(rng.integers(3))], 300)) for k in gone[:3]]   # the same ids, other vectors, new serials
        script.append(("add", back))
        script.append(("covis", [(0, k, rng.integers(0, 26, int(rng.integers(0, 11))).tolist()) for k, *_ in [b[1:] for b in back]]))
        if it == 2:
            script.append(("clear", [3]))
            script.append(("reloc", [q(3), q(0)]))
            kfs, cv, scenes[3] = make_database(rng, 10)
            script.append(("add", [(3, k, i, v) for k, i, v in kfs]))
            script.append(("covis", [(3, k, [x for x in l if x < 12]) for k, l in cv]))
    script.append(("reloc", [q(0), q(2), q(3)]))
    return script


@functools.lru_cache(maxsize=None)
def state_fixture():
    script = state_script()
    expected, _ = run_reference(script)
    return script, expected


def identity_script(seed=5):
    """64 databases of 12 keyframes; one batch of 64 loop queries and one of 64 reloc queries (the bit-identity test runs query 37 alone as well)."""
    rng = np.random.default_rng(seed)
    adds, covis, loops, relocs = [], [], [], []
    for d in range(64):
        kfs, cv, sc = make_database(rng, 12)
        adds += [(d, k, i, v) for k, i, v in kfs]
        covis += [(d, k, [x for x in l if x < 16]) for k, l in cv]
        q = scene_vector(rng, sc[0], 300, 40, 100)
        loops.append((d,) + q + (float(rng.uniform(0.28, 0.42)), rng.choice(12, 2, replace=False).tolist()))
        relocs.append((d,) + scene_vector(rng, sc[1], 300, 40, 100))
    return [("add", adds), ("covis", covis), ("loop", loops), ("reloc", relocs)]


@functools.lru_cache(maxsize=None)
def identity_fixture():
    script = identity_script()
    expected, _ = run_reference(script)
    return script, expected


N_REFUSALS = 12


def refusal_script(seed=9):
    """One database of 16 keyframes (database 1 of 2) and the same pair of queries, reloc then loop, N_REFUSALS + 1 times over: the refusal test puts a call
    that must be refused between them, and the state the queries see is the one the restatement has."""
    rng = np.random.default_rng(seed)
    kfs, cv, sc = make_database(rng, 16)
    qr = (1,) + scene_vector(rng, sc[0], 300, 40, 100)
    ql = (1,) + scene_vector(rng, sc[1], 300, 40, 100) + (0.35, [2, 5])
    script = [("add", [(1, k, i, v) for k, i, v in kfs]), ("covis", [(1, k, [x for x in l if x < 16]) for k, l in cv])]
    for _ in range(N_REFUSALS + 1):
        script += [("reloc", [qr]), ("loop", [ql])]
    return script


@functools.lru_cache(maxsize=None)
def refusal_fixture():
    script = refusal_script()
    expected, _ = run_reference(script)
    return script, expected
