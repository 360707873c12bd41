// Host-side unit checks of the map storage (object_slam_amd/csrc/seq_arena.h and the observation lists of csrc/slam_map.h): list operations across every
// capacity boundary, reuse of freed blocks, chunks returned on a map reset, and a seeded differential run of the four list-changing functions against a
// std::vector restatement.  No GPU, no oracle.  Built twice by tests/test_seq_arena_cpu.py: as it is, and with -fsanitize=address,undefined
// -DOSLAM_ARENA_PASSTHROUGH (every block a malloc block with exact bounds; the checks of the arena's own bookkeeping are compiled out there).
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../object_slam_amd/csrc/slam_map.h"

using namespace oslam_drv;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int add_kf(Map& m, int nkp, std::mt19937& rng) {
    m.kfs.emplace_back();
    KeyFrm& k = m.kfs.back();
    k.id = (int)m.kfs.size() - 1; k.frameId = k.id; k.N = nkp;
    k.keys.resize(nkp); k.keysUn.resize(nkp); k.uRight.resize(nkp); k.depth.assign(nkp, 1.f);
    for (int i = 0; i < nkp; i++) {
        k.keysUn[i].x = (float)(k.id * 1000 + i); k.keysUn[i].y = (float)(i * 7 - k.id);
        k.keysUn[i].octave = (int)(rng() % 8);
        k.uRight[i] = (rng() % 3) ? (float)(k.id + i) : -1.f;   // a third of the keypoints are monocular
    }
    k.mp.assign(nkp, -1);
    return k.id;
}

// ---- the std::vector restatement (the lists as two parallel vectors; same order of journal events) ----
struct ModelPt { std::vector<std::pair<int, int>> obs; std::vector<ObsKp> okp; int nObs = 0; uint64_t lvl = 0; int bad = 0, replaced = -1, refKF = -1, obsVer = 0; };
struct Model {
    std::vector<ModelPt> pts;
    std::vector<std::vector<int>> kfmp;
    std::vector<uint32_t> ev;
    const Map* geo = nullptr;   // keypoints are read from the map's keyframes (never changed)
    void jr(int set, int kf, int idx, int p) { ev.push_back((uint32_t)kf); ev.push_back((uint32_t)idx | (set ? 0x80000000u : 0u)); ev.push_back((uint32_t)p); }
    void add(int p, int kf, int idx) {
        ModelPt& m = pts[p];
        size_t at = 0;
        while (at < m.obs.size() && m.obs[at].first < kf) at++;
        if (at < m.obs.size() && m.obs[at].first == kf) return;
        const KeyFrm& k = geo->kfs[kf];
        const ObsKp o = {k.keysUn[idx].x, k.keysUn[idx].y, k.uRight[idx], k.keysUn[idx].octave};
        m.obs.insert(m.obs.begin() + at, std::make_pair(kf, idx));
        m.okp.insert(m.okp.begin() + at, o);
        m.lvl += 1ull << (8 * o.octave);
        m.nObs += o.ur >= 0 ? 2 : 1;
        m.obsVer++;
        jr(1, kf, idx, p);
    }
    void set_bad(int p) {
        ModelPt& m = pts[p];
        m.bad = 1;
        std::vector<std::pair<int, int>> o;
        o.swap(m.obs); m.okp.clear(); m.lvl = 0;
        for (auto& e : o) { kfmp[e.first][e.second] = -1; jr(0, e.first, e.second, p); }
    }
    void erase(int p, int kf) {
        ModelPt& m = pts[p];
        bool bad = false;
        for (size_t i = 0; i < m.obs.size(); i++)
            if (m.obs[i].first == kf) {
                m.nObs -= m.okp[i].ur >= 0 ? 2 : 1;
                jr(0, kf, m.obs[i].second, p);
                m.lvl -= 1ull << (8 * m.okp[i].octave);
                m.obs.erase(m.obs.begin() + i); m.okp.erase(m.okp.begin() + i);
                m.obsVer++;
                if (m.refKF == kf && !m.obs.empty()) m.refKF = m.obs.front().first;
                if (m.nObs <= 2) bad = true;
                break;
            }
        if (bad) set_bad(p);
    }
    bool replace(int p, int by) {
        if (p == by) return false;
        ModelPt& m = pts[p];
        std::vector<std::pair<int, int>> o;
        o.swap(m.obs); m.okp.clear(); m.lvl = 0;
        m.bad = 1; m.replaced = by;
        for (auto& e : o) {
            jr(0, e.first, e.second, p);
            bool in = false;
            for (auto& f : pts[by].obs) in |= f.first == e.first;
            if (!in) { kfmp[e.first][e.second] = by; add(by, e.first, e.second); }
            else kfmp[e.first][e.second] = -1;
        }
        return true;
    }
};

static bool same_list(const MapPt& a, const ModelPt& b) {
    if (a.obs.size() != b.obs.size() || a.okp.size() != b.okp.size() || a.obs.empty() != b.obs.empty()) return false;
    for (size_t i = 0; i < b.obs.size(); i++) {
        if (a.obs[i] != b.obs[i]) return false;
        if (a.okp[i].x != b.okp[i].x || a.okp[i].y != b.okp[i].y || a.okp[i].ur != b.okp[i].ur || a.okp[i].octave != b.okp[i].octave) return false;
    }
    size_t n = 0;
    for (auto& e : a.obs) { if (e != b.obs[n]) return false; n++; }
    return n == b.obs.size() && (b.obs.empty() || (a.obs.front() == b.obs.front() && a.obs.data() == &a.obs[0] && a.okp.data() == &a.okp[0]));
}

static int list_operations() {
    std::mt19937 rng(7);
    Map m;
    const int NKF = 300;
    for (int k = 0; k < NKF; k++) add_kf(m, 4, rng);
    Model md; md.geo = &m; md.pts.resize(1); md.kfmp.assign(NKF, std::vector<int>(4, -1));
    const float x[3] = {0, 0, 1};
    const int p = m.new_point(x, 0, 0);
    CHECK(m.mps[p].obs.empty() && m.mps[p].okp.empty() && m.mps[p].obs.begin() == m.mps[p].obs.end());
    // back, front, middle; then growth over every capacity boundary up to 256 (the fused update kernel refuses more than 128 observations, so the driver
    // does hold such lists): keyframes in an order that keeps inserting at the front, in the middle and at the back
    std::vector<int> order = {100, 50, 150, 75, 125};
    for (int k = 0; k < NKF; k++) if (k != 100 && k != 50 && k != 150 && k != 75 && k != 125) order.push_back(k);
    std::shuffle(order.begin() + 5, order.end(), rng);
    uint32_t lastCap = 0;
    int grows = 0;
    for (size_t i = 0; i < 200; i++) {
        const int kf = order[i], idx = (int)(rng() % 4);
        m.add_observation(p, kf, idx); md.add(0, kf, idx);
        CHECK(same_list(m.mps[p], md.pts[0]));
        CHECK(m.pNObs[p] == md.pts[0].nObs && m.pLvl[p] == md.pts[0].lvl);
        const uint32_t cap = m.mps[p].lst.cap;
        CHECK(cap >= m.mps[p].lst.n && (cap & (cap - 1)) == 0);
        if (cap != lastCap) { CHECK(lastCap == 0 ? cap == 2 : cap == 2 * lastCap); lastCap = cap; grows++; }
        m.add_observation(p, kf, idx); md.add(0, kf, idx);   // a second observation from the same keyframe is refused
        CHECK(same_list(m.mps[p], md.pts[0]));
    }
    CHECK(m.mps[p].obs.size() == 200 && lastCap == 256 && grows == 8 && !m.lvlOverflow);
    // erase first, middle, last
    const int first = m.mps[p].obs[0].first, mid = m.mps[p].obs[100].first, last = m.mps[p].obs[199].first;
    m.mps[p].refKF = first; md.pts[0].refKF = first;
    for (int kf : {first, mid, last}) {
        m.erase_observation(p, kf); md.erase(0, kf);
        CHECK(same_list(m.mps[p], md.pts[0]) && m.pNObs[p] == md.pts[0].nObs && m.pLvl[p] == md.pts[0].lvl && m.mps[p].refKF == md.pts[0].refKF);
    }
    CHECK(m.mps[p].obs.size() == 197 && m.mps[p].lst.cap == 256);
    m.erase_observation(p, 9999);   // not an observer
    CHECK(same_list(m.mps[p], md.pts[0]));
    while (m.mps[p].obs.size() > 0 && !m.pBad[p]) { const int kf = m.mps[p].obs[m.mps[p].obs.size() / 2].first; m.erase_observation(p, kf); md.erase(0, kf); CHECK(same_list(m.mps[p], md.pts[0])); }
    CHECK(m.pBad[p] && md.pts[0].bad && m.mps[p].obs.empty() && m.mps[p].lst.blk == nullptr && m.mps[p].lst.cap == 0);
    return 0;
}

#ifndef OSLAM_ARENA_PASSTHROUGH
static int block_reuse() {
    for (size_t b = 1; b <= SeqArena::kMaxSmall; b += (b < 512 ? 1 : 509)) {   // every request fits its class, and the class below does not hold it
        const int c = SeqArena::class_of(b);
        CHECK(c >= 0 && c < SeqArena::kClasses && SeqArena::class_bytes(c) >= b && (c == 0 || SeqArena::class_bytes(c - 1) < b));
    }
    for (uint32_t cap = 2; cap <= 1024; cap *= 2) CHECK(SeqArena::class_bytes(SeqArena::class_of(obs_block_bytes(cap))) == obs_block_bytes(cap));   // no slack in a list block
    SeqArena a;
    void* p = a.alloc(96);
    void* q = a.alloc(96);
    CHECK(p != q && ((uintptr_t)p & 15) == 0);
    a.dealloc(p, 96);
    CHECK(a.alloc(90) == p);          // same class
    a.dealloc(q, 96); a.dealloc(p, 96);
    CHECK(a.alloc(96) == p && a.alloc(96) == q);   // last freed first
    void* big = a.alloc(SeqArena::kMaxSmall);
    CHECK(((uintptr_t)big & 63) == 0);
    // through the map: the block of a point that went bad serves the next list that reaches its capacity
    std::mt19937 rng(3);
    Map m;
    for (int k = 0; k < 8; k++) add_kf(m, 4, rng);
    const float x[3] = {0, 0, 1};
    const int p0 = m.new_point(x, 0, 0), p1 = m.new_point(x, 0, 0);
    for (int k = 0; k < 3; k++) m.add_observation(p0, k, 0);
    CHECK(m.mps[p0].lst.cap == 4);
    const char* blk = m.mps[p0].lst.blk;
    m.set_bad_point(p0);
    for (int k = 0; k < 3; k++) m.add_observation(p1, k, 1);
    CHECK(m.mps[p1].lst.cap == 4 && m.mps[p1].lst.blk == blk);
    return 0;
}

static int arena_reset() {
    std::mt19937 rng(5);
    const float x[3] = {0, 0, 1};
    auto fill = [&](Map& m) {
        for (int k = 0; k < 16; k++) add_kf(m, 8, rng);
        for (int p = 0; p < 3000; p++) { m.new_point(x, 0, 0); for (int k = 0; k < 1 + p % 9; k++) m.add_observation(p, (p + k) % 16, p % 8); }
    };
    Map m;
    fill(m);
    const size_t held = m.arena.chunks_held();
    CHECK(held * kArenaChunk >= 3000 * sizeof(MapPt));   // (the point records alone)
    const SlabPoolStats s0 = SlabPool::instance().stats();
    m = Map();          // Seq::reset, with live lists
    const SlabPoolStats s1 = SlabPool::instance().stats();
    CHECK(m.arena.chunks_held() == 0 && m.mps.size() == 0 && m.pNObs.size() == 0);
    CHECK(s1.chunks_free == s0.chunks_free + held && s1.chunks_carved == s0.chunks_carved && s1.slabs == s0.slabs);
    {
        Map m2;
        fill(m2);
        const SlabPoolStats s2 = SlabPool::instance().stats();
        CHECK(m2.arena.chunks_held() == held);                                            // the same work takes the same chunks ...
        CHECK(s2.chunks_carved == s1.chunks_carved && s2.chunks_free == s1.chunks_free - held);   // ... and all of them come from the free list
        Map m3(std::move(m2));                                                            // a moved map keeps its blocks
        CHECK(m2.arena.chunks_held() == 0 && m3.arena.chunks_held() == held && m3.mps[2999].obs.size() == 1 + 2999 % 9);
    }
    const SlabPoolStats s3 = SlabPool::instance().stats();
    CHECK(s3.chunks_free == s1.chunks_free && s3.chunks_carved == s1.chunks_carved);      // the destructor returned them
    return 0;
}
#endif

static int differential() {
    std::mt19937 rng(20240607);
    const int NP = 64, NKF = 16, NKP = 32, OPS = 120000;
    Map m;
    for (int k = 0; k < NKF; k++) add_kf(m, NKP, rng);
    m.jrOn = true;
    Model md; md.geo = &m; md.pts.resize(NP); md.kfmp.assign(NKF, std::vector<int>(NKP, -1));
    const float x[3] = {0, 0, 1};
    for (int p = 0; p < NP; p++) { m.new_point(x, 0, 0); md.pts[p].refKF = m.mps[p].refKF; }
    long long nadd = 0, nerase = 0, nbad = 0, nrep = 0;
    for (int it = 0; it < OPS; it++) {
        const int r = (int)(rng() % 100), p = (int)(rng() % NP), kf = (int)(rng() % NKF), idx = (int)(rng() % NKP);
        if (r < 58) { m.add_observation(p, kf, idx); m.set_kf_mp(kf, idx, p); md.add(p, kf, idx); md.kfmp[kf][idx] = p; nadd++; }
        else if (r < 88) { m.erase_observation(p, kf); md.erase(p, kf); nerase++; }
        else if (r < 90) { m.set_bad_point(p); md.set_bad(p); nbad++; }
        else { const int by = (int)(rng() % NP); CHECK(m.replace_point(p, by) == md.replace(p, by)); m.pFound[by] = m.pVisible[by] = 1; nrep++; }   // (the counters Replace sums are not lists: kept from doubling out of an int)
        for (int q = 0; q < NP; q++) {
            CHECK(same_list(m.mps[q], md.pts[q]));
            CHECK(m.pNObs[q] == md.pts[q].nObs && m.pLvl[q] == md.pts[q].lvl && m.pBad[q] == md.pts[q].bad && m.pReplaced[q] == md.pts[q].replaced);
            CHECK(m.mps[q].obsVer == md.pts[q].obsVer && m.mps[q].refKF == md.pts[q].refKF);
        }
        if (it % 512 == 511) {
            for (int k = 0; k < NKF; k++) CHECK(m.kfs[k].mp == md.kfmp[k]);
            CHECK(m.jrOkf == md.ev);   // the journal's AddObservation / EraseObservation events, in program order
            m.jrOkf.clear(); md.ev.clear(); m.jrCells.clear();
        }
    }
    CHECK(!m.lvlOverflow && nadd > 50000 && nerase > 25000 && nbad > 1000 && nrep > 8000);
    printf("differential: %d calls (%lld add, %lld erase, %lld bad, %lld replace), %zu arena chunks\n", OPS, nadd, nerase, nbad, nrep, m.arena.chunks_held());
    return 0;
}

int main() {
    if (list_operations()) return 1;
#ifndef OSLAM_ARENA_PASSTHROUGH
    if (block_reuse()) return 1;
    if (arena_reset()) return 1;
#endif
    if (differential()) return 1;
    printf("seq_arena_check ok\n");
    return 0;
}
