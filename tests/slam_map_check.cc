// Host-side unit checks of the driver's map bookkeeping (object_slam_amd/csrc/slam_map.h) against the behaviour of the reference's
// KeyFrame / MapPoint methods (src/KeyFrame.cc:123-567, src/MapPoint.cc:196-318), on a hand-built map.  No GPU, no oracle.
// `slam_map_check replay <script>` replays a scripted operation sequence with the change log on and prints the arrays of Map::journal_changes at every flush
// (tests/test_mirror_cases_cpu.py compares them with the change sets of the Python model of tests/mirror_common.py, which feeds the device mirror's tests).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../object_slam_amd/csrc/slam_map.h"

using namespace oslam_drv;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int add_kf(Map& m, int nkp, bool stereo) {
    m.kfs.emplace_back();
    KeyFrm& k = m.kfs.back();
    k.id = (int)m.kfs.size() - 1; k.frameId = k.id * 5; k.N = nkp;
    k.keys.resize(nkp); k.keysUn.resize(nkp); k.desc.assign((size_t)nkp * 32, 0); k.uRight.assign(nkp, stereo ? 10.f : -1.f); k.depth.assign(nkp, stereo ? 2.f : -1.f);
    for (int i = 0; i < nkp; i++) { k.keysUn[i].octave = 0; k.keys[i].octave = 0; }
    k.mp.assign(nkp, -1);
    M4 T = eye4(); T.m[3] = -0.1f * k.id;
    k.pose.set_keyframe(T);
    k.Tcp = eye4();
    m.nKFsInMap++;
    return k.id;
}
static void observe(Map& m, int p, int kf, int idx) { m.add_observation(p, kf, idx); m.kfs[kf].mp[idx] = p; }

// One operation per line (tests/mirror_common.py REPLAY_SCRIPT): K kf | P | A p kf idx | M kf idx p | E p kf | B p | R p q | X kf | Z | F.  Keypoint i of every
// keyframe: octave i % 8; class (i / 8) % 5: 0-2 stereo at 2 m, 3 stereo at 100 m (beyond mThDepth), 4 no depth.
static int replay(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    const int NK = 64;
    const float thDepth = 40.0f * 40.0f / 520.908620f;
    Map m;
    m.jrOn = true;
    Map::JrScratch sc;
    char op[8];
    while (fscanf(f, "%7s", op) == 1) {
        int a = 0, b = 0, c = 0;
        switch (op[0]) {
        case 'K': {
            if (fscanf(f, "%d", &a) != 1) return 2;
            CHECK(a == (int)m.kfs.size());
            add_kf(m, NK, true);
            KeyFrm& k = m.kfs.back();
            for (int i = 0; i < NK; i++) {
                const int cls = (i / 8) % 5;
                k.keysUn[i].octave = k.keys[i].octave = i % 8;
                k.uRight[i] = cls == 4 ? -1.f : 10.f; k.depth[i] = cls == 4 ? -1.f : (cls == 3 ? 100.f : 2.f);
            }
            if (k.id > 0) { k.parent = 0; m.kfs[0].children.insert(k.id); }
            m.jr_new_kf(k.id);
            break; }
        case 'P': { const float x[3] = {0, 0, 2}; m.new_point(x, 0, 0); m.nMPsInMap++; break; }
        case 'A': if (fscanf(f, "%d %d %d", &a, &b, &c) != 3) return 2; m.add_observation(a, b, c); break;
        case 'M': if (fscanf(f, "%d %d %d", &a, &b, &c) != 3) return 2; m.set_kf_mp(a, b, c); break;
        case 'E': if (fscanf(f, "%d %d", &a, &b) != 2) return 2; m.erase_observation(a, b); break;
        case 'B': if (fscanf(f, "%d", &a) != 1) return 2; m.set_bad_point(a); break;
        case 'R': if (fscanf(f, "%d %d", &a, &b) != 2) return 2; m.replace_point(a, b); break;
        case 'X': if (fscanf(f, "%d", &a) != 1) return 2; m.set_bad_keyframe(a); break;
        case 'Z': m = Map(); m.jrOn = true; m.jrReset = true; break;   // (Seq::reset of csrc/slam_driver.hip)
        case 'F': {
            oslam_map_changes_t ch;
            m.journal_changes(0, thDepth, sc, ch);
            printf("flush reset=%d\n", ch.reset);
            for (int k = 0; k < ch.n_new; k++) {
                const oslam_map_new_kf_t& e = ch.new_kfs[k];
                printf("new %d %d :", e.kf, e.N);
                for (int i = 0; i < e.N; i++) printf(" %d", e.mp[i]);
                printf(" :");
                for (int i = 0; i < (e.N + 31) / 32; i++) printf(" %u", e.good[i]);
                printf("\n");
            }
            for (int i = 0; i < ch.n_cells; i++) printf("cell %d %d %d\n", ch.cells[3 * i], ch.cells[3 * i + 1], ch.cells[3 * i + 2]);
            for (int i = 0; i < ch.n_events; i++) printf("event %u %u %u\n", ch.events[3 * i], ch.events[3 * i + 1], ch.events[3 * i + 2]);
            for (int i = 0; i < ch.n_points; i++) printf("point %u %u %u %u %u\n", ch.points[5 * i], ch.points[5 * i + 1], ch.points[5 * i + 2], ch.points[5 * i + 3], ch.points[5 * i + 4]);
            CHECK(!m.lvlOverflow);
            break; }
        default: fprintf(stderr, "bad operation %s\n", op); return 2;
        }
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "replay")) return replay(argv[2]);
    Map m;
    std::vector<int> counter(64, 0);
    const int NK = 50;   // slots 40..49 stay free for the single-point scenarios
    for (int k = 0; k < 5; k++) add_kf(m, NK, true);
    // points 0..19 seen by keyframes 0,1,2; points 20..39 seen by 1,2,3,4; point 40 only by 4 and 3
    const float x[3] = {0, 0, 2};
    for (int p = 0; p < 41; p++) { m.new_point(x, 0, 0); m.nMPsInMap++; }
    for (int p = 0; p < 20; p++) for (int k = 0; k <= 2; k++) observe(m, p, k, p);
    for (int p = 20; p < 40; p++) for (int k = 1; k <= 4; k++) observe(m, p, k, p);
    CHECK(m.pNObs[0] == 6);     // stereo observations count twice (src/MapPoint.cc:203-206)
    CHECK(m.pNObs[20] == 8);
    for (int k = 0; k < 5; k++) m.update_connections(k, counter);
    for (int v : counter) CHECK(v == 0);
    // weights: (0,1)=20 (0,2)=20 (1,2)=40 (1,3)=20 (1,4)=20 (2,3)=20 (2,4)=20 (3,4)=20
    CHECK(m.weight(1, 2) == 40 && m.weight(2, 1) == 40 && m.weight(0, 3) == 0 && m.weight(3, 4) == 20);
    // ordered by descending (weight, id): keyframe 1 sees 2 (40) first, then ids 4, 3, 0 (20 each)
    CHECK(m.kfs[1].ordered.size() == 4 && m.kfs[1].ordered[0] == 2 && m.kfs[1].ordered[1] == 4 && m.kfs[1].ordered[2] == 3 && m.kfs[1].ordered[3] == 0);
    // spanning tree (first connection, src/KeyFrame.cc:371-376): 1 -> 0 (only keyframe 0 existed with links when 1 connected)
    CHECK(m.kfs[0].parent == -1);
    CHECK(m.kfs[1].parent == 2 || m.kfs[1].parent == 0);   // all observations already present in this construction: best covisible
    CHECK(m.kfs[3].parent >= 0 && m.kfs[m.kfs[3].parent].children.count(3) == 1);
    // th = 15: a link below the threshold only survives as the single best link (src/KeyFrame.cc:348-352)
    const int k5 = add_kf(m, NK, true);
    for (int p = 0; p < 5; p++) observe(m, p, k5, p);
    m.update_connections(k5, counter);
    CHECK(m.kfs[k5].ordered.size() == 1 && m.kfs[k5].orderedW[0] == 5);
    CHECK(m.kfs[k5].connW.size() == 3);   // mConnectedKeyFrameWeights keeps every counter (KFcounter), :367
    // erase_observation: refKF moves to the first remaining observer; <= 2 observations left -> point culled (src/MapPoint.cc:209-239)
    // (free slot 38 of keyframes 3 and 4 first: point 38 loses two stereo observations)
    m.erase_observation(38, 3); m.erase_observation(38, 4);
    CHECK(m.pNObs[38] == 4 && !m.pBad[38] && m.kfs[3].mp[38] == 38);   // EraseObservation does not touch the keyframe slot; the caller does (src/Optimizer.cc:752-753)
    m.kfs[3].mp[38] = -1; m.kfs[4].mp[38] = -1;
    m.kfs[3].uRight[38] = -1.f; m.kfs[4].uRight[38] = -1.f;   // two monocular observations: nObs = 2
    observe(m, 40, 3, 38); observe(m, 40, 4, 38);
    m.mps[40].refKF = 3;
    CHECK(m.pNObs[40] == 2);
    m.erase_observation(40, 3);
    CHECK(m.pBad[40] && m.mps[40].obs.empty() && m.kfs[4].mp[38] == -1);   // nObs <= 2 -> SetBadFlag clears the remaining slot
    // Replace (src/MapPoint.cc:279-318): observations move unless the target is already in that keyframe
    const int pa = m.new_point(x, 0, 0), pb = m.new_point(x, 0, 0);
    m.nMPsInMap += 2;
    observe(m, pa, 0, 45); observe(m, pa, 1, 46); observe(m, pb, 1, 47); observe(m, pb, 2, 48);
    m.pFound[pa] = 3; m.pVisible[pa] = 7;
    const int f0 = m.pFound[pb], v0 = m.pVisible[pb];
    CHECK(m.replace_point(pa, pb));
    CHECK(m.pBad[pa] && m.pReplaced[pa] == pb && m.mps[pa].obs.empty());
    CHECK(m.kfs[0].mp[45] == pb && m.kfs[1].mp[46] == -1 && m.kfs[1].mp[47] == pb);   // keyframe 1 already observed pb: pa's slot is erased
    CHECK(m.mps[pb].obs.size() == 3 && m.pFound[pb] == f0 + 3 && m.pVisible[pb] == v0 + 7);
    // SetBadFlag of keyframe 2 (src/KeyFrame.cc:453-545): links and observations removed, children re-attached, mTcp stored, id 0 is immune
    const int nk = m.nKFsInMap;
    m.set_bad_keyframe(0);
    CHECK(!m.kfs[0].bad && m.nKFsInMap == nk);
    const int par2 = m.kfs[2].parent;
    std::set<int> ch2 = m.kfs[2].children;
    m.set_bad_keyframe(2);
    CHECK(m.kfs[2].bad && m.nKFsInMap == nk - 1 && m.kfs[2].ordered.empty() && m.kfs[2].connW.empty());
    for (int k = 0; k < (int)m.kfs.size(); k++) {
        if (k == 2) continue;
        // keyframe 5 keeps its one-sided counter for keyframe 2: mConnectedKeyFrameWeights = KFcounter holds every co-observer (src/KeyFrame.cc:367) while
        // only links >= 15 (or the single best) are mirrored (:341-352), and SetBadFlag erases the mirrored ones (:466-467)
        if (k != k5) CHECK(m.weight(k, 2) == 0);
        else CHECK(m.weight(k, 2) == 5);
        for (int o : m.kfs[k].ordered) CHECK(o != 2);
        if (m.kfs[k].parent >= 0) CHECK(!m.kfs[m.kfs[k].parent].bad);
    }
    for (int c : ch2) CHECK(m.kfs[c].parent != 2 && m.kfs[c].parent >= 0);
    if (par2 >= 0) CHECK(m.kfs[par2].children.count(2) == 0);
    for (int p = 0; p < 40; p++) CHECK(m.mps[p].obs_index(2) < 0);
    // points 0..19 had observers 0,1,2 (+5 for the first five): after losing keyframe 2 they keep nObs = 4 (or 6)
    CHECK(m.pNObs[10] == 4 && !m.pBad[10] && m.pNObs[0] == 6);
    // Tcp = Tcw * parent.Twc
    const M4 Tcp = mul4(m.kfs[2].pose.Tcw, m.kfs[par2].pose.Twc);
    for (int i = 0; i < 16; i++) CHECK(m.kfs[2].Tcp.m[i] == Tcp.m[i]);
    printf("slam_map_check ok\n");
    return 0;
}
