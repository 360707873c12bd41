// A caller of ORB_SLAM2::KeyFrameDatabase written only against include/orb_slam2_adapter.hpp: one database that keyframes are added to and erased from, and
// the two queries Tracking::Relocalization (src/Tracking.cc:1616) and LoopClosing::DetectLoop (src/LoopClosing.cc:143) make.  Reads <dir>/voc.txt and
// <dir>/ops.txt, one operation per line:
//   A <mnId> <n> {<word> <value>} x n <m> {<covisible id>} x m      add
//   E <mnId>                                                         erase
//   C                                                                clear
//   R <mnId> <n> {<word> <value>} x n                                DetectRelocalizationCandidates
//   L <mnId> <n> {<word> <value>} x n <minScore> <m> {<connected id>} x m   DetectLoopCandidates
// and prints per query one line: "R|L <n_cand> {<id> <accumulated score>} x n_cand | <5 diagnostics> [| <score of each connected id>]", floats as %.9g.
// tests/test_keyframe_db_gpu.py builds it, runs it and compares the lines with the Python view's.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "orb_slam2_adapter.hpp"

static DBoW2::BowVector read_bow(std::istream& in) {
    DBoW2::BowVector v;
    int n = 0;
    in >> n;
    for (int i = 0; i < n; i++) {
        unsigned w; double x;
        in >> w >> x;
        v[w] = x;
    }
    return v;
}

static std::vector<int32_t> read_ids(std::istream& in) {
    int m = 0;
    in >> m;
    std::vector<int32_t> ids(m);
    for (int i = 0; i < m; i++) in >> ids[i];
    return ids;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const std::string d = argv[1];
    try {
        ORB_SLAM2::ORBVocabulary voc;
        if (!voc.loadFromTextFile(d + "/voc.txt")) throw std::runtime_error(std::string("vocabulary: ") + oslam_last_error());
        ORB_SLAM2::KeyFrameDatabase db(voc, atoi(argv[2]), atoi(argv[3]));
        std::ifstream f(d + "/ops.txt");
        std::string line;
        while (std::getline(f, line)) {
            std::istringstream in(line);
            char op = 0;
            in >> op;
            if (op == 'C') { db.clear(); continue; }
            ORB_SLAM2::KeyFrameDatabaseKeyFrameView KF;
            in >> KF.mnId;
            if (op == 'E') { db.erase(KF); continue; }
            const DBoW2::BowVector bow = read_bow(in);
            KF.mBowVec = &bow;
            if (op == 'A') {
                KF.vpBestCovisibles = read_ids(in);
                db.add(KF);
                continue;
            }
            std::vector<int32_t> cand;
            std::vector<float> cs;
            if (op == 'R') cand = db.DetectRelocalizationCandidates(KF.mnId, bow);
            else if (op == 'L') {
                float minScore = 0.f;
                in >> minScore;
                KF.spConnected = read_ids(in);
                cand = db.DetectLoopCandidates(KF, minScore, &cs);
            } else throw std::runtime_error("ops.txt: unknown operation");
            printf("%c %zu", op, cand.size());
            for (size_t i = 0; i < cand.size(); i++) printf(" %d %.9g", cand[i], db.accumulatedScores()[i]);
            printf(" |");
            for (int i = 0; i < 5; i++) printf(" %d", db.diagnostics()[i]);
            if (op == 'L') { printf(" |"); for (float s : cs) printf(" %.9g", s); }
            printf("\n");
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
