// A caller of ORB_SLAM2::LoopClosing::DetectLoop written only against include/orb_slam2_adapter.hpp: one sequence whose keyframes arrive one after the other,
// as LocalMapping hands them to LoopClosing (src/LoopClosing.cc:104-230).  Reads <dir>/voc.txt and <dir>/ops.txt, one operation per line:
//   S <mnId> <m> {<connected id>} x m                                          SetConnectedKeyFrames
//   V <mnId> <m> {<covisible id>} x m                                          KeyFrameDatabase::UpdateCovisibility of a keyframe that is in the database
//   M <id>                                                                     mLastLoopKFid = id (what CorrectLoop does, :585)
//   D <mnId> <n> {<word> <value>} x n <m> {<connected id>} x m <c> {<best covisible id>} x c      DetectLoop
// and prints per D one line: "D <mnId> 0 gated" when the +10 gate (:115) answered, otherwise
// "D <mnId> <0|1> <n_enough> {<id>} | <n_cand> {<id>} | <minScore %.9g> | <groups>".
// tests/test_loop_detect_gpu.py builds it, runs it and compares the lines with the Python view's.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "orb_slam2_adapter.hpp"

static std::vector<int32_t> read_ids(std::istream& in) {
    int m = 0;
    in >> m;
    std::vector<int32_t> ids(m);
    for (int i = 0; i < m; i++) in >> ids[i];
    return ids;
}

static void print_ids(const std::vector<int32_t>& ids) {
    printf("%zu ", ids.size());
    for (size_t i = 0; i < ids.size(); i++) printf("%s%d", i ? " " : "", ids[i]);
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const std::string d = argv[1];
    try {
        ORB_SLAM2::ORBVocabulary voc;
        if (!voc.loadFromTextFile(d + "/voc.txt")) throw std::runtime_error(std::string("vocabulary: ") + oslam_last_error());
        ORB_SLAM2::KeyFrameDatabase db(voc, atoi(argv[2]), atoi(argv[3]));
        ORB_SLAM2::LoopClosing lc(&db);
        std::ifstream f(d + "/ops.txt");
        std::string line;
        while (std::getline(f, line)) {
            std::istringstream in(line);
            char op = 0;
            in >> op;
            ORB_SLAM2::KeyFrameDatabaseKeyFrameView KF;
            in >> KF.mnId;
            if (op == 'M') { lc.mLastLoopKFid = (long unsigned int)KF.mnId; continue; }
            if (op == 'S') { lc.SetConnectedKeyFrames(KF.mnId, read_ids(in)); continue; }
            if (op == 'V') { KF.vpBestCovisibles = read_ids(in); db.UpdateCovisibility(KF); continue; }
            if (op != 'D') throw std::runtime_error("ops.txt: unknown operation");
            DBoW2::BowVector bow;
            int n = 0;
            in >> n;
            for (int i = 0; i < n; i++) {
                unsigned w; double x;
                in >> w >> x;
                bow[w] = x;
            }
            KF.mBowVec = &bow;
            KF.spConnected = read_ids(in);
            KF.vpBestCovisibles = read_ids(in);
            const bool gated = (long)KF.mnId < (long)lc.mLastLoopKFid + 10;
            const bool loop = lc.DetectLoop(KF);
            if (gated) { printf("D %d %d gated\n", KF.mnId, loop ? 1 : 0); continue; }
            printf("D %d %d ", KF.mnId, loop ? 1 : 0);
            print_ids(lc.mvpEnoughConsistentCandidates);
            printf(" | ");
            print_ids(lc.mvpCandidateKFs);
            printf(" | %.9g | %d\n", lc.minScore(), lc.consistentGroups());
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
