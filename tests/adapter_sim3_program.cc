// A caller of ORB_SLAM2::Sim3Solver written only against include/orb_slam2_adapter.hpp: the solver of one loop candidate as LoopClosing::ComputeSim3
// makes and drives it (src/LoopClosing.cc:275-277, :299-309): iterate(5) until a Sim3 or bNoMore, then — as after a failed OptimizeSim3 — iterate(5)
// again until the next Sim3 or bNoMore.  Reads <dir>/{keys1,keys2,matched,bad1,bad2,index1,index2,Xw1,Xw2,sigma2,pose1,pose2}.bin and meta.txt, writes
// <dir>/out_{T12,inliers}_{a,b}.bin, out_best.bin and out_results.txt.  tests/test_sim3_gpu.py builds it, runs it and compares with the ctypes path.
#include <cstdio>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "orb_slam2_adapter.hpp"

template <class T>
static std::vector<T> load(const std::string& path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("cannot open " + path);
    const size_t bytes = (size_t)f.tellg();
    std::vector<T> v(bytes / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}

struct Round { bool found = false, bNoMore = false; int nInliers = 0, calls = 0, iterations = 0; float T12[16] = {0}; std::vector<bool> vbInliers; };

static Round until_sim3_or_no_more(ORB_SLAM2::Sim3Solver* pSolver) {
    Round r;
    while (!r.found && !r.bNoMore) {
        r.found = pSolver->iterate(5, r.bNoMore, r.vbInliers, r.nInliers, r.T12);
        r.calls++;
    }
    r.iterations = pSolver->mnIterations();
    return r;
}

static void write_round(const std::string& d, const char* tag, const Round& r) {
    std::vector<uint8_t> flags(r.vbInliers.size());
    for (size_t i = 0; i < flags.size(); i++) flags[i] = r.vbInliers[i] ? 1 : 0;
    std::ofstream(d + "/out_T12_" + tag + ".bin", std::ios::binary).write(reinterpret_cast<const char*>(r.T12), sizeof(r.T12));
    std::ofstream(d + "/out_inliers_" + tag + ".bin", std::ios::binary).write(reinterpret_cast<const char*>(flags.data()), (std::streamsize)flags.size());
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string d = argv[1];
    try {
        std::map<std::string, double> meta;
        { std::ifstream f(d + "/meta.txt"); std::string k; double v; while (f >> k >> v) meta[k] = v; }
        const auto keys1 = load<oslam::KeyPoint>(d + "/keys1.bin"), keys2 = load<oslam::KeyPoint>(d + "/keys2.bin");
        const auto matched = load<uint8_t>(d + "/matched.bin"), bad1 = load<uint8_t>(d + "/bad1.bin"), bad2 = load<uint8_t>(d + "/bad2.bin");
        const auto index1 = load<int32_t>(d + "/index1.bin"), index2 = load<int32_t>(d + "/index2.bin");
        const auto Xw1 = load<float>(d + "/Xw1.bin"), Xw2 = load<float>(d + "/Xw2.bin");
        const auto sigma2 = load<float>(d + "/sigma2.bin"), pose1 = load<float>(d + "/pose1.bin"), pose2 = load<float>(d + "/pose2.bin");   // pose: Rcw (9), tcw (3)
        ORB_SLAM2::Sim3KeyFrameView KF1, KF2;
        KF1.N = (int)keys1.size(); KF1.mvKeysUn = keys1.data(); KF1.mvLevelSigma2 = sigma2.data(); KF1.nLevels = (int)sigma2.size();
        KF2.N = (int)keys2.size(); KF2.mvKeysUn = keys2.data(); KF2.mvLevelSigma2 = sigma2.data(); KF2.nLevels = (int)sigma2.size();
        KF1.fx = KF2.fx = (float)meta["fx"]; KF1.fy = KF2.fy = (float)meta["fy"]; KF1.cx = KF2.cx = (float)meta["cx"]; KF1.cy = KF2.cy = (float)meta["cy"];
        for (int i = 0; i < 9; i++) { KF1.Rcw[i] = pose1[i]; KF2.Rcw[i] = pose2[i]; }
        for (int i = 0; i < 3; i++) { KF1.tcw[i] = pose1[9 + i]; KF2.tcw[i] = pose2[9 + i]; }
        ORB_SLAM2::Sim3MatchView M;
        M.N1 = (int)matched.size(); M.matched = matched.data(); M.has_mp1 = nullptr; M.bad1 = bad1.data(); M.bad2 = bad2.data();
        M.indexKF1 = index1.data(); M.indexKF2 = index2.data(); M.Xw1 = Xw1.data(); M.Xw2 = Xw2.data();
        ORB_SLAM2::Sim3Solver* pSolver = new ORB_SLAM2::Sim3Solver(KF1, KF2, M, meta["fix_scale"] != 0, (uint32_t)meta["seed"]);
        pSolver->SetRansacParameters(0.99, 20, 300);
        const Round a = until_sim3_or_no_more(pSolver);
        const Round b = until_sim3_or_no_more(pSolver);
        write_round(d, "a", a);
        write_round(d, "b", b);
        float best[13];
        pSolver->GetEstimatedRotation(best); pSolver->GetEstimatedTranslation(best + 9); best[12] = pSolver->GetEstimatedScale();
        std::ofstream(d + "/out_best.bin", std::ios::binary).write(reinterpret_cast<const char*>(best), sizeof(best));
        std::ofstream r(d + "/out_results.txt");
        r << "N " << pSolver->mvSigma2_1.size() << "\nmN1 " << pSolver->mN1 << "\nmaxIts " << pSolver->Adjusted().iterations;
        const Round* rounds[2] = {&a, &b};
        for (int k = 0; k < 2; k++) {
            const char t = k ? 'b' : 'a';
            r << "\nfound_" << t << " " << (rounds[k]->found ? 1 : 0) << "\nbNoMore_" << t << " " << (rounds[k]->bNoMore ? 1 : 0) << "\nnInliers_" << t << " " << rounds[k]->nInliers
              << "\ncalls_" << t << " " << rounds[k]->calls << "\niterations_" << t << " " << rounds[k]->iterations;
        }
        r << "\nbestInliers " << pSolver->mnBestInliers() << "\n";
        delete pSolver;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
