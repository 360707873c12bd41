// A caller of ORB_SLAM2::PnPsolver written only against include/orb_slam2_adapter.hpp: the solver of one (lost frame, candidate keyframe) pair as
// Tracking::Relocalization makes it (src/Tracking.cc:1650-1651, :1675-1676).  Reads <dir>/{keys,has,bad,Xw,sigma2}.bin and meta.txt, writes
// <dir>/out_{Tcw,inliers}.bin and out_results.txt.  tests/test_pnp_gpu.py builds it, runs it and compares with the ctypes path.
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

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string d = argv[1];
    try {
        std::map<std::string, double> meta;
        { std::ifstream f(d + "/meta.txt"); std::string k; double v; while (f >> k >> v) meta[k] = v; }
        const auto keys = load<oslam::KeyPoint>(d + "/keys.bin");
        const auto has = load<uint8_t>(d + "/has.bin");
        const auto bad = load<uint8_t>(d + "/bad.bin");
        const auto Xw = load<float>(d + "/Xw.bin");
        const auto sigma2 = load<float>(d + "/sigma2.bin");
        ORB_SLAM2::PnPFrameView F;
        F.N = (int)keys.size(); F.mvKeysUn = keys.data(); F.mvLevelSigma2 = sigma2.data(); F.nLevels = (int)sigma2.size();
        F.fx = (float)meta["fx"]; F.fy = (float)meta["fy"]; F.cx = (float)meta["cx"]; F.cy = (float)meta["cy"];
        ORB_SLAM2::PnPMatchView M;
        M.has_mp = has.data(); M.bad = bad.data(); M.Xw = Xw.data();
        ORB_SLAM2::PnPsolver* pSolver = new ORB_SLAM2::PnPsolver(F, M, (uint32_t)meta["seed"]);
        pSolver->SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
        std::vector<bool> vbInliers;
        int nInliers = 0;
        bool bNoMore = false;
        float Tcw[16] = {0};
        const bool found = pSolver->iterate(5, bNoMore, vbInliers, nInliers, Tcw);
        // a second call has nothing left to do
        std::vector<bool> vb2;
        int n2 = 0;
        bool noMore2 = false;
        float T2[16];
        const bool found2 = pSolver->iterate(5, noMore2, vb2, n2, T2);
        std::vector<uint8_t> flags(vbInliers.size());
        for (size_t i = 0; i < vbInliers.size(); i++) flags[i] = vbInliers[i] ? 1 : 0;
        std::ofstream(d + "/out_Tcw.bin", std::ios::binary).write(reinterpret_cast<const char*>(Tcw), sizeof(Tcw));
        std::ofstream(d + "/out_inliers.bin", std::ios::binary).write(reinterpret_cast<const char*>(flags.data()), (std::streamsize)flags.size());
        std::ofstream r(d + "/out_results.txt");
        r << "found " << (found ? 1 : 0) << "\nbNoMore " << (bNoMore ? 1 : 0) << "\nnInliers " << nInliers << "\nN " << pSolver->mvSigma2.size() << "\niterations "
          << pSolver->mnIterations << "\nminInliers " << pSolver->Adjusted().min_inliers << "\nfound2 " << (found2 ? 1 : 0) << "\nnoMore2 " << (noMore2 ? 1 : 0) << "\n";
        delete pSolver;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
