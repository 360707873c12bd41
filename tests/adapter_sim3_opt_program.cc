// A caller of ORB_SLAM2::ORBmatcher::SearchBySim3 and ORB_SLAM2::Optimizer::OptimizeSim3 written only against include/orb_slam2_adapter.hpp: the body of
// LoopClosing::ComputeSim3's loop after a solver returned a Sim3 (src/LoopClosing.cc:318-330): SearchBySim3 with th = 7.5 on vpMapPointMatches, gScm from the
// solver's float R, t, s, OptimizeSim3 with th2 = 10 and mbFixScale, and the `nInliers >= 20` decision.  Reads the files of adapter_sim3_match_program.cc and
// invsigma.bin (mvInvLevelSigma2); meta.txt also holds fixScale.  Prints "nFound <n>", "nInliers <n>", "bMatch <0|1>", one line "<i1> <entry of
// vpMapPointMatches after both calls>" per keypoint of KF1 and "S12" followed by R (row-major), t, s with 17 digits.  tests/test_sim3_opt_gpu.py builds
// it, runs it and compares the lines.
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

struct KeyFrameData {
    std::vector<oslam::KeyPoint> keys;
    std::vector<uint8_t> desc, has_mp, mp_desc;
    std::vector<float> Xw, maxD, minD, pose;
};

static KeyFrameData load_kf(const std::string& d, const char* tag) {
    KeyFrameData k;
    k.keys = load<oslam::KeyPoint>(d + "/keys" + tag + ".bin"); k.desc = load<uint8_t>(d + "/desc" + tag + ".bin"); k.has_mp = load<uint8_t>(d + "/has_mp" + tag + ".bin");
    k.mp_desc = load<uint8_t>(d + "/mp_desc" + tag + ".bin"); k.Xw = load<float>(d + "/Xw" + tag + ".bin"); k.maxD = load<float>(d + "/maxD" + tag + ".bin");
    k.minD = load<float>(d + "/minD" + tag + ".bin"); k.pose = load<float>(d + "/pose" + tag + ".bin");
    return k;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string d = argv[1];
    try {
        std::map<std::string, double> meta;
        { std::ifstream f(d + "/meta.txt"); std::string k; double v; while (f >> k >> v) meta[k] = v; }
        const KeyFrameData k1 = load_kf(d, "1"), k2 = load_kf(d, "2");
        const auto scale = load<float>(d + "/scale.bin"), sim3 = load<float>(d + "/sim3.bin"), invsigma = load<float>(d + "/invsigma.bin");
        std::vector<int32_t> vpMapPointMatches = load<int32_t>(d + "/matched.bin");
        const KeyFrameData* data[2] = {&k1, &k2};
        ORB_SLAM2::Sim3MatchKeyFrameView KF[2];
        ORB_SLAM2::Sim3OptKeyFrameView OF[2];
        for (int i = 0; i < 2; i++) {
            const KeyFrameData& k = *data[i];
            KF[i].N = (int)k.keys.size(); KF[i].mvKeysUn = k.keys.data(); KF[i].mDescriptors = k.desc.data(); KF[i].has_mp = k.has_mp.data(); KF[i].Xw = k.Xw.data();
            KF[i].mpDescriptors = k.mp_desc.data(); KF[i].mfMaxDistance = k.maxD.data(); KF[i].mfMinDistance = k.minD.data();
            for (int j = 0; j < 16; j++) KF[i].Tcw[j] = OF[i].Tcw[j] = k.pose[j];
            KF[i].fx = OF[i].fx = (float)meta["fx"]; KF[i].fy = OF[i].fy = (float)meta["fy"]; KF[i].cx = OF[i].cx = (float)meta["cx"]; KF[i].cy = OF[i].cy = (float)meta["cy"];
            KF[i].mnMinX = (float)meta["minX"]; KF[i].mnMinY = (float)meta["minY"]; KF[i].mnMaxX = (float)meta["maxX"]; KF[i].mnMaxY = (float)meta["maxY"];
            KF[i].mvScaleFactors = scale.data(); KF[i].mnScaleLevels = (int)scale.size(); KF[i].mfLogScaleFactor = (float)meta["logScaleFactor"];
            OF[i].N = KF[i].N; OF[i].mvKeysUn = k.keys.data(); OF[i].has_mp = k.has_mp.data(); OF[i].Xw = k.Xw.data(); OF[i].mvInvLevelSigma2 = invsigma.data();
        }
        const bool mbFixScale = meta["fixScale"] != 0;
        ORB_SLAM2::ORBmatcher matcher(0.75f, true);   // src/LoopClosing.cc:238
        const int nFound = matcher.SearchBySim3(KF[0], KF[1], vpMapPointMatches, sim3[0], sim3.data() + 1, sim3.data() + 10, 7.5f);   // :324
        ORB_SLAM2::Sim3 gScm;                                                                                                          // :326
        for (int k = 0; k < 9; k++) gScm.R[k] = sim3[1 + k];
        for (int k = 0; k < 3; k++) gScm.t[k] = sim3[10 + k];
        gScm.s = sim3[0];
        const int nInliers = ORB_SLAM2::Optimizer::OptimizeSim3(OF[0], OF[1], vpMapPointMatches, gScm, 10, mbFixScale);              // :327
        const bool bMatch = nInliers >= 20;                                                                                            // :330
        printf("nFound %d\nnInliers %d\nbMatch %d\n", nFound, nInliers, bMatch ? 1 : 0);
        for (size_t i1 = 0; i1 < vpMapPointMatches.size(); i1++) printf("%zu %d\n", i1, vpMapPointMatches[i1]);
        printf("S12");
        for (int k = 0; k < 9; k++) printf(" %.17g", gScm.R[k]);
        for (int k = 0; k < 3; k++) printf(" %.17g", gScm.t[k]);
        printf(" %.17g\n", gScm.s);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
