// A caller of ORB_SLAM2::ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) and ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) written only
// against include/orb_slam2_adapter.hpp: the end of LoopClosing::ComputeSim3 (src/LoopClosing.cc:376-386: the search over mvpLoopMapPoints with th = 10, then
// nTotalMatches >= 40 decides) and one keyframe's step of LoopClosing::SearchAndFuse (:600, th = 4).  Reads <dir>/{keys,desc}{1,2}.bin (keyframe 1: the current
// keyframe of the search; keyframe 2: a corrected keyframe of the Fuse), state2.bin, matched.bin (vpMatched on entry), scw{1,2}.bin, the points' Xw.bin, normal.bin,
// pdesc.bin, maxD.bin, minD.bin, skip{1,2}.bin, scale.bin and meta.txt.  Prints "nmatches <n>", "nTotalMatches <n>", "accept <0|1>", one line "m <idx> <entry of
// vpMatched after the call>" per keypoint, "nFused <n>" and one line "r <i> <vpReplacePoint[i]> <keypoint of the added observation or -1>" per point.
// tests/test_sim3_project_gpu.py builds it, runs it and compares the lines.
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
        const auto scale = load<float>(d + "/scale.bin");
        const auto keys1 = load<oslam::KeyPoint>(d + "/keys1.bin"), keys2 = load<oslam::KeyPoint>(d + "/keys2.bin");
        const auto desc1 = load<uint8_t>(d + "/desc1.bin"), desc2 = load<uint8_t>(d + "/desc2.bin"), state2 = load<uint8_t>(d + "/state2.bin");
        const auto scw1 = load<float>(d + "/scw1.bin"), scw2 = load<float>(d + "/scw2.bin");
        const auto Xw = load<float>(d + "/Xw.bin"), normal = load<float>(d + "/normal.bin"), maxD = load<float>(d + "/maxD.bin"), minD = load<float>(d + "/minD.bin");
        const auto pdesc = load<uint8_t>(d + "/pdesc.bin"), skip1 = load<uint8_t>(d + "/skip1.bin"), skip2 = load<uint8_t>(d + "/skip2.bin");
        std::vector<int32_t> vpMatched = load<int32_t>(d + "/matched.bin");   // mvpCurrentMatchedPoints as OptimizeSim3's candidate left it: -1 = NULL

        ORB_SLAM2::Sim3ProjKeyFrameView KF[2];
        KF[0].N = (int)keys1.size(); KF[0].mvKeysUn = keys1.data(); KF[0].mDescriptors = desc1.data(); KF[0].mapPointState = nullptr;
        KF[1].N = (int)keys2.size(); KF[1].mvKeysUn = keys2.data(); KF[1].mDescriptors = desc2.data(); KF[1].mapPointState = state2.data();
        for (int i = 0; i < 2; i++) {
            KF[i].fx = (float)meta["fx"]; KF[i].fy = (float)meta["fy"]; KF[i].cx = (float)meta["cx"]; KF[i].cy = (float)meta["cy"];
            KF[i].mnMinX = (float)meta["minX"]; KF[i].mnMinY = (float)meta["minY"]; KF[i].mnMaxX = (float)meta["maxX"]; KF[i].mnMaxY = (float)meta["maxY"];
            KF[i].mvScaleFactors = scale.data(); KF[i].mnScaleLevels = (int)scale.size(); KF[i].mfLogScaleFactor = (float)meta["logScaleFactor"];
        }
        ORB_SLAM2::Sim3ProjPointsView points = {(int)maxD.size(), Xw.data(), normal.data(), pdesc.data(), maxD.data(), minD.data(), skip1.data()};

        ORB_SLAM2::ORBmatcher matcher(0.75f, true);   // src/LoopClosing.cc:238
        const int nmatches = matcher.SearchByProjection(KF[0], scw1.data(), points, vpMatched, 10);   // :376
        int nTotalMatches = 0;   // :379-384
        for (size_t i = 0; i < vpMatched.size(); i++)
            if (vpMatched[i] != -1) nTotalMatches++;
        printf("nmatches %d\nnTotalMatches %d\naccept %d\n", nmatches, nTotalMatches, nTotalMatches >= 40 ? 1 : 0);   // :386
        for (size_t i = 0; i < vpMatched.size(); i++) printf("m %zu %d\n", i, vpMatched[i]);

        points.skip = skip2.data();
        std::vector<int32_t> vpReplacePoint((size_t)points.n, -1), addedKp;   // :599
        const int nFused = matcher.Fuse(KF[1], scw2.data(), points, 4.f, vpReplacePoint, &addedKp);   // :600
        printf("nFused %d\n", nFused);
        for (int i = 0; i < points.n; i++) printf("r %d %d %d\n", i, vpReplacePoint[i], addedKp[i]);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
