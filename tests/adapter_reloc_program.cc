// A caller of ORB_SLAM2::ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) written only against include/orb_slam2_adapter.hpp: the body of
// Tracking::Relocalization for one frame and one candidate keyframe once PnP has a pose (src/Tracking.cc:1705-1752): PoseOptimization, drop the outliers, with fewer
// than 50 inliers the coarse search (10, 100), with enough matches PoseOptimization again, with 31 to 49 inliers sFound rebuilt and the fine search (3, 64), with
// enough matches the final PoseOptimization, and the nGood >= 50 decision.
// Reads <dir>/keys.bin, desc.bin (the frame), tcw.bin (the PnP pose), mp.bin (int32 per keypoint: mvpMapPoints after :1694-1703 as a slot of the keyframe, -1 = NULL),
// the keyframe's slots Xw.bin, pdesc.bin, maxD.bin, minD.bin, angle.bin, bad.bin (pMP == NULL || pMP->isBad()), scale.bin and meta.txt.
// Prints "nGood <n>" after every PoseOptimization; per search "search <th> <ORBdist>", "Tcw <16 hex floats>" (the pose it passed in), "before <mvpMapPoints>",
// "has_mp <bytes>", "skip <bytes>", "nadditional <n>", "after <mvpMapPoints>"; at the end "final <mvpMapPoints>" and "decision <0|1>".
// tests/test_reloc_project_gpu.py builds it, runs it and replays every search.
#include <cstdio>
#include <fstream>
#include <map>
#include <set>
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

static void print_ints(const char* tag, const std::vector<int32_t>& v) {
    printf("%s", tag);
    for (int32_t x : v) printf(" %d", x);
    printf("\n");
}

static void print_bytes(const char* tag, const std::vector<uint8_t>& v) {
    printf("%s ", tag);
    for (uint8_t x : v) putchar(x ? '1' : '0');
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string d = argv[1];
    try {
        std::map<std::string, double> meta;
        { std::ifstream f(d + "/meta.txt"); std::string k; double v; while (f >> k >> v) meta[k] = v; }
        const auto scale = load<float>(d + "/scale.bin");
        const auto keys = load<oslam::KeyPoint>(d + "/keys.bin");
        const auto desc = load<uint8_t>(d + "/desc.bin");
        const auto Xw = load<float>(d + "/Xw.bin"), maxD = load<float>(d + "/maxD.bin"), minD = load<float>(d + "/minD.bin"), angle = load<float>(d + "/angle.bin");
        const auto pdesc = load<uint8_t>(d + "/pdesc.bin"), bad = load<uint8_t>(d + "/bad.bin");
        std::vector<float> mTcw = load<float>(d + "/tcw.bin");                 // Tcw.copyTo(mCurrentFrame.mTcw), :1688
        std::vector<int32_t> mvpMapPoints = load<int32_t>(d + "/mp.bin");      // :1694-1703
        const int N = (int)keys.size(), nSlots = (int)maxD.size();
        if ((int)mvpMapPoints.size() != N || mTcw.size() != 16) throw std::runtime_error("mp.bin / tcw.bin do not fit the frame");
        std::set<int32_t> sFound;
        for (int j = 0; j < N; j++)
            if (mvpMapPoints[j] != -1) sFound.insert(mvpMapPoints[j]);

        std::vector<float> invLevelSigma2(scale.size()), uRight((size_t)N + 1, -1.f);
        for (size_t l = 0; l < scale.size(); l++) invLevelSigma2[l] = 1.0f / (scale[l] * scale[l]);
        std::vector<uint8_t> mvbOutlier((size_t)N + 1), has_mp((size_t)N + 1);
        std::vector<float> kpXw((size_t)N * 3 + 3);
        auto PoseOptimization = [&]() {   // Optimizer::PoseOptimization(&mCurrentFrame)
            for (int k = 0; k < N; k++) {
                has_mp[k] = mvpMapPoints[k] != -1;
                if (has_mp[k]) memcpy(&kpXw[(size_t)k * 3], &Xw[(size_t)mvpMapPoints[k] * 3], 12);
            }
            ORB_SLAM2::PoseFrameView F = {N, mTcw.data(), kpXw.data(), has_mp.data(), keys.data(), uRight.data(), invLevelSigma2.data(), mvbOutlier.data(),
                                          (float)meta["fx"], (float)meta["fy"], (float)meta["cx"], (float)meta["cy"], 0.f};
            const int n = ORB_SLAM2::Optimizer::PoseOptimization(F);
            printf("nGood %d\n", n);
            return n;
        };
        auto drop_outliers = [&]() {
            for (int io = 0; io < N; io++)
                if (mvpMapPoints[io] != -1 && mvbOutlier[io]) mvpMapPoints[io] = -1;
        };
        ORB_SLAM2::ORBmatcher matcher2(0.9f, true);   // :1661
        auto SearchByProjection = [&](float th, int ORBdist) {   // matcher2.SearchByProjection(mCurrentFrame, vpCandidateKFs[i], sFound, th, ORBdist)
            std::vector<uint8_t> skip((size_t)nSlots), had((size_t)N);
            for (int i = 0; i < nSlots; i++) skip[i] = bad[i] || sFound.count(i);
            for (int k = 0; k < N; k++) had[k] = mvpMapPoints[k] != -1;
            ORB_SLAM2::RelocFrameView F;
            F.N = N; F.mvKeysUn = keys.data(); F.mDescriptors = desc.data();
            memcpy(F.Tcw, mTcw.data(), sizeof(F.Tcw));
            F.fx = (float)meta["fx"]; F.fy = (float)meta["fy"]; F.cx = (float)meta["cx"]; F.cy = (float)meta["cy"];
            F.mnMinX = (float)meta["minX"]; F.mnMinY = (float)meta["minY"]; F.mnMaxX = (float)meta["maxX"]; F.mnMaxY = (float)meta["maxY"];
            F.mvScaleFactors = scale.data(); F.mnScaleLevels = (int)scale.size(); F.mfLogScaleFactor = (float)meta["logScaleFactor"];
            const ORB_SLAM2::RelocKeyFrameView KF = {nSlots, Xw.data(), pdesc.data(), maxD.data(), minD.data(), angle.data(), skip.data()};
            printf("search %g %d\nTcw", th, ORBdist);
            for (int i = 0; i < 16; i++) printf(" %a", F.Tcw[i]);
            printf("\n");
            print_ints("before", mvpMapPoints);
            print_bytes("has_mp", had);
            print_bytes("skip", skip);
            const int n = matcher2.SearchByProjection(F, KF, mvpMapPoints, th, ORBdist);
            printf("nadditional %d\n", n);
            print_ints("after", mvpMapPoints);
            return n;
        };

        int nGood = PoseOptimization();   // :1705
        if (nGood >= 10) {                // :1707
            drop_outliers();              // :1710-1712
            if (nGood < 50) {             // :1715
                int nadditional = SearchByProjection(10, 100);   // :1717
                if (nadditional + nGood >= 50) {                 // :1719
                    nGood = PoseOptimization();                  // :1721
                    if (nGood > 30 && nGood < 50) {              // :1725
                        sFound.clear();                          // :1727-1730
                        for (int ip = 0; ip < N; ip++)
                            if (mvpMapPoints[ip] != -1) sFound.insert(mvpMapPoints[ip]);
                        nadditional = SearchByProjection(3, 64); // :1731
                        if (nGood + nadditional >= 50) {         // :1734
                            nGood = PoseOptimization();          // :1736
                            drop_outliers();                     // :1738-1740
                        }
                    }
                }
            }
        }
        print_ints("final", mvpMapPoints);
        printf("decision %d\n", nGood >= 50 ? 1 : 0);   // :1748 (nGood < 10 continues with the next candidate: no match either)
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
