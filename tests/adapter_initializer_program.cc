// A caller of ORB_SLAM2::Initializer written only against include/orb_slam2_adapter.hpp: Tracking::MonocularInitialization after the match
// (src/Tracking.cc:691-714) — Initialize, the loop that clears mvIniMatches[i] where the match was not triangulated, the pose Tcw = [R | t].
// Reads <dir>/{keys1,keys2,matches}.bin and meta.txt, writes <dir>/out_{Tcw,P3D,matches}.bin and out_results.txt.  tests/test_initializer_gpu.py builds
// it, runs it and compares with the ctypes path.
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
        const auto keys1 = load<oslam::KeyPoint>(d + "/keys1.bin");
        const auto keys2 = load<oslam::KeyPoint>(d + "/keys2.bin");
        const auto matches = load<int32_t>(d + "/matches.bin");
        ORB_SLAM2::InitFrameView mInitialFrame, mCurrentFrame;
        mInitialFrame.N = (int)keys1.size(); mInitialFrame.mvKeysUn = keys1.data();
        mCurrentFrame.N = (int)keys2.size(); mCurrentFrame.mvKeysUn = keys2.data();
        mInitialFrame.fx = mCurrentFrame.fx = (float)meta["fx"]; mInitialFrame.fy = mCurrentFrame.fy = (float)meta["fy"];
        mInitialFrame.cx = mCurrentFrame.cx = (float)meta["cx"]; mInitialFrame.cy = mCurrentFrame.cy = (float)meta["cy"];
        ORB_SLAM2::Initializer* mpInitializer = new ORB_SLAM2::Initializer(mInitialFrame, 1.0, (int)meta["iterations"], (uint32_t)meta["seed"]);   // :661
        std::vector<int> mvIniMatches(matches.begin(), matches.end());
        int nmatches = 0;
        for (int m : mvIniMatches) nmatches += m >= 0 ? 1 : 0;
        float Rcw[9] = {0}, tcw[3] = {0};   // Current Camera Rotation, Current Camera Translation
        std::vector<bool> vbTriangulated;   // Triangulated Correspondences (mvIniMatches)
        std::vector<ORB_SLAM2::Point3f> mvIniP3D;
        float Tcw[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        const bool ok = mpInitializer->Initialize(mCurrentFrame, mvIniMatches, Rcw, tcw, mvIniP3D, vbTriangulated);
        if (ok) {
            for (size_t i = 0, iend = mvIniMatches.size(); i < iend; i++) {   // :697-704
                if (mvIniMatches[i] >= 0 && !vbTriangulated[i]) {
                    mvIniMatches[i] = -1;
                    nmatches--;
                }
            }
            for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) Tcw[4 * r + c] = Rcw[3 * r + c]; Tcw[4 * r + 3] = tcw[r]; }   // :707-711
        }
        std::vector<int32_t> out_matches(mvIniMatches.begin(), mvIniMatches.end());
        std::ofstream(d + "/out_Tcw.bin", std::ios::binary).write(reinterpret_cast<const char*>(Tcw), sizeof(Tcw));
        std::ofstream(d + "/out_P3D.bin", std::ios::binary).write(reinterpret_cast<const char*>(mvIniP3D.data()), (std::streamsize)(mvIniP3D.size() * sizeof(ORB_SLAM2::Point3f)));
        std::ofstream(d + "/out_matches.bin", std::ios::binary).write(reinterpret_cast<const char*>(out_matches.data()), (std::streamsize)(out_matches.size() * sizeof(int32_t)));
        std::ofstream r(d + "/out_results.txt");
        r << "ok " << (ok ? 1 : 0) << "\nnmatches " << nmatches << "\nmodel " << mpInitializer->status[1] << "\nN " << mpInitializer->status[2] << "\nnGood " << mpInitializer->status[3]
          << "\nmotion " << mpInitializer->status[4] << "\n";
        delete mpInitializer;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
