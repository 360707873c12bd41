// A caller written only against include/orb_slam2_adapter.hpp: the body of Tracking::MonocularInitialization (src/Tracking.cc:644-716) over a short list of
// frames — the reference frame and mvbPrevMatched, ORBmatcher(0.9, true).SearchForInitialization(mInitialFrame, mCurrentFrame, mvbPrevMatched, mvIniMatches,
// 100), the reset below 100 matches, Initializer::Initialize, the loop that clears the matches that were not triangulated, Tcw = [R | t].
// Reads <dir>/meta.txt and <dir>/{keys,desc}_<j>.bin, prints per frame the decision and, for every search, its inputs (the carried points as hex floats) and
// outputs.  tests/test_search_init_gpu.py builds it, runs it and replays every printed search with the restatement.
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

struct Frame {   // what the caller keeps of a Frame
    std::vector<oslam::KeyPoint> mvKeysUn;
    std::vector<uint8_t> mDescriptors;
};

static void print_points(const char* tag, const std::vector<ORB_SLAM2::Point2f>& v) {
    printf("%s", tag);
    for (const ORB_SLAM2::Point2f& p : v) printf(" %a %a", p.x, p.y);
    printf("\n");
}

static void print_ints(const char* tag, const std::vector<int>& v) {
    printf("%s", tag);
    for (int m : v) printf(" %d", m);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string d = argv[1];
    try {
        std::map<std::string, double> meta;
        { std::ifstream f(d + "/meta.txt"); std::string k; double v; while (f >> k >> v) meta[k] = v; }
        const int n_frames = (int)meta["n_frames"];
        std::vector<Frame> frames(n_frames);
        for (int j = 0; j < n_frames; j++) {
            frames[j].mvKeysUn = load<oslam::KeyPoint>(d + "/keys_" + std::to_string(j) + ".bin");
            frames[j].mDescriptors = load<uint8_t>(d + "/desc_" + std::to_string(j) + ".bin");
        }
        const auto match_view = [&](const Frame& F) {
            return ORB_SLAM2::InitMatchFrameView{(int)F.mvKeysUn.size(), F.mvKeysUn.data(), F.mDescriptors.data(), (float)meta["minX"], (float)meta["minY"], (float)meta["maxX"],
                                                 (float)meta["maxY"]};
        };
        const auto init_view = [&](const Frame& F) {
            return ORB_SLAM2::InitFrameView{(int)F.mvKeysUn.size(), F.mvKeysUn.data(), (float)meta["fx"], (float)meta["fy"], (float)meta["cx"], (float)meta["cy"]};
        };

        ORB_SLAM2::Initializer* mpInitializer = nullptr;
        int mInitialFrame = -1;
        std::vector<ORB_SLAM2::Point2f> mvbPrevMatched;
        std::vector<int> mvIniMatches;
        std::vector<ORB_SLAM2::Point3f> mvIniP3D;
        for (int j = 0; j < n_frames; j++) {
            const Frame& mCurrentFrame = frames[j];
            printf("frame %d %zu\n", j, mCurrentFrame.mvKeysUn.size());
            if (!mpInitializer) {
                if (mCurrentFrame.mvKeysUn.size() > 100) {   // Set Reference Frame (:650-666)
                    mInitialFrame = j;
                    mvbPrevMatched.resize(mCurrentFrame.mvKeysUn.size());
                    for (size_t i = 0; i < mCurrentFrame.mvKeysUn.size(); i++) {
#ifdef OSLAM_ADAPTER_USE_OPENCV
                        mvbPrevMatched[i] = mCurrentFrame.mvKeysUn[i].pt;
#else
                        mvbPrevMatched[i].x = mCurrentFrame.mvKeysUn[i].x; mvbPrevMatched[i].y = mCurrentFrame.mvKeysUn[i].y;
#endif
                    }
                    mpInitializer = new ORB_SLAM2::Initializer(init_view(mCurrentFrame), 1.0, (int)meta["iterations"], (uint32_t)meta["seed"]);
                    std::fill(mvIniMatches.begin(), mvIniMatches.end(), -1);
                    printf("decision reference\n");
                } else {
                    printf("decision idle\n");
                }
                continue;
            }
            if ((int)mCurrentFrame.mvKeysUn.size() <= 100) {   // :671-677
                delete mpInitializer;
                mpInitializer = nullptr;
                std::fill(mvIniMatches.begin(), mvIniMatches.end(), -1);
                printf("decision few_keys\n");
                continue;
            }
            // Find correspondences (:680-681)
            ORB_SLAM2::ORBmatcher matcher(0.9f, true);
            printf("search %d %d\n", mInitialFrame, j);
            print_points("prev", mvbPrevMatched);
            int nmatches = matcher.SearchForInitialization(match_view(frames[mInitialFrame]), match_view(mCurrentFrame), mvbPrevMatched, mvIniMatches, 100);
            printf("nmatches %d\n", nmatches);
            print_ints("matches", mvIniMatches);
            print_points("prev_after", mvbPrevMatched);
            if (nmatches < 100) {   // Check if there are enough correspondences (:684-689)
                delete mpInitializer;
                mpInitializer = nullptr;
                printf("decision few_matches\n");
                continue;
            }
            float Rcw[9] = {0}, tcw[3] = {0};   // Current Camera Rotation, Current Camera Translation
            std::vector<bool> vbTriangulated;   // Triangulated Correspondences (mvIniMatches)
            if (mpInitializer->Initialize(init_view(mCurrentFrame), mvIniMatches, Rcw, tcw, mvIniP3D, vbTriangulated)) {
                for (size_t i = 0, iend = mvIniMatches.size(); i < iend; i++) {   // :697-704
                    if (mvIniMatches[i] >= 0 && !vbTriangulated[i]) {
                        mvIniMatches[i] = -1;
                        nmatches--;
                    }
                }
                float Tcw[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // Set Frame Poses (:707-711)
                for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) Tcw[4 * r + c] = Rcw[3 * r + c]; Tcw[4 * r + 3] = tcw[r]; }
                printf("triangulated %d\n", nmatches);
                print_ints("ini_matches", mvIniMatches);
                printf("Tcw");
                for (float v : Tcw) printf(" %a", v);
                printf("\ndecision initialized\n");
                break;   // (CreateInitialMapMonocular follows, :713)
            }
            printf("decision failed\n");
        }
        delete mpInitializer;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
