// The body of Tracking::TrackObject (reference src/Tracking.cc:1058-1076) over a short list of frames, written only against include/orb_slam2_adapter.hpp:
// per frame the HSV histograms of its detections (Frame::ExtractHSVHistogramsFromMask), ObjectMatcher::MatchTwoFrame against the previous frame and
// ObjectMatcher::MatchMapToFrame against a map this program keeps with the bookkeeping of the Object3D constructor and Object3D::Update
// (src/ObjectTypes.cc:44-45, :131-132): an unmatched detection makes a new object with one observation, a matched one appends an observation.
// usage: adapter_object_program DIR   (DIR/meta.txt, DIR/frame_K.txt, DIR/image_K.bin, DIR/masks_K.bin; floats are written as C hex floats)
// prints per frame "frame K ids ..." : the track_id of every detection in the frame's order.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "orb_slam2_adapter.hpp"

using namespace ORB_SLAM2;

static std::vector<uint8_t> read_bytes(const std::string& path, size_t want) {
    std::ifstream f(path, std::ios::binary);
    std::vector<uint8_t> v((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (!f.good() && !f.eof()) throw std::runtime_error("cannot read " + path);
    if (v.size() != want) throw std::runtime_error(path + ": unexpected size");
    return v;
}

static float next_float(std::istream& in) {
    std::string t;
    if (!(in >> t)) throw std::runtime_error("frame file: a number is missing");
    return std::strtof(t.c_str(), nullptr);
}

static void expect(std::istream& in, const char* word) {
    std::string t;
    if (!(in >> t) || t != word) throw std::runtime_error(std::string("frame file: expected ") + word);
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
    try {
        const std::string dir = argv[1];
        std::map<std::string, double> meta;
        {
            std::ifstream f(dir + "/meta.txt");
            std::string k, v;
            while (f >> k >> v) meta[k] = std::strtod(v.c_str(), nullptr);
        }
        const int nFrames = (int)meta.at("n_frames"), W = (int)meta.at("width"), H = (int)meta.at("height");
        ObjectMatcher ObjMatcher;
        std::map<int, Object3DView> map3d;   // Map::mspObject3Ds, by mTrackID
        int nNextId = 0;
        ObjectFrameView mLastFrame;
        for (int k = 0; k < nFrames; k++) {
            std::ifstream in(dir + "/frame_" + std::to_string(k) + ".txt");
            ObjectFrameView mCurrentFrame;
            mCurrentFrame.cols = W; mCurrentFrame.rows = H; mCurrentFrame.step = 3 * W;
            mCurrentFrame.fx = (float)meta.at("fx"); mCurrentFrame.fy = (float)meta.at("fy"); mCurrentFrame.cx = (float)meta.at("cx"); mCurrentFrame.cy = (float)meta.at("cy");
            expect(in, "Rwc");
            for (float& v : mCurrentFrame.mRwc) v = next_float(in);
            expect(in, "Ow");
            for (float& v : mCurrentFrame.mOw) v = next_float(in);
            expect(in, "n_det");
            const int n = (int)next_float(in);
            std::vector<uint8_t> image = read_bytes(dir + "/image_" + std::to_string(k) + ".bin", (size_t)H * 3 * W);
            std::vector<uint8_t> masks = read_bytes(dir + "/masks_" + std::to_string(k) + ".bin", (size_t)n * H * W);
            mCurrentFrame.imRGB = image.data();
            std::vector<std::vector<float>> centers(n, std::vector<float>(3));
            for (int j = 0; j < n; j++) {
                Object2DView d;
                expect(in, "det");
                d.label = (int)next_float(in);
                d.x = next_float(in); d.y = next_float(in); d.w = next_float(in); d.h = next_float(in);
                const int nk = (int)next_float(in);
                expect(in, "kps");
                d.kps.resize(3 * (size_t)nk);
                for (float& v : d.kps) v = next_float(in);
                expect(in, "center");   // what the map layer records as ObjectCenterW for this detection (CalculateCenterAndSize is not part of the operator)
                for (float& v : centers[j]) v = next_float(in);
                d.mask = masks.data() + (size_t)j * H * W;
                d.mask_step = W;
                mCurrentFrame.mvObject2Ds.push_back(d);
            }
            mCurrentFrame.mvpObject3Ds.assign(n, -1);
            mCurrentFrame.mvObject3DLabels.assign(n, 0);

            ExtractHSVHistogramsFromMask(ObjMatcher, mCurrentFrame);
            // ---- Tracking::TrackObject ----
            if (k > 0) ObjMatcher.MatchTwoFrame(mLastFrame, mCurrentFrame);
            std::vector<Object3DView> vpMapObject3Ds;
            for (const auto& e : map3d) vpMapObject3Ds.push_back(e.second);   // ascending mTrackID
            ObjMatcher.MatchMapToFrame(vpMapObject3Ds, mCurrentFrame);
            // ---- the map: new objects and new observations ----
            std::printf("frame %d ids", k);
            for (int j = 0; j < n; j++) {
                Object2DView& d = mCurrentFrame.mvObject2Ds[j];
                int id = mCurrentFrame.mvpObject3Ds[j];
                if (id < 0) {
                    id = nNextId++;
                    map3d[id].mTrackID = id;
                    map3d[id].mLabel = d.label;
                    mCurrentFrame.mvpObject3Ds[j] = id;
                    d.track_id = id;
                }
                ObjectObservationView obs;
                std::copy(centers[j].begin(), centers[j].end(), obs.ObjectCenterW);
                std::copy(d.mHSVHistogram, d.mHSVHistogram + OSLAM_OBJMATCH_BINS, obs.AppearanceVec);
                map3d[id].mvObservations.push_back(obs);
                mCurrentFrame.mvObject3DLabels[j] = map3d[id].mLabel;
                std::printf(" %d", d.track_id);
            }
            std::printf("\n");
            mLastFrame = mCurrentFrame;   // (the histograms, boxes and ids; the image and mask pointers are not read again)
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
