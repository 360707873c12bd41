// The body of Tracking::UpdateCurrentObject (reference src/Tracking.cc:1079-1207) over a short list of frames and then Map::ObjectMapRegularization
// (src/Map.cc:67-112), written only against include/orb_slam2_adapter.hpp: per frame the label counts of the map points, Object3D::Update for every detection
// that has an object, and the new-object path (clustering, the shortcut, the two rules) for every detection that has none.
// usage: adapter_object_map_program FILE
//   FILE: "n_points M", M lines "x y z" (C hex floats), "n_frames K", per frame "frame n_kps n_det", n_kps lines "point_index_or_-1 outlier", n_det lines
//   "label track_id_or_-1 n idx ..." (track_id: the object TrackObject gave the detection).
// prints per frame "frame K: id:points ..." and at the end one line per object: ids, counts, and the floats as the hex of their bits.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "orb_slam2_adapter.hpp"

using namespace ORB_SLAM2;

template <class T> static T next(std::istream& in) {
    std::string t;
    if (!(in >> t)) throw std::runtime_error("input: a token is missing");
    return (T)std::strtod(t.c_str(), nullptr);
}

static void expect(std::istream& in, const char* word) {
    std::string t;
    if (!(in >> t) || t != word) throw std::runtime_error(std::string("input: expected ") + word);
}

static unsigned bits(float v) {
    unsigned u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    try {
        std::ifstream in(argv[1]);
        expect(in, "n_points");
        std::vector<MapPointView> points(next<int>(in));
        for (MapPointView& p : points)
            for (float& v : p.mWorldPos) v = next<float>(in);
        expect(in, "n_frames");
        const int nFrames = next<int>(in);
        std::map<int, std::unique_ptr<Object3D>> objects;   // Map::mspObject3Ds, by mTrackID
        for (int k = 0; k < nFrames; k++) {
            expect(in, "frame");
            ObjectFrameView mCurrentFrame;
            const int N = next<int>(in), N_O = next<int>(in);
            for (int i = 0; i < N; i++) {
                const int id = next<int>(in);
                mCurrentFrame.mvpMapPoints.push_back(id < 0 ? nullptr : &points[id]);
                mCurrentFrame.mvbOutlier.push_back(next<int>(in) != 0);
            }
            std::vector<int> vObjectKp(N, -1);   // Frame::mvObjectKpIndices: the detection of every keypoint
            for (int j = 0; j < N_O; j++) {
                Object2DView d;
                d.label = next<int>(in);
                mCurrentFrame.mvpObject3Ds.push_back(next<int>(in));
                const int n = next<int>(in);
                for (int q = 0; q < n; q++) {
                    d.mvFrameKpIndices.push_back(next<int>(in));
                    vObjectKp[d.mvFrameKpIndices.back()] = j;
                }
                mCurrentFrame.mvObject2Ds.push_back(d);
            }
            // ---- Tracking::UpdateCurrentObject(true) ----
            for (int i = 0; i < N; i++) {   // :1083-1099
                MapPointView* pMp = mCurrentFrame.mvpMapPoints[i];
                if (pMp) pMp->AddLabelCnt(vObjectKp[i] >= 0 ? mCurrentFrame.mvObject2Ds[vObjectKp[i]].label : -1);
            }
            for (int i = 0; i < N_O; i++) {   // :1101-1207
                const int id = mCurrentFrame.mvpObject3Ds[i];
                if (id >= 0) {
                    objects.at(id)->Update(i, mCurrentFrame);
                    continue;
                }
                std::vector<MapPointView*> vpCandidateMps;
                for (int idx : mCurrentFrame.mvObject2Ds[i].mvFrameKpIndices)
                    if (mCurrentFrame.mvpMapPoints[idx]) vpCandidateMps.push_back(mCurrentFrame.mvpMapPoints[idx]);
                if (!RejectNewObjectOutliers(vpCandidateMps)) continue;
                std::unique_ptr<Object3D> pObj3D(new Object3D(vpCandidateMps, i, mCurrentFrame));
                mCurrentFrame.mvpObject3Ds[i] = pObj3D->mTrackID;
                objects[pObj3D->mTrackID] = std::move(pObj3D);
            }
            std::printf("frame %d:", k);
            for (const auto& e : objects) std::printf(" %d:%zu", e.first, e.second->mvpMapPoints.size());
            std::printf("\n");
        }
        std::vector<Object3D*> vpObj3Ds;
        for (const auto& e : objects) vpObj3Ds.push_back(e.second.get());   // ascending mTrackID
        const std::vector<Object3D*> erased = ObjectMapRegularization(vpObj3Ds);
        std::printf("erased %zu left %zu\n", erased.size(), vpObj3Ds.size());
        for (const auto& e : objects) {
            const Object3D& o = *e.second;
            std::printf("object %d label %d updates %d valid %d replaced %d obs %zu n %zu center %08x %08x %08x bbox %08x %08x %08x %08x %08x %08x ids", o.mTrackID, o.mLabel, o.mUpdateCnt,
                        o.isVaild() ? 1 : 0, o.mpReplaced ? o.mpReplaced->mTrackID : -1, o.mvObservations.size(), o.mvpMapPoints.size(), bits(o.mCenterW[0]), bits(o.mCenterW[1]),
                        bits(o.mCenterW[2]), bits(o.mMaxXw), bits(o.mMaxYw), bits(o.mMaxZw), bits(o.mMinXw), bits(o.mMinYw), bits(o.mMinZw));
            for (const MapPointView* p : o.mvpMapPoints) std::printf(" %d", (int)(p - points.data()));
            std::printf("\n");
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
