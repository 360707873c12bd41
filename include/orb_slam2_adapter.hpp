// orb_slam2_adapter.hpp — header-only C++ adapter that re-exposes the reference's class API on top of the C ABI in oslam_hip.h:
// ORB_SLAM2::ORBextractor (include/ORBextractor.h:45-110), ORB_SLAM2::ORBmatcher (include/ORBmatcher.h:41-83: the projection searches, the relocalisation one included,
// SearchForInitialization, SearchByBoW (both overloads), SearchForTriangulation, Fuse, SearchBySim3, DescriptorDistance), Frame::ComputeStereoMatches (src/Frame.cc:706), ORB_SLAM2::Optimizer
// (include/Optimizer.h:38-57: PoseOptimization, LocalBundleAdjustment, BundleAdjustment, OptimizeSim3, OptimizeEssentialGraph) and ObjectOptimizer::PoseOptimization2
// (include/ObjectOptimizer.h:23), ORB_SLAM2::ORBVocabulary (include/ORBVocabulary.h: loadFromTextFile, transform, score) ORB_SLAM2::PnPsolver (include/PnPsolver.h: SetRansacParameters, iterate, find) and ORB_SLAM2::Sim3Solver (include/Sim3Solver.h: SetRansacParameters, iterate, find, GetEstimatedRotation / Translation / Scale) and ORB_SLAM2::KeyFrameDatabase (include/KeyFrameDatabase.h: add, erase, clear,
// DetectLoopCandidates, DetectRelocalizationCandidates) and ORB_SLAM2::LoopClosing (include/LoopClosing.h: DetectLoop, the LoopConnections loop of CorrectLoop) over ORB_SLAM2::KeyFrameGraph (KeyFrame's covisibility members, MapPoint's observations, Tracking::UpdateLocalKeyFrames) and ORB_SLAM2::ObjectMatcher (include/ObjectMatcher.h: MatchTwoFrame, MatchMapToFrame) with Frame::ExtractHSVHistogramsFromMask
// (src/Frame.cc:388) as a free function, and ORB_SLAM2::Object3D (include/ObjectTypes.h: Update, RejectOutliers, CalculateCenterAndSize) with RejectNewObjectOutliers
// (the new-object path of Tracking::UpdateCurrentObject) and ObjectMapRegularization / MergeObject (src/Map.cc:67-157) as free functions.  The reference methods walk Frame / KeyFrame / MapPoint pointer graphs; here every method takes a flat
// "view" of exactly the members it reads and writes (the gather loops are in INTEGRATION.md).  tests/adapter_program.cc uses nothing but
// these classes; tests/test_adapter_gpu.py builds it, runs it and compares its outputs with the ctypes path.
//
// It is written against POD mirrors of cv::KeyPoint / cv::Mat so it compiles without OpenCV
// (OpenCV is not installed in the build image).  In the reference tree, define
// OSLAM_ADAPTER_USE_OPENCV before including it: oslam::KeyPoint becomes cv::KeyPoint (identical
// 28-byte layout) and descriptors are cv::Mat CV_8U N x 32.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "oslam_hip.h"

#ifdef OSLAM_ADAPTER_USE_OPENCV
#include <opencv2/core/core.hpp>
#endif

namespace oslam {

#ifdef OSLAM_ADAPTER_USE_OPENCV
typedef cv::KeyPoint KeyPoint;
static_assert(sizeof(cv::KeyPoint) == sizeof(oslam_keypoint_t), "cv::KeyPoint layout");
#else
typedef oslam_keypoint_t KeyPoint;
#endif

struct Image8 {   // CV_8UC1 view
    const uint8_t* data; int cols, rows, step;
    bool empty() const { return !data || cols == 0 || rows == 0; }
};

inline void throw_on(int rc) {
    if (rc != OSLAM_OK) throw std::runtime_error(std::string("oslam: ") + oslam_last_error());
}

}  // namespace oslam

namespace ORB_SLAM2 {

// Same constructor arguments and getters as the reference class; the image geometry is bound at
// the first call (the reference sizes its pyramid per call, src/ORBextractor.cc:1111-1116).
class ORBextractor {
public:
    ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int device = 0)
        : nfeatures_(nfeatures), scaleFactor_(scaleFactor), nlevels_(nlevels), iniTh_(iniThFAST), minTh_(minThFAST),
          device_(device) {}
    ~ORBextractor() { oslam_orb_destroy(h_); }
    ORBextractor(const ORBextractor&) = delete;
    ORBextractor& operator=(const ORBextractor&) = delete;

    // void operator()(InputArray image, InputArray mask /*ignored*/, vector<KeyPoint>&, OutputArray descriptors)
    void operator()(const oslam::Image8& image, std::vector<oslam::KeyPoint>& keypoints,
                    std::vector<uint8_t>& descriptors /* N x 32 row-major */) {
        keypoints.clear();
        descriptors.clear();
        if (image.empty()) return;   // reference: silent return, src/ORBextractor.cc:1046
        ensure(image.cols, image.rows);
        const int cap = oslam_orb_max_keypoints(h_);
        keypoints.resize(cap);
        descriptors.resize((size_t)cap * 32);
        int n = 0;
        oslam::throw_on(oslam_orb_extract(h_, image.data, image.cols, image.rows, image.step,
                                          reinterpret_cast<oslam_keypoint_t*>(keypoints.data()), descriptors.data(), cap, &n));
        keypoints.resize(n);
        descriptors.resize((size_t)n * 32);
    }

    // the reference signature carries a mask argument that it ignores (src/ORBextractor.cc:1043-1044)
    void operator()(const oslam::Image8& image, const oslam::Image8& /*mask: ignored like the reference*/, std::vector<oslam::KeyPoint>& keypoints,
                    std::vector<uint8_t>& descriptors) {
        (*this)(image, keypoints, descriptors);
    }

    int GetLevels() { return nlevels_; }
    float GetScaleFactor() { return scaleFactor_; }
    std::vector<float> GetScaleFactors() { return table(0); }
    std::vector<float> GetInverseScaleFactors() { return table(1); }
    std::vector<float> GetScaleSigmaSquares() { return table(2); }
    std::vector<float> GetInverseScaleSigmaSquares() { return table(3); }

    // mvImagePyramid[level] (public member in the reference, include/ORBextractor.h:85)
    std::vector<uint8_t> ImagePyramidLevel(int level, int& cols, int& rows) {
        oslam::throw_on(oslam_orb_level_size(h_, level, &cols, &rows));
        std::vector<uint8_t> out((size_t)cols * rows);
        oslam::throw_on(oslam_orb_get_pyramid_level(h_, 0, level, out.data()));
        return out;
    }
    oslam_orb_t* handle() { return h_; }

private:
    void ensure(int w, int hgt) {
        if (h_ && w == w_ && hgt == hgt_) return;
        oslam_orb_destroy(h_);
        h_ = nullptr;
        oslam::throw_on(oslam_orb_create(&h_, nfeatures_, scaleFactor_, nlevels_, iniTh_, minTh_, w, hgt, 1, device_));
        w_ = w; hgt_ = hgt;
    }
    std::vector<float> table(int which) {
        // the tables depend only on the constructor arguments: the float chain of src/ORBextractor.cc:415-432, computed on the host (no GPU handle)
        std::vector<float> sc(nlevels_), s2(nlevels_), is(nlevels_), is2(nlevels_);
        sc[0] = 1.f; s2[0] = 1.f;
        const double sf = scaleFactor_;
        for (int i = 1; i < nlevels_; i++) { sc[i] = (float)(sc[i - 1] * sf); s2[i] = sc[i] * sc[i]; }
        for (int i = 0; i < nlevels_; i++) { is[i] = 1.0f / sc[i]; is2[i] = 1.0f / s2[i]; }
        return which == 0 ? sc : which == 1 ? is : which == 2 ? s2 : is2;
    }
    int nfeatures_; float scaleFactor_; int nlevels_, iniTh_, minTh_, device_;
    oslam_orb_t* h_ = nullptr;
    int w_ = 0, hgt_ = 0;
};

// Flat view of the Frame members the projection searches read/write (include/Frame.h).
struct FrameView {
    int N;
    const oslam::KeyPoint* mvKeysUn;
    const float* mvuRight;
    const uint8_t* mDescriptors;          // N x 32
    const uint8_t* blocked;               // mvpMapPoints[i] && mvpMapPoints[i]->Observations()>0
    float mnMinX, mnMinY, mnMaxX, mnMaxY;
};

// Flat view of what ORBmatcher::SearchBySim3 reads of a KeyFrame and of its map points (src/ORBmatcher.cc:1102-1326); one entry per keypoint
struct Sim3MatchKeyFrameView {
    int N;                                // mvKeysUn.size() = GetMapPointMatches().size()
    const oslam::KeyPoint* mvKeysUn;
    const uint8_t* mDescriptors;          // N x 32
    const uint8_t* has_mp;                // pMP && !pMP->isBad()
    const float* Xw;                      // [N][3] pMP->GetWorldPos()
    const uint8_t* mpDescriptors;         // N x 32 pMP->GetDescriptor()
    const float* mfMaxDistance; const float* mfMinDistance;   // the members (GetMaxDistanceInvariance() / 1.2f, GetMinDistanceInvariance() / 0.8f is NOT the same float)
    float Tcw[16];                        // GetPose(), row-major
    float fx, fy, cx, cy;                 // read of KF1 only (:1105-1108)
    float mnMinX, mnMinY, mnMaxX, mnMaxY; // the same for both keyframes (one camera)
    const float* mvScaleFactors; int mnScaleLevels; float mfLogScaleFactor;
};

// Flat views of what ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cc:290-403) and ORBmatcher::Fuse(pKF, Scw, vpPoints, th,
// vpReplacePoint) (:977-1100) read of the keyframe and of the candidate points (LoopClosing's mvpLoopMapPoints)
struct Sim3ProjKeyFrameView {
    int N;                                // mvKeysUn.size()
    const oslam::KeyPoint* mvKeysUn;
    const uint8_t* mDescriptors;          // N x 32
    const uint8_t* mapPointState;         // Fuse only: 0 = GetMapPoint(idx) is NULL, 1 = a point that is not bad, 2 = a bad one
    float fx, fy, cx, cy;
    float mnMinX, mnMinY, mnMaxX, mnMaxY;
    const float* mvScaleFactors; int mnScaleLevels; float mfLogScaleFactor;
};
struct Sim3ProjPointsView {
    int n;                                // vpPoints.size()
    const float* Xw;                      // [n][3] GetWorldPos()
    const float* normal;                  // [n][3] GetNormal()
    const uint8_t* mDescriptors;          // n x 32 GetDescriptor()
    const float* mfMaxDistance; const float* mfMinDistance;   // the members, as in Sim3MatchKeyFrameView
    const uint8_t* skip;                  // pMP->isBad() || spAlreadyFound.count(pMP) (:317 / :1005); NULL: no point is skipped
};

// Flat views of what ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1472-1599) reads of the frame and of the
// keyframe's map-point slots (Tracking::Relocalization, src/Tracking.cc:1717, :1731)
struct RelocFrameView {
    int N;                                // mvKeysUn.size()
    const oslam::KeyPoint* mvKeysUn;      // pt, octave and angle are read
    const uint8_t* mDescriptors;          // N x 32
    float Tcw[16];                        // mTcw, row-major
    float fx, fy, cx, cy;
    float mnMinX, mnMinY, mnMaxX, mnMaxY;
    const float* mvScaleFactors; int mnScaleLevels; float mfLogScaleFactor;
};
struct RelocKeyFrameView {                // one entry per slot i of pKF->GetMapPointMatches()
    int n;
    const float* Xw;                      // [n][3] pMP->GetWorldPos()
    const uint8_t* mDescriptors;          // n x 32 pMP->GetDescriptor()
    const float* mfMaxDistance; const float* mfMinDistance;   // the members, as in Sim3MatchKeyFrameView
    const float* angle;                   // pKF->mvKeysUn[i].angle
    const uint8_t* skip;                  // pMP == NULL || pMP->isBad() || sAlreadyFound.count(pMP) (:1492-1494); the other rows of a skipped slot are not read
};

// Flat view of what ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:405-520) reads of a Frame (Tracking::MonocularInitialization, src/Tracking.cc:681)
struct InitMatchFrameView {
    int N;                                // mvKeysUn.size()
    const oslam::KeyPoint* mvKeysUn;      // pt, octave and angle are read
    const uint8_t* mDescriptors;          // N x 32
    float mnMinX, mnMinY, mnMaxX, mnMaxY;
};
#ifdef OSLAM_ADAPTER_USE_OPENCV
typedef cv::Point2f Point2f;
#else
struct Point2f { float x, y; };
#endif
static_assert(sizeof(Point2f) == 2 * sizeof(float), "vbPrevMatched is handed over as float [.][2]");

class ORBmatcher {
public:
    static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;   // src/ORBmatcher.cc:37-39
    ORBmatcher(float nnratio = 0.6f, bool checkOri = true, int max_keypoints = 2400, int max_queries = 8192, int device = 0)
        : mfNNratio(nnratio), mbCheckOrientation(checkOri) {
        oslam::throw_on(oslam_matcher_create(&h_, 1, max_keypoints, max_queries, device));
    }
    ~ORBmatcher() { oslam_matcher_destroy(h_); oslam_bow_destroy(bow_); oslam_sim3_match_destroy(sim3m_); oslam_sim3_proj_destroy(sim3p_); oslam_reloc_proj_destroy(relocp_); oslam_init_match_destroy(initm_); }
    ORBmatcher(const ORBmatcher&) = delete;

    // int SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, const float th):
    // the caller gathers one oslam_proj_query_t per map point (INTEGRATION.md shows the loop) and
    // applies kp_match[k] >= 0  =>  F.mvpMapPoints[k] = vpMapPoints[kp_match[k]].
    int SearchByProjection(const FrameView& F, const std::vector<oslam_proj_query_t>& queries, std::vector<int32_t>& kp_match,
                           std::vector<int32_t>* q_match = nullptr) {
        const float bounds[4] = {F.mnMinX, F.mnMinY, F.mnMaxX, F.mnMaxY};
        kp_match.assign(F.N > 0 ? F.N : 1, -1);
        std::vector<int32_t> qm(queries.size() + 1), qd(queries.size() + 1);
        int32_t nm = 0;
        oslam::throw_on(oslam_match_search_by_projection(h_, F.N, reinterpret_cast<const oslam_keypoint_t*>(F.mvKeysUn), F.mvuRight,
                                                         F.mDescriptors, F.blocked, bounds, queries.data(), (int)queries.size(),
                                                         mfNNratio, 1, 0, qm.data(), qd.data(), kp_match.data(), &nm));
        kp_match.resize(F.N);
        if (q_match) { qm.resize(queries.size()); *q_match = qm; }
        return nm;
    }

    // int SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono)
    int SearchByProjection(const FrameView& Cur, int Nlast, const float* lastXw, const uint8_t* last_has_mp,
                           const oslam::KeyPoint* lastKeysUn, const uint8_t* lastMpDesc, const float Tcw[16], const float Tlw[16],
                           const oslam_camera_t& cam, const std::vector<float>& scaleFactors, float th, bool bMono,
                           std::vector<int32_t>& kp_match) {
        const float bounds[4] = {Cur.mnMinX, Cur.mnMinY, Cur.mnMaxX, Cur.mnMaxY};
        kp_match.assign(Cur.N > 0 ? Cur.N : 1, -1);
        std::vector<int32_t> qm(Nlast + 1), qd(Nlast + 1);
        int32_t nm = 0;
        oslam::throw_on(oslam_match_project_last_frame(h_, Cur.N, reinterpret_cast<const oslam_keypoint_t*>(Cur.mvKeysUn), Cur.mvuRight,
                                                       Cur.mDescriptors, Cur.blocked, bounds, Nlast, lastXw, last_has_mp,
                                                       reinterpret_cast<const oslam_keypoint_t*>(lastKeysUn), lastMpDesc, Tcw, Tlw, &cam,
                                                       scaleFactors.data(), (int)scaleFactors.size(), th, bMono ? 1 : 0,
                                                       mbCheckOrientation ? 1 : 0, qm.data(), qd.data(), kp_match.data(), &nm));
        kp_match.resize(Cur.N);
        return nm;
    }

    // static int DescriptorDistance(const cv::Mat &a, const cv::Mat &b) (src/ORBmatcher.cc:1647-1663)
    static int DescriptorDistance(const uint8_t* a, const uint8_t* b) {
        int d = 0;
        for (int i = 0; i < 8; i++) {
            uint32_t x, y;
            memcpy(&x, a + 4 * i, 4); memcpy(&y, b + 4 * i, 4);
            d += __builtin_popcount(x ^ y);
        }
        return d;
    }

    // int Fuse(KeyFrame* pKF, const vector<MapPoint*> &vpMapPoints, const float th) (src/ORBmatcher.cc:825-975), search half: the caller gathers
    // one query per candidate point that passes the projection gates (:840-890) and applies the surgery (:950-970) in query order
    // for q_match[i] >= 0.  Returns the number of fused points.
    int Fuse(const FrameView& KF, const std::vector<oslam_proj_query_t>& queries, const std::vector<float>& invLevelSigma2, std::vector<int32_t>& q_match) {
        const float bounds[4] = {KF.mnMinX, KF.mnMinY, KF.mnMaxX, KF.mnMaxY};
        q_match.assign(queries.size() + 1, -1);
        std::vector<int32_t> qd(queries.size() + 1);
        int32_t nf = 0;
        oslam::throw_on(oslam_match_fuse_search(h_, KF.N, reinterpret_cast<const oslam_keypoint_t*>(KF.mvKeysUn), KF.mvuRight, KF.mDescriptors, bounds,
                                                queries.data(), (int)queries.size(), invLevelSigma2.data(), (int)invLevelSigma2.size(), q_match.data(),
                                                qd.data(), &nf));
        q_match.resize(queries.size());
        return nf;
    }

    // DBoW2::FeatureVector of one side (node id -> keypoint indices), flattened as oslam_hip.h describes (ORBVocabulary::flatten below builds it)
    struct FeatureVector {
        std::vector<int32_t> q_idx; std::vector<uint32_t> q_node;               // side 1: (node ascending, index order)
        std::vector<uint32_t> nodes; std::vector<int32_t> start, items;        // side 2: CSR over the sorted unique node ids
    };

    // int SearchByBoW(KeyFrame* pKF, Frame &F, vector<MapPoint*> &vpMapPointMatches) (:159-288): match_f[k] = keyframe keypoint whose map point goes to
    // vpMapPointMatches[k]; kf_has_good_mp[i] = pKF's map point i exists and is not bad
    int SearchByBoW(const FrameView& KF, const FeatureVector& fvKF, const uint8_t* kf_has_good_mp, const FrameView& F, const FeatureVector& fvF,
                    std::vector<int32_t>& match_f) {
        ensure_bow();
        oslam_bow_side1_t s1 = {KF.N, reinterpret_cast<const oslam_keypoint_t*>(KF.mvKeysUn), KF.mDescriptors, nullptr, kf_has_good_mp,
                                (int32_t)fvKF.q_idx.size(), fvKF.q_idx.data(), fvKF.q_node.data()};
        oslam_bow_side2_t s2 = {F.N, reinterpret_cast<const oslam_keypoint_t*>(F.mvKeysUn), F.mDescriptors, nullptr, nullptr,
                                (int32_t)fvF.nodes.size(), fvF.nodes.data(), fvF.start.data(), fvF.items.data()};
        match_f.assign(F.N + 1, -1);
        int32_t nm = 0;
        oslam::throw_on(oslam_match_search_by_bow(bow_, &s1, &s2, mfNNratio, mbCheckOrientation ? 1 : 0, match_f.data(), &nm));
        match_f.resize(F.N);
        return nm;
    }

    // int SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12) (:522-655), the first step of LoopClosing::ComputeSim3: match12[i] = keypoint
    // of KF2 whose map point goes to vpMatches12[i] (-1 none, -2 removed by the rotation check); kfN_has_good_mp[i] = the map point exists and is not bad
    int SearchByBoW(const FrameView& KF1, const FeatureVector& fv1, const uint8_t* kf1_has_good_mp, const FrameView& KF2, const FeatureVector& fv2,
                    const uint8_t* kf2_has_good_mp, std::vector<int32_t>& match12) {
        ensure_bow();
        oslam_bow_side1_t s1 = {KF1.N, reinterpret_cast<const oslam_keypoint_t*>(KF1.mvKeysUn), KF1.mDescriptors, nullptr, kf1_has_good_mp,
                                (int32_t)fv1.q_idx.size(), fv1.q_idx.data(), fv1.q_node.data()};
        oslam_bow_side2_t s2 = {KF2.N, reinterpret_cast<const oslam_keypoint_t*>(KF2.mvKeysUn), KF2.mDescriptors, nullptr, kf2_has_good_mp,
                                (int32_t)fv2.nodes.size(), fv2.nodes.data(), fv2.start.data(), fv2.items.data()};
        match12.assign(KF1.N + 1, -1);
        int32_t nm = 0;
        oslam::throw_on(oslam_match_search_by_bow_kf(bow_, &s1, &s2, mfNNratio, mbCheckOrientation ? 1 : 0, match12.data(), &nm));
        match12.resize(KF1.N);
        return nm;
    }

    // int SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12, vector<pair<size_t,size_t>> &vMatchedPairs, const bool bOnlyStereo) (:657-823):
    // match12[i] = keypoint of KF2 matched to keypoint i of KF1 or -1; (ex, ey) = epipole of camera 1 in image 2 (:663-670)
    int SearchForTriangulation(const FrameView& KF1, const FeatureVector& fv1, const uint8_t* kf1_has_mp, const FrameView& KF2, const FeatureVector& fv2,
                               const uint8_t* kf2_has_mp, const float F12[9], float ex, float ey, const std::vector<float>& scaleFactors,
                               const std::vector<float>& levelSigma2, bool bOnlyStereo, std::vector<int32_t>& match12) {
        ensure_bow();
        oslam_bow_side1_t s1 = {KF1.N, reinterpret_cast<const oslam_keypoint_t*>(KF1.mvKeysUn), KF1.mDescriptors, KF1.mvuRight, kf1_has_mp,
                                (int32_t)fv1.q_idx.size(), fv1.q_idx.data(), fv1.q_node.data()};
        oslam_bow_side2_t s2 = {KF2.N, reinterpret_cast<const oslam_keypoint_t*>(KF2.mvKeysUn), KF2.mDescriptors, KF2.mvuRight, kf2_has_mp,
                                (int32_t)fv2.nodes.size(), fv2.nodes.data(), fv2.start.data(), fv2.items.data()};
        match12.assign(KF1.N + 1, -1);
        int32_t nm = 0;
        oslam::throw_on(oslam_match_search_for_triangulation(bow_, &s1, &s2, F12, ex, ey, scaleFactors.data(), levelSigma2.data(), (int)scaleFactors.size(),
                                                             bOnlyStereo ? 1 : 0, mbCheckOrientation ? 1 : 0, match12.data(), &nm));
        match12.resize(KF1.N);
        return nm;
    }

    // int SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12, const float& s12, const cv::Mat& R12, const cv::Mat& t12, const float th)
    // (:1102-1326).  vpMatches12 [KF1.N]: -1 = NULL, otherwise pMP->GetIndexInKeyFrame(pKF2) of the matched point (-2: matched, not in KF2); where the
    // reference sets vpMatches12[i1] = vpMapPoints2[idx2] the entry becomes idx2.  R12 3 x 3 row-major.  Returns nFound.
    int SearchBySim3(const Sim3MatchKeyFrameView& KF1, const Sim3MatchKeyFrameView& KF2, std::vector<int32_t>& vpMatches12, float s12, const float R12[9], const float t12[3],
                     float th) {
        if ((int)vpMatches12.size() != KF1.N) throw std::runtime_error("SearchBySim3: vpMatches12 must have one entry per keypoint of KF1");
        if (!sim3m_) oslam::throw_on(oslam_sim3_match_create(&sim3m_, 1, 2400, 0));
        const Sim3MatchKeyFrameView* kf[2] = {&KF1, &KF2};
        const size_t n = (size_t)KF1.N + (size_t)KF2.N;
        std::vector<oslam_keypoint_t> keys(n);
        std::vector<uint8_t> desc(n * 32), has(n), mpd(n * 32);
        std::vector<float> Xw(n * 3), maxD(n), minD(n);
        size_t at = 0;
        for (int k = 0; k < 2; k++) {   // rows 0 .. N1 - 1 are KF1's, the rest KF2's
            const size_t m = (size_t)kf[k]->N;
            if (m) {
                memcpy(keys.data() + at, kf[k]->mvKeysUn, m * sizeof(oslam_keypoint_t)); memcpy(desc.data() + at * 32, kf[k]->mDescriptors, m * 32);
                memcpy(has.data() + at, kf[k]->has_mp, m); memcpy(Xw.data() + at * 3, kf[k]->Xw, m * 12); memcpy(mpd.data() + at * 32, kf[k]->mpDescriptors, m * 32);
                memcpy(maxD.data() + at, kf[k]->mfMaxDistance, m * 4); memcpy(minD.data() + at, kf[k]->mfMinDistance, m * 4);
            }
            at += m;
        }
        oslam_sim3_pair_t pr;
        pr.n1 = KF1.N; pr.off1 = 0; pr.n2 = KF2.N; pr.off2 = KF1.N; pr.out_off = 0; pr.s12 = s12; pr.th = th;
        memcpy(pr.R12, R12, sizeof(pr.R12)); memcpy(pr.t12, t12, sizeof(pr.t12)); memcpy(pr.T1w, KF1.Tcw, sizeof(pr.T1w)); memcpy(pr.T2w, KF2.Tcw, sizeof(pr.T2w));
        const oslam_sim3_match_rows_t rows = {(int32_t)n, keys.data(), desc.data(), has.data(), Xw.data(), mpd.data(), maxD.data(), minD.data()};
        const oslam_camera_t cam = {KF1.fx, KF1.fy, KF1.cx, KF1.cy, 0.f, 0.f};
        const float bounds[4] = {KF1.mnMinX, KF1.mnMinY, KF1.mnMaxX, KF1.mnMaxY};
        std::vector<int32_t> match12((size_t)KF1.N + 1, -1);
        int32_t nFound = 0;
        oslam::throw_on(oslam_match_search_by_sim3_batch(sim3m_, 1, &pr, &rows, KF1.N, vpMatches12.data(), &cam, bounds, KF1.mvScaleFactors, KF1.mnScaleLevels, KF1.mfLogScaleFactor,
                                                         match12.data(), &nFound));
        if (nFound < 0) return 0;   // (a Sim3 or pose that is not finite: nothing matches)
        for (int i1 = 0; i1 < KF1.N; i1++)
            if (match12[i1] >= 0) vpMatches12[i1] = match12[i1];
        return nFound;
    }

    // int SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched, int th) (:290-403).  Scw 4 x 4 row-major.
    // vpMatched [KF.N]: -1 = NULL, any other value on entry = a matched point; where the reference sets vpMatched[bestIdx] = pMP the entry becomes the point's index
    // in `points`.  Returns nmatches.
    int SearchByProjection(const Sim3ProjKeyFrameView& KF, const float Scw[16], const Sim3ProjPointsView& points, std::vector<int32_t>& vpMatched, float th) {
        if ((int)vpMatched.size() != KF.N) throw std::runtime_error("SearchByProjection: vpMatched must have one entry per keypoint of the keyframe");
        ensure_proj(points.n);
        std::vector<uint8_t> state((size_t)KF.N + 1);
        for (int k = 0; k < KF.N; k++) state[k] = vpMatched[k] != -1;
        const oslam_sim3_proj_problem_t pr = proj_problem(KF, Scw, points, th);
        const oslam_sim3_proj_kf_rows_t kf = {KF.N, reinterpret_cast<const oslam_keypoint_t*>(KF.mvKeysUn), KF.mDescriptors, state.data()};
        const oslam_sim3_proj_pt_rows_t pts = {points.n, points.Xw, points.normal, points.mDescriptors, points.mfMaxDistance, points.mfMinDistance};
        const oslam_camera_t cam = {KF.fx, KF.fy, KF.cx, KF.cy, 0.f, 0.f};
        const float bounds[4] = {KF.mnMinX, KF.mnMinY, KF.mnMaxX, KF.mnMaxY};
        std::vector<int32_t> matched((size_t)KF.N + 1, -1);
        int32_t nmatches = 0;
        oslam::throw_on(oslam_match_search_by_projection_sim3_batch(sim3p_, 1, &pr, &kf, &pts, points.n, points.skip, KF.N, &cam, bounds, KF.mvScaleFactors, KF.mnScaleLevels,
                                                                    KF.mfLogScaleFactor, matched.data(), &nmatches, nullptr));
        if (nmatches < 0) return 0;   // (an Scw that is not finite or has no positive scale: nothing matches)
        for (int k = 0; k < KF.N; k++)
            if (matched[k] >= 0) vpMatched[k] = matched[k];
        return nmatches;
    }

    // int Fuse(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, float th, vector<MapPoint*>& vpReplacePoint) (:977-1100).  The surgery is reported:
    // vpReplacePoint [points.n] is -1 = NULL, OSLAM_FUSE_OCCUPANT = the keyframe's own point at fusedKp[i] (pKF->GetMapPoint(fusedKp[i])), or p >= 0 = points[p],
    // which this call added at that keypoint earlier; addedKp [points.n] (may be NULL) is bestIdx where the reference calls pMP->AddObservation(pKF, bestIdx) and
    // pKF->AddMapPoint(pMP, bestIdx), -1 elsewhere; fusedKp [points.n] (may be NULL) is bestIdx of every point that counts in nFused.  Returns nFused.
    int Fuse(const Sim3ProjKeyFrameView& KF, const float Scw[16], const Sim3ProjPointsView& points, float th, std::vector<int32_t>& vpReplacePoint,
             std::vector<int32_t>* addedKp = nullptr, std::vector<int32_t>* fusedKp = nullptr) {
        if ((int)vpReplacePoint.size() != points.n) throw std::runtime_error("Fuse: vpReplacePoint must have one entry per point");
        if (KF.N > 0 && !KF.mapPointState) throw std::runtime_error("Fuse: the keyframe view has no mapPointState");
        ensure_proj(points.n);
        const oslam_sim3_proj_problem_t pr = proj_problem(KF, Scw, points, th);
        const oslam_sim3_proj_kf_rows_t kf = {KF.N, reinterpret_cast<const oslam_keypoint_t*>(KF.mvKeysUn), KF.mDescriptors, KF.mapPointState};
        const oslam_sim3_proj_pt_rows_t pts = {points.n, points.Xw, points.normal, points.mDescriptors, points.mfMaxDistance, points.mfMinDistance};
        const oslam_camera_t cam = {KF.fx, KF.fy, KF.cx, KF.cy, 0.f, 0.f};
        const float bounds[4] = {KF.mnMinX, KF.mnMinY, KF.mnMaxX, KF.mnMaxY};
        std::vector<int32_t> fused((size_t)points.n + 1, -1), replace((size_t)points.n + 1, -1);
        int32_t nFused = 0;
        oslam::throw_on(oslam_match_fuse_sim3_batch(sim3p_, 1, &pr, &kf, &pts, points.n, points.skip, &cam, bounds, KF.mvScaleFactors, KF.mnScaleLevels, KF.mfLogScaleFactor,
                                                    fused.data(), replace.data(), &nFused));
        if (addedKp) addedKp->assign((size_t)points.n, -1);
        if (fusedKp) fusedKp->assign((size_t)points.n, -1);
        if (nFused < 0) return 0;
        for (int i = 0; i < points.n; i++) {
            if (replace[i] == OSLAM_FUSE_ADDED) { if (addedKp) (*addedKp)[i] = fused[i]; }
            else if (replace[i] != -1) vpReplacePoint[i] = replace[i];
            if (fusedKp) (*fusedKp)[i] = fused[i];
        }
        return nFused;
    }

    // int SearchByProjection(Frame &CurrentFrame, KeyFrame* pKF, const set<MapPoint*> &sAlreadyFound, const float th, const int ORBdist) (:1472-1599).
    // mvpMapPoints [F.N] is CurrentFrame.mvpMapPoints: -1 = NULL, any other value on entry = a point the frame holds; where the reference sets
    // mvpMapPoints[bestIdx2] = pMP and the rotation histogram leaves it, the entry becomes the slot index i of the keyframe (pMP = vpMPs[i]).  Returns nmatches.
    int SearchByProjection(const RelocFrameView& F, const RelocKeyFrameView& KF, std::vector<int32_t>& mvpMapPoints, float th, int ORBdist) {
        if ((int)mvpMapPoints.size() != F.N) throw std::runtime_error("SearchByProjection: mvpMapPoints must have one entry per keypoint of the frame");
        if (KF.n < 0) throw std::runtime_error("ORBmatcher: negative slot count");
        if (!relocp_ || KF.n > relocp_cap_) {   // made at the first call and again when a keyframe has more slots than it holds
            oslam_reloc_proj_destroy(relocp_);
            relocp_ = nullptr;
            relocp_cap_ = KF.n > 16384 ? KF.n : 16384;
            oslam::throw_on(oslam_reloc_proj_create(&relocp_, 1, 2400, relocp_cap_, 0));
        }
        std::vector<uint8_t> has_mp((size_t)F.N + 1);
        for (int k = 0; k < F.N; k++) has_mp[k] = mvpMapPoints[k] != -1;
        oslam_reloc_proj_problem_t pr;
        pr.n_kp = F.N; pr.kp_off = 0; pr.n_pts = KF.n; pr.pt_off = 0; pr.kp_out_off = 0; pr.pt_out_off = 0; pr.th = th; pr.ORBdist = ORBdist;
        memcpy(pr.Tcw, F.Tcw, sizeof(pr.Tcw));
        const oslam_reloc_proj_frame_rows_t fr = {F.N, reinterpret_cast<const oslam_keypoint_t*>(F.mvKeysUn), F.mDescriptors, has_mp.data()};
        const oslam_reloc_proj_pt_rows_t pts = {KF.n, KF.Xw, KF.mDescriptors, KF.mfMaxDistance, KF.mfMinDistance, KF.angle};
        const oslam_camera_t cam = {F.fx, F.fy, F.cx, F.cy, 0.f, 0.f};
        const float bounds[4] = {F.mnMinX, F.mnMinY, F.mnMaxX, F.mnMaxY};
        std::vector<int32_t> matched((size_t)F.N + 1, -1);
        int32_t nmatches = 0;
        oslam::throw_on(oslam_match_search_by_projection_reloc_batch(relocp_, 1, &pr, &fr, &pts, KF.n, KF.skip, F.N, &cam, bounds, F.mvScaleFactors, F.mnScaleLevels,
                                                                     F.mfLogScaleFactor, mbCheckOrientation ? 1 : 0, matched.data(), &nmatches, nullptr, nullptr));
        if (nmatches < 0) return 0;   // (a pose that is not finite: nothing matches)
        for (int k = 0; k < F.N; k++)
            if (matched[k] >= 0) mvpMapPoints[k] = matched[k];
        return nmatches;
    }

    // int SearchForInitialization(Frame &F1, Frame &F2, std::vector<cv::Point2f> &vbPrevMatched, std::vector<int> &vnMatches12, int windowSize=10) (:405-520).
    // vbPrevMatched [F1.N]: the carried points, read as the window centres and updated for the surviving matches; vnMatches12 is resized to F1.N.  The image
    // bounds are F2's (the frame GetFeaturesInArea is asked of).  Returns nmatches.
    int SearchForInitialization(const InitMatchFrameView& F1, const InitMatchFrameView& F2, std::vector<Point2f>& vbPrevMatched, std::vector<int>& vnMatches12, int windowSize = 10) {
        if (F1.N < 0 || F2.N < 0) throw std::runtime_error("SearchForInitialization: negative key count");
        if ((int)vbPrevMatched.size() != F1.N) throw std::runtime_error("SearchForInitialization: vbPrevMatched must have one entry per key of F1");
        if (!initm_ || F1.N > initm_cap_) {   // made at the first call and again when F1 has more keys than it holds
            oslam_init_match_destroy(initm_);
            initm_ = nullptr;
            initm_cap_ = F1.N > 16384 ? F1.N : 16384;
            oslam::throw_on(oslam_init_match_create(&initm_, 1, 2400, initm_cap_, 0));
        }
        oslam_init_match_problem_t pr;
        pr.n1 = F1.N; pr.off1 = 0; pr.n2 = F2.N; pr.off2 = 0; pr.windowSize = windowSize; pr.reserved = 0;
        const oslam_init_match_f1_rows_t r1 = {F1.N, reinterpret_cast<const oslam_keypoint_t*>(F1.mvKeysUn), F1.mDescriptors};
        const oslam_init_match_f2_rows_t r2 = {F2.N, reinterpret_cast<const oslam_keypoint_t*>(F2.mvKeysUn), F2.mDescriptors};
        const float bounds[4] = {F2.mnMinX, F2.mnMinY, F2.mnMaxX, F2.mnMaxY};
        std::vector<int32_t> m12((size_t)F1.N + 1, -1);
        std::vector<float> prev(2 * (size_t)F1.N + 2);
        if (F1.N) memcpy(prev.data(), vbPrevMatched.data(), 2 * (size_t)F1.N * sizeof(float));
        int32_t nmatches = 0;
        oslam::throw_on(oslam_match_search_for_initialization_batch(initm_, 1, &pr, &r1, &r2, bounds, mfNNratio, mbCheckOrientation ? 1 : 0, prev.data(), m12.data(), &nmatches,
                                                                    nullptr, nullptr, nullptr));
        if (F1.N) memcpy(vbPrevMatched.data(), prev.data(), 2 * (size_t)F1.N * sizeof(float));
        vnMatches12.assign(m12.begin(), m12.begin() + F1.N);
        return nmatches;
    }

    float mfNNratio;
    bool mbCheckOrientation;

private:
    // the handle SearchByProjection(pKF, Scw, ...) and Fuse(pKF, Scw, ...) share, made at the first call and again when a list is longer than it holds
    void ensure_proj(int n_points) {
        if (n_points < 0) throw std::runtime_error("ORBmatcher: negative point count");
        if (sim3p_ && n_points <= sim3p_cap_) return;
        oslam_sim3_proj_destroy(sim3p_);
        sim3p_ = nullptr;
        sim3p_cap_ = n_points > 16384 ? n_points : 16384;
        oslam::throw_on(oslam_sim3_proj_create(&sim3p_, 1, 2400, sim3p_cap_, 0));
    }
    static oslam_sim3_proj_problem_t proj_problem(const Sim3ProjKeyFrameView& KF, const float Scw[16], const Sim3ProjPointsView& points, float th) {
        oslam_sim3_proj_problem_t pr;
        pr.n_kp = KF.N; pr.kp_off = 0; pr.n_pts = points.n; pr.pt_off = 0; pr.kp_out_off = 0; pr.pt_out_off = 0; pr.th = th;
        memcpy(pr.Scw, Scw, sizeof(pr.Scw));
        return pr;
    }
    void ensure_bow() { if (!bow_) oslam::throw_on(oslam_bow_create(&bow_, 2400, 0)); }
    oslam_matcher_t* h_ = nullptr;
    oslam_bow_t* bow_ = nullptr;
    oslam_sim3_match_t* sim3m_ = nullptr;
    oslam_sim3_proj_t* sim3p_ = nullptr;
    int sim3p_cap_ = 0;
    oslam_reloc_proj_t* relocp_ = nullptr;
    int relocp_cap_ = 0;
    oslam_init_match_t* initm_ = nullptr;
    int initm_cap_ = 0;
};

}  // namespace ORB_SLAM2

namespace DBoW2 {
typedef std::map<unsigned, double> BowVector;                      // word id -> value (DBoW2/BowVector.h)
typedef std::map<unsigned, std::vector<unsigned>> FeatureVector;   // node id -> feature indices, ascending (DBoW2/FeatureVector.h)
}  // namespace DBoW2

namespace ORB_SLAM2 {

// typedef DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB> ORBVocabulary (include/ORBVocabulary.h): the three members the
// reference calls — loadFromTextFile (src/System.cc:68), transform(desc, BowVector, FeatureVector, levelsup) (src/Frame.cc:640,
// src/KeyFrame.cc:66, src/ObjectTypes.cc:30) and score — over the oslam_voc_* functions of oslam_hip.h (see there for the format, the algorithms
// and the one normalisation).  transform runs the gfx950 kernel; only L1_NORM vocabularies (the reference's ORBvoc.txt) are scored.
class ORBVocabulary {
public:
    ORBVocabulary() {}
    ~ORBVocabulary() { oslam_voc_destroy(h_); }
    ORBVocabulary(const ORBVocabulary&) = delete;
    ORBVocabulary& operator=(const ORBVocabulary&) = delete;

    // false when the file cannot be read or does not parse (oslam_last_error() says which line)
    bool loadFromTextFile(const std::string& filename) {
        oslam_voc_destroy(h_);
        h_ = nullptr;
        return oslam_voc_load_text(&h_, filename.c_str()) == OSLAM_OK;
    }
    bool empty() const { return !h_; }
    const oslam_voc_t* handle() const { return h_; }   // for oslam_slam_set_vocabulary

    // void transform(const std::vector<TDescriptor>& features, BowVector &v, FeatureVector &fv, int levelsup) const; descriptors N x 32 row-major
    // (the reference converts mDescriptors with Converter::toDescriptorVector first: the same bytes)
    void transform(const std::vector<uint8_t>& descriptors, DBoW2::BowVector& v, DBoW2::FeatureVector& fv, int levelsup) const {
        v.clear();
        fv.clear();
        const int n = (int)(descriptors.size() / 32);
        if (n == 0) return;
        std::vector<uint32_t> word(n), node(n), bow_ids(n), fv_nodes(n);
        std::vector<double> weight(n), bow_vals(n);
        std::vector<int32_t> fv_start(n + 1), fv_items(n);
        int32_t nb = 0, nf = 0;
        oslam::throw_on(oslam_voc_transform(h_, descriptors.data(), n, levelsup, word.data(), node.data(), weight.data()));
        oslam::throw_on(oslam_voc_vectors(h_, n, word.data(), node.data(), weight.data(), bow_ids.data(), bow_vals.data(), &nb, fv_nodes.data(), fv_start.data(),
                                          fv_items.data(), &nf));
        for (int j = 0; j < nb; j++) v[bow_ids[j]] = bow_vals[j];
        for (int r = 0; r < nf; r++) fv[fv_nodes[r]].assign(fv_items.begin() + fv_start[r], fv_items.begin() + fv_start[r + 1]);
    }

    // double score(const BowVector &a, const BowVector &b) const
    double score(const DBoW2::BowVector& a, const DBoW2::BowVector& b) const {
        std::vector<uint32_t> ia, ib;
        std::vector<double> va, vb;
        for (const auto& e : a) { ia.push_back(e.first); va.push_back(e.second); }
        for (const auto& e : b) { ib.push_back(e.first); vb.push_back(e.second); }
        int rc = OSLAM_OK;
        const double s = oslam_voc_score(h_, (int)ia.size(), ia.data(), va.data(), (int)ib.size(), ib.data(), vb.data(), &rc);
        oslam::throw_on(rc);
        return s;
    }

    // The flat views ORBmatcher::SearchByBoW / SearchForTriangulation take, from a DBoW2::FeatureVector (std::map order = node ascending)
    static ORBmatcher::FeatureVector flatten(const DBoW2::FeatureVector& fv) {
        ORBmatcher::FeatureVector out;
        for (const auto& e : fv) {
            out.nodes.push_back(e.first);
            out.start.push_back((int32_t)out.items.size());
            for (unsigned i : e.second) { out.items.push_back((int32_t)i); out.q_idx.push_back((int32_t)i); out.q_node.push_back(e.first); }
        }
        out.start.push_back((int32_t)out.items.size());
        return out;
    }

private:
    oslam_voc_t* h_ = nullptr;
};

// void Frame::ComputeStereoMatches() (src/Frame.cc:706-880): reads the two extractors' pyramids (mvImagePyramid) where they are, in HBM
inline void ComputeStereoMatches(ORBextractor& left, ORBextractor& right, const std::vector<oslam::KeyPoint>& mvKeys, const std::vector<uint8_t>& mDescriptors,
                                 const std::vector<oslam::KeyPoint>& mvKeysRight, const std::vector<uint8_t>& mDescriptorsRight, float mbf, float mb,
                                 std::vector<float>& mvuRight, std::vector<float>& mvDepth) {
    oslam_stereo_t* st = nullptr;
    oslam::throw_on(oslam_stereo_create(&st, 1, 2400, 0));
    mvuRight.assign(mvKeys.size() + 1, -1.f); mvDepth.assign(mvKeys.size() + 1, -1.f);
    const int rc = oslam_stereo_match(st, left.handle(), right.handle(), (int)mvKeys.size(), reinterpret_cast<const oslam_keypoint_t*>(mvKeys.data()),
                                      mDescriptors.data(), (int)mvKeysRight.size(), reinterpret_cast<const oslam_keypoint_t*>(mvKeysRight.data()),
                                      mDescriptorsRight.data(), left.GetLevels(), mbf, mb, mvuRight.data(), mvDepth.data());
    oslam_stereo_destroy(st);
    oslam::throw_on(rc);
    mvuRight.resize(mvKeys.size()); mvDepth.resize(mvKeys.size());
}

// Flat view of what Optimizer::PoseOptimization reads from / writes to a Frame (src/Optimizer.cc:239-451)
struct PoseFrameView {
    int N;
    float* mTcw;                          // 4x4 row-major CV_32F: input estimate, overwritten by SetPose
    const float* Xw;                      // [N][3] pMP->GetWorldPos() where has_mp[i]
    const uint8_t* has_mp;                // mvpMapPoints[i] != NULL
    const oslam::KeyPoint* mvKeysUn;
    const float* mvuRight;
    const float* mvInvLevelSigma2;        // [nLevels]
    uint8_t* mvbOutlier;                  // [N] out
    float fx, fy, cx, cy, mbf;
};

struct SemanticView {                     // what ObjectOptimizer::PoseOptimization2 adds (src/ObjectOptimizer.cc:685-767), see oslam_semantic_t
    int nObj, H, W; const uint8_t* masks;                               // [nObj][H][W] Object2D masks of the matched objects
    int nObjMp; const float* objmp_Xw; const int32_t* objmp_obj;        // map points of the matched Object3Ds
    int nJoint; const int32_t* joint_kp; const int32_t* joint_obj;      // keypoints with a map point of object joint_obj lying outside its Object2D
    float mnMinX, mnMinY, mnMaxX, mnMaxY;
};

// Flat local-BA graph: what Optimizer::LocalBundleAdjustment gathers at src/Optimizer.cc:456-650 and writes back at :746-777
struct BAGraph {
    int nKF; float* poses /*[nKF][16] in/out*/; const uint8_t* fixed /* 0 local, 1 fixed camera, 2 local keyframe with mnId == 0 */;
    int nP; float* points /*[nP][3] in/out*/;
    int nE; const int32_t* edge_kf; const int32_t* edge_pt; const float* edge_obs /*[nE][3] u, v, uR (<0 mono)*/; const float* edge_invSigma2;
    uint8_t* erase;                       // [nE] out: observations the reference erases (:711-757); may be NULL for BundleAdjustment
    float fx, fy, cx, cy, mbf;
};

// Flat view of what Optimizer::OptimizeSim3 reads of a KeyFrame and of its map points (src/Optimizer.cc:1046-1178); one entry per keypoint
struct Sim3OptKeyFrameView {
    int N;                                // mvKeysUn.size() = GetMapPointMatches().size()
    const oslam::KeyPoint* mvKeysUn;
    const uint8_t* has_mp;                // pMP && !pMP->isBad() of the keypoint's map point
    const float* Xw;                      // [N][3] pMP->GetWorldPos()
    const float* mvInvLevelSigma2;
    float Tcw[16];                        // GetRotation() / GetTranslation(), row-major 4 x 4
    float fx, fy, cx, cy;                 // mK
};
struct Sim3 {                             // g2o::Sim3 as rotation().toRotationMatrix() (row-major), translation(), scale()
    double R[9], t[3], s;
};

// Flat view of what Optimizer::OptimizeEssentialGraph reads of the map (src/Optimizer.cc:781-1044).  The keyframes are the good ones (!isBad()) in
// ascending mnId, re-indexed 0 .. nKF - 1; every list below names keyframes by that index and is a CSR pair: entries ptr[k] .. ptr[k + 1] - 1 belong to
// keyframe k.  The driver does not close loops: this is an operator for a caller that does.
struct EssentialGraphView {
    int nKF;
    float* Tcw;                              // [nKF][16] GetPose() in, SetPose() out
    const int32_t* parent;                   // [nKF] GetParent(), -1 without one
    const int32_t* children_ptr; const int32_t* children;       // what hasChild() answers true for
    const int32_t* loop_ptr; const int32_t* loop_edges;         // GetLoopEdges()
    const int32_t* covis_ptr; const int32_t* covisibles;        // GetCovisiblesByWeight(100), in its order, bad keyframes left out
    const int32_t* conn_ptr; const int32_t* conn; const int32_t* conn_weight;   // LoopConnections[pKF] (empty for a keyframe that is no key) and pKF->GetWeight of each
    const uint8_t* has_corrected; const Sim3* Corrected;        // [nKF] CorrectedSim3.find(pKF) != end(), and its value
    const uint8_t* has_noncorrected; const Sim3* NonCorrected;  // [nKF] NonCorrectedSim3
    int pLoopKF, pCurKF;
    int nMP;                                 // the map points that are not bad
    float* Xw;                               // [nMP][3] GetWorldPos() in, SetWorldPos() out
    const int32_t* ref;                      // [nMP] mnCorrectedByKF == pCurKF->mnId ? mnCorrectedReference : GetReferenceKeyFrame(), as an index; -1 skips the point
};

class Optimizer {
public:
    // int static OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2, const bool bFixScale)
    // (include/Optimizer.h:56, src/Optimizer.cc:1046-1241).  vpMatches1 [KF1.N] as SearchBySim3 leaves it: -1 = NULL, a value in [0, KF2.N) = the map point
    // of that keypoint of KF2 (its GetIndexInKeyFrame(pKF2)), anything else = a map point without an index in KF2 (skipped by :1114, the entry stays).
    // Entries the reference clears become -1.  g2oS12 is read as the floats LoopClosing builds gScm from (:326) and written when the reference writes it.
    static int OptimizeSim3(const Sim3OptKeyFrameView& KF1, const Sim3OptKeyFrameView& KF2, std::vector<int32_t>& vpMatches1, Sim3& g2oS12, float th2, bool bFixScale) {
        if ((int)vpMatches1.size() != KF1.N) throw std::runtime_error("OptimizeSim3: vpMatches1 must have one entry per keypoint of KF1");
        std::vector<float> X1, X2, o1, o2, i1, i2;
        std::vector<int> row;   // vnIndexEdge
        for (int i = 0; i < KF1.N; i++) {   // :1099-1137
            const int k2 = vpMatches1[i];
            if (k2 == -1) continue;
            if (k2 < 0 || k2 >= KF2.N) continue;                  // i2 < 0
            if (!KF1.has_mp[i] || !KF2.has_mp[k2]) continue;      // !pMP1 || pMP1->isBad() || pMP2->isBad()
            float P[3];
            to_camera(KF1.Tcw, KF1.Xw + (size_t)i * 3, P); X1.insert(X1.end(), P, P + 3);
            to_camera(KF2.Tcw, KF2.Xw + (size_t)k2 * 3, P); X2.insert(X2.end(), P, P + 3);
            o1.push_back(KF1.mvKeysUn[i].x); o1.push_back(KF1.mvKeysUn[i].y); i1.push_back(KF1.mvInvLevelSigma2[KF1.mvKeysUn[i].octave]);
            o2.push_back(KF2.mvKeysUn[k2].x); o2.push_back(KF2.mvKeysUn[k2].y); i2.push_back(KF2.mvInvLevelSigma2[KF2.mvKeysUn[k2].octave]);
            row.push_back(i);
        }
        const int n = (int)row.size();
        oslam_sim3_opt_problem_t pr;
        pr.count = n; pr.offset = 0;
        pr.fx1 = KF1.fx; pr.fy1 = KF1.fy; pr.cx1 = KF1.cx; pr.cy1 = KF1.cy; pr.fx2 = KF2.fx; pr.fy2 = KF2.fy; pr.cx2 = KF2.cx; pr.cy2 = KF2.cy;
        pr.s12 = (float)g2oS12.s;
        for (int k = 0; k < 9; k++) pr.R12[k] = (float)g2oS12.R[k];
        for (int k = 0; k < 3; k++) pr.t12[k] = (float)g2oS12.t[k];
        pr.th2 = th2; pr.fix_scale = bFixScale ? 1 : 0;
        double S[13];
        memcpy(S, g2oS12.R, sizeof(g2oS12.R)); memcpy(S + 9, g2oS12.t, sizeof(g2oS12.t)); S[12] = g2oS12.s;
        std::vector<uint8_t> inl((size_t)n + 1, 0);
        int32_t status[4] = {0, 0, 0, 0};
        oslam::throw_on(oslam_optimize_sim3_batch(sim3_opt_handle(n), 1, &pr, n, X1.data(), X2.data(), o1.data(), o2.data(), i1.data(), i2.data(), S, inl.data(), status, nullptr,
                                                  nullptr));
        for (int e = 0; e < n; e++)
            if (!inl[e]) vpMatches1[row[e]] = -1;
        if (status[0] < 0) return 0;   // (an input that is not finite: every entry is cleared, g2oS12 stays)
        memcpy(g2oS12.R, S, sizeof(g2oS12.R)); memcpy(g2oS12.t, S + 9, sizeof(g2oS12.t)); g2oS12.s = S[12];   // (S is unchanged where the reference returns early)
        return status[0];
    }
    // cv::Mat P3Dc = Rcw * P3Dw + tcw (:1118, :1126): the three float products summed in float from left to right, `+ t` in double, rounded once
    static void to_camera(const float T[16], const float X[3], float P[3]) {
        for (int r = 0; r < 3; r++) {
            const float p0 = T[4 * r] * X[0], p1 = T[4 * r + 1] * X[1], p2 = T[4 * r + 2] * X[2];
            const float s01 = p0 + p1;
            const float s = s01 + p2;
            P[r] = (float)((double)s + (double)T[4 * r + 3]);
        }
    }
    static oslam_sim3_opt_t* sim3_opt_handle(int n) {   // one handle per thread (the reference's static methods keep no state)
        static thread_local oslam_sim3_opt_t* h = nullptr;
        static thread_local int cap = 0;
        if (!h || n > cap) {
            oslam_sim3_opt_destroy(h);
            h = nullptr;
            cap = n < 2400 ? 2400 : n;
            oslam::throw_on(oslam_sim3_opt_create(&h, 1, cap, 0));
        }
        return h;
    }
    // The edges of OptimizeEssentialGraph (:847-983) as (i, j, kind) triples in the reference's order: i is setVertex(0), j setVertex(1), kind 0 a new loop
    // connection (measured between the corrected Sim3s), 1 a spanning-tree, old-loop or covisibility edge (non-corrected where present).  The reference walks
    // its std::map<KeyFrame*, ...> and std::set<KeyFrame*> in pointer order; here both run in ascending keyframe index.
    static std::vector<int32_t> EssentialGraphEdges(const EssentialGraphView& G) {
        const int minFeat = 100;
        std::vector<int32_t> out;
        std::set<std::pair<int32_t, int32_t>> sInsertedEdges;
        auto sorted = [](const int32_t* v, int a, int b) { return std::set<int32_t>(v + a, v + b); };
        for (int i = 0; i < G.nKF; i++) {   // :852-880
            std::map<int32_t, int32_t> w;
            for (int q = G.conn_ptr[i]; q < G.conn_ptr[i + 1]; q++) w[G.conn[q]] = G.conn_weight[q];
            for (const auto& c : w) {
                const int j = c.first;
                if ((i != G.pCurKF || j != G.pLoopKF) && c.second < minFeat) continue;
                out.insert(out.end(), {i, j, 0});
                sInsertedEdges.insert(std::make_pair(std::min(i, j), std::max(i, j)));
            }
        }
        for (int i = 0; i < G.nKF; i++) {   // :883-983
            const int p = G.parent[i];
            if (p >= 0) out.insert(out.end(), {i, p, 1});
            const std::set<int32_t> sLoopEdges = sorted(G.loop_edges, G.loop_ptr[i], G.loop_ptr[i + 1]);
            for (int l : sLoopEdges)
                if (l < i) out.insert(out.end(), {i, l, 1});
            const std::set<int32_t> ch = sorted(G.children, G.children_ptr[i], G.children_ptr[i + 1]);
            for (int q = G.covis_ptr[i]; q < G.covis_ptr[i + 1]; q++) {
                const int n = G.covisibles[q];
                if (n != p && !ch.count(n) && !sLoopEdges.count(n) && n < i) {
                    if (sInsertedEdges.count(std::make_pair(std::min(i, n), std::max(i, n)))) continue;
                    out.insert(out.end(), {i, n, 1});
                }
            }
        }
        return out;
    }
    // void static OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const KeyFrameAndPose& NonCorrectedSim3, const KeyFrameAndPose&
    // CorrectedSim3, const map<KeyFrame*, set<KeyFrame*>>& LoopConnections, const bool& bFixScale) (include/Optimizer.h, src/Optimizer.cc:781-1044): writes
    // G.Tcw (SetPose) and G.Xw (SetWorldPos); UpdateNormalAndDepth (:1042) stays with the caller (the map-point operator).  Throws on an invalid graph.
    static void OptimizeEssentialGraph(EssentialGraphView& G, bool bFixScale) {
        const int n = G.nKF;
        if (n <= 0) return;
        const std::vector<int32_t> edges = EssentialGraphEdges(G);
        const int E = (int)(edges.size() / 3);
        std::vector<float> Scw((size_t)n * 13), Snc((size_t)n * 13, 0.f);
        std::vector<uint8_t> fixed((size_t)n, 0);
        auto put = [](float* o, const Sim3& S) {
            o[0] = (float)S.s;
            for (int k = 0; k < 9; k++) o[1 + k] = (float)S.R[k];
            for (int k = 0; k < 3; k++) o[10 + k] = (float)S.t[k];
        };
        for (int k = 0; k < n; k++) {   // :809-844
            float* o = Scw.data() + (size_t)k * 13;
            if (G.has_corrected[k]) put(o, G.Corrected[k]);
            else {
                const float* T = G.Tcw + (size_t)k * 16;
                o[0] = 1.f;
                for (int r = 0; r < 3; r++) {
                    for (int c = 0; c < 3; c++) o[1 + 3 * r + c] = T[4 * r + c];
                    o[10 + r] = T[4 * r + 3];
                }
            }
            if (G.has_noncorrected[k]) put(Snc.data() + (size_t)k * 13, G.NonCorrected[k]);
            fixed[k] = k == G.pLoopKF ? 1 : 0;
        }
        oslam_essential_graph_problem_t pr;
        memset(&pr, 0, sizeof(pr));
        pr.n_kf = n; pr.n_edges = E; pr.fix_scale = bFixScale ? 1 : 0;
        std::vector<int32_t> row_first((size_t)n);
        int64_t blocks = 0;
        oslam::throw_on(oslam_essential_graph_envelope(1, &pr, n, fixed.data(), E, edges.data(), row_first.data(), &blocks));
        oslam_essential_graph_t* h = nullptr;
        oslam::throw_on(oslam_essential_graph_create(&h, 1, n, E > 0 ? E : 1, blocks > 0 ? blocks : 1, 0));
        std::vector<double> Sout((size_t)n * 13);
        std::vector<float> Tout((size_t)n * 16);
        int32_t status[4] = {0, 0, 0, 0};
        int rc = oslam_optimize_essential_graph_batch(h, 1, &pr, n, Scw.data(), Snc.data(), G.has_noncorrected, fixed.data(), E, edges.data(), Sout.data(), Tout.data(), status, nullptr,
                                                      nullptr);
        if (rc == OSLAM_OK && status[0] == 0 && G.nMP > 0) {
            std::vector<int32_t> pp((size_t)G.nMP, 0);
            std::vector<float> Xout(G.Xw, G.Xw + (size_t)G.nMP * 3);
            rc = oslam_essential_graph_correct_points(h, 1, &pr, n, Scw.data(), Sout.data(), status, G.nMP, pp.data(), G.ref, G.Xw, Xout.data());
            if (rc == OSLAM_OK) memcpy(G.Xw, Xout.data(), Xout.size() * sizeof(float));
        }
        oslam_essential_graph_destroy(h);
        oslam::throw_on(rc);
        if (status[0] != 0) throw std::runtime_error("OptimizeEssentialGraph: invalid graph (a value that is not finite, a scale that is not positive, or no loop keyframe)");
        memcpy(G.Tcw, Tout.data(), Tout.size() * sizeof(float));
    }
    // int static PoseOptimization(Frame* pFrame) (include/Optimizer.h:46)
    static int PoseOptimization(PoseFrameView& F) {
        std::vector<float> obs, inv;
        gather(F, obs, inv);
        const float K5[5] = {F.fx, F.fy, F.cx, F.cy, F.mbf};
        float Tout[16];
        int32_t n = 0;
        oslam::throw_on(oslam_pose_optimize(pose_handle(F.N), F.N, F.mTcw, F.Xw, obs.data(), inv.data(), F.has_mp, K5, Tout, F.mvbOutlier, &n, nullptr));
        memcpy(F.mTcw, Tout, sizeof(Tout));
        return n;
    }
    // void static LocalBundleAdjustment(KeyFrame* pKF, bool *pbStopFlag, Map* pMap) (include/Optimizer.h:45)
    static void LocalBundleAdjustment(BAGraph& g, bool* pbStopFlag = nullptr) {
        oslam_lba_t* h = lba_handle();
        volatile int32_t* flag = oslam_lba_stop_flag(h);
        *flag = (pbStopFlag && *pbStopFlag) ? 1 : 0;   // LocalMapping::InterruptBA sets the flag from another thread through StopFlag()
        const float K5[5] = {g.fx, g.fy, g.cx, g.cy, g.mbf};
        std::vector<float> po((size_t)g.nKF * 16), xo((size_t)g.nP * 3 + 3);
        oslam::throw_on(oslam_lba_optimize(h, g.nKF, g.poses, g.fixed, g.nP, g.points, g.nE, g.edge_kf, g.edge_pt, g.edge_obs, g.edge_invSigma2, K5, 1, po.data(),
                                           xo.data(), g.erase, nullptr));
        memcpy(g.poses, po.data(), po.size() * 4);
        if (g.nP) memcpy(g.points, xo.data(), (size_t)g.nP * 12);
    }
    static volatile int32_t* StopFlag() { return oslam_lba_stop_flag(lba_handle()); }
    // void static BundleAdjustment(const vector<KeyFrame*>&, const vector<MapPoint*>&, int nIterations, bool* pbStopFlag, const unsigned long nLoopKF, const bool bRobust)
    static void BundleAdjustment(BAGraph& g, int nIterations = 5, bool* pbStopFlag = nullptr, bool bRobust = true) {
        oslam_lba_t* h = lba_handle();
        *oslam_lba_stop_flag(h) = (pbStopFlag && *pbStopFlag) ? 1 : 0;
        const float K5[5] = {g.fx, g.fy, g.cx, g.cy, g.mbf};
        std::vector<float> po((size_t)g.nKF * 16), xo((size_t)g.nP * 3 + 3);
        oslam::throw_on(oslam_ba_optimize(h, g.nKF, g.poses, g.fixed, g.nP, g.points, g.nE, g.edge_kf, g.edge_pt, g.edge_obs, g.edge_invSigma2, K5, nIterations,
                                          bRobust ? 1 : 0, pbStopFlag ? 1 : 0, po.data(), xo.data()));
        memcpy(g.poses, po.data(), po.size() * 4);
        if (g.nP) memcpy(g.points, xo.data(), (size_t)g.nP * 12);
    }

    static void gather(const PoseFrameView& F, std::vector<float>& obs, std::vector<float>& inv) {
        obs.resize((size_t)F.N * 3 + 3); inv.resize(F.N + 1);
        for (int i = 0; i < F.N; i++) {
            obs[(size_t)i * 3] = F.mvKeysUn[i].x; obs[(size_t)i * 3 + 1] = F.mvKeysUn[i].y; obs[(size_t)i * 3 + 2] = F.mvuRight[i];
            inv[i] = F.mvInvLevelSigma2[F.mvKeysUn[i].octave];
        }
    }
    static oslam_poseopt_t* pose_handle(int N) {   // one handle per thread (the reference's static methods keep no state)
        static thread_local oslam_poseopt_t* h = nullptr;
        static thread_local int cap = 0;
        if (!h || N > cap) {
            oslam_poseopt_destroy(h);
            h = nullptr;
            cap = N < 2400 ? 2400 : N;
            oslam::throw_on(oslam_poseopt_create(&h, 1, cap, 0));
        }
        return h;
    }
    static oslam_lba_t* lba_handle() {
        static thread_local oslam_lba_t* h = nullptr;
        if (!h) oslam::throw_on(oslam_lba_create(&h, 1, 128, 4096, 32768, 0));
        return h;
    }
};

// Flat view of what LoopClosing::CorrectLoop's propagation touches (src/LoopClosing.cc:436-517).  The keyframes are mvpCurrentConnectedKFs in ascending mnId,
// re-indexed 0 .. nKF - 1; the points are those any of them observes.  The driver does not close loops: this is an operator for a caller that does.
struct LoopCorrectionView {
    int nKF, pCurKF;
    float* Tiw;                              // [nKF][16] GetPose() in, SetPose() out
    Sim3 Scw;                                // mg2oScw (ComputeScw)
    const int32_t* mp_ptr; const int32_t* mp;   // CSR: GetMapPointMatches() of keyframe k as indices into the points, -1 = NULL
    int nMP;
    float* Xw;                               // [nMP][3] GetWorldPos() in, SetWorldPos() out
    const uint8_t* bad;                      // [nMP] isBad()
    Sim3* Corrected; Sim3* NonCorrected;     // [nKF] out: CorrectedSim3, NonCorrectedSim3 (what OptimizeEssentialGraph takes)
    int32_t* mnCorrectedReference;           // [nMP] out: the keyframe that corrected the point (mnCorrectedByKF == pCurKF->mnId) or -1
};
// Flat view of the map update after global BA (src/LoopClosing.cc:677-738): every keyframe of the map in ascending mnId, every map point.
struct GlobalBAUpdateView {
    int nKF;
    const int32_t* parent;                   // [nKF] GetParent(), -1 for a member of mvpKeyFrameOrigins
    const uint8_t* kf_in_ba;                 // [nKF] mnBAGlobalForKF == nLoopKF
    float* Tcw;                              // [nKF][16] GetPose() in (mTcwBefGBA afterwards: keep a copy), SetPose() out
    const float* TcwGBA;                     // [nKF][16] mTcwGBA, read where kf_in_ba is set
    uint8_t* reached;                        // [nKF] out: the walk from the origins came by
    int nMP;
    float* Xw;                               // [nMP][3] GetWorldPos() in, SetWorldPos() out
    const float* PosGBA;                     // [nMP][3] mPosGBA, read where mp_in_ba is set
    const uint8_t* mp_in_ba; const uint8_t* bad;   // [nMP] mnBAGlobalForKF == nLoopKF, isBad()
    const int32_t* ref;                      // [nMP] GetReferenceKeyFrame() as an index
};

// The arithmetic of ORB_SLAM2::LoopClosing (include/LoopClosing.h) that is not one of the other classes' operators.  Static, as the state lives with the caller.
// LoopClosing itself (below KeyFrameDatabase, which its DetectLoop needs) derives from it: callers write LoopClosing::ComputeScw and so on.
class LoopClosingArithmetic {
public:
    // mg2oScw = gScm * gSmw and mScw = Converter::toCvMat(mg2oScw) (src/LoopClosing.cc:334-336); gScm as OptimizeSim3 returned it, Tmw = pKF->GetPose()
    static Sim3 ComputeScw(const Sim3& gScm, const float Tmw[16], float mScw[16]) {
        Sim3 out;
        static_assert(sizeof(Sim3) == 13 * sizeof(double), "Sim3 is the 13 doubles R, t, s of the ABI");
        oslam::throw_on(oslam_loop_compose_scw(handle(1, 1, 1), 1, gScm.R, Tmw, out.R, mScw));
        return out;
    }
    // :436-517: fills V.Corrected / V.NonCorrected / V.mnCorrectedReference, writes V.Xw (SetWorldPos) and V.Tiw (SetPose).  UpdateNormalAndDepth and
    // UpdateConnections stay with the caller.  Throws on an invalid problem.
    static void PropagateCorrection(LoopCorrectionView& V) {
        const int n = V.nKF, E = n > 0 ? V.mp_ptr[n] : 0;
        if (n <= 0) return;
        oslam_loop_correct_problem_t pr;
        memset(&pr, 0, sizeof(pr));
        pr.n_kf = n; pr.cur = V.pCurKF; pr.n_points = V.nMP; pr.n_entries = E;
        std::vector<int32_t> kfe((size_t)n * 2), cref((size_t)V.nMP + 1, -1);
        for (int k = 0; k < n; k++) { kfe[2 * (size_t)k] = V.mp_ptr[k]; kfe[2 * (size_t)k + 1] = V.mp_ptr[k + 1] - V.mp_ptr[k]; }
        std::vector<double> Sc((size_t)n * 13), Sn((size_t)n * 13);
        std::vector<float> Tout((size_t)n * 16), Xout(V.Xw, V.Xw + (size_t)V.nMP * 3);
        Xout.resize((size_t)V.nMP * 3 + 3);
        int32_t status[4] = {0, 0, 0, 0};
        oslam::throw_on(oslam_loop_propagate(handle(n, E, V.nMP), 1, &pr, n, V.Tiw, V.Scw.R, kfe.data(), E, V.mp, V.nMP, V.Xw, V.bad, Sc.data(), Sn.data(), Tout.data(),
                                             Xout.data(), cref.data(), status));
        if (status[0] != 0) throw std::runtime_error("PropagateCorrection: invalid problem (a value that is not finite, a scale that is not positive, or an index outside its table)");
        memcpy(V.Tiw, Tout.data(), Tout.size() * sizeof(float));
        if (V.nMP) { memcpy(V.Xw, Xout.data(), (size_t)V.nMP * 3 * sizeof(float)); memcpy(V.mnCorrectedReference, cref.data(), (size_t)V.nMP * sizeof(int32_t)); }
        memcpy(V.Corrected, Sc.data(), Sc.size() * sizeof(double));
        memcpy(V.NonCorrected, Sn.data(), Sn.size() * sizeof(double));
    }
    // :677-738: writes V.Tcw (SetPose), V.reached and V.Xw (SetWorldPos).  Throws on an invalid map (a parent outside the map, a cycle, a root outside the BA).
    static void UpdateMapAfterGlobalBA(GlobalBAUpdateView& V) {
        const int n = V.nKF;
        if (n <= 0) return;
        oslam_loop_gba_problem_t pr;
        memset(&pr, 0, sizeof(pr));
        pr.n_kf = n; pr.n_points = V.nMP;
        std::vector<float> Tout((size_t)n * 16), Xout(V.Xw, V.Xw + (size_t)V.nMP * 3);
        Xout.resize((size_t)V.nMP * 3 + 3);
        int32_t status[4] = {0, 0, 0, 0};
        oslam::throw_on(oslam_loop_update_after_gba(handle(n, 1, V.nMP), 1, &pr, n, V.parent, V.kf_in_ba, V.Tcw, V.TcwGBA, V.nMP, V.Xw, V.PosGBA, V.mp_in_ba, V.bad, V.ref,
                                                    Tout.data(), V.reached, Xout.data(), status));
        if (status[0] != 0) throw std::runtime_error("UpdateMapAfterGlobalBA: invalid map (a parent outside the map, a cycle, a root outside the BA or a value that is not finite)");
        memcpy(V.Tcw, Tout.data(), Tout.size() * sizeof(float));
        if (V.nMP) memcpy(V.Xw, Xout.data(), (size_t)V.nMP * 3 * sizeof(float));
    }

private:
    static oslam_loop_correct_t* handle(int nKF, int nEntries, int nMP) {   // one handle per thread, grown on demand
        static thread_local oslam_loop_correct_t* h = nullptr;
        static thread_local int capK = 0, capE = 0, capP = 0;
        if (!h || nKF > capK || nEntries > capE || nMP > capP) {
            oslam_loop_correct_destroy(h);
            h = nullptr;
            capK = nKF > capK ? nKF : capK; capE = nEntries > capE ? nEntries : capE; capP = nMP > capP ? nMP : capP;
            if (capK < 256) capK = 256;
            if (capE < 65536) capE = 65536;
            if (capP < 65536) capP = 65536;
            oslam::throw_on(oslam_loop_correct_create(&h, 1, capK, capE, capP, 0));
        }
        return h;
    }
};

class ObjectOptimizer {
public:
    // static int PoseOptimization2(Frame* pFrame) (include/ObjectOptimizer.h:23); *nSemNum receives what the reference adds to N_AllSemanticConstraintNum
    static int PoseOptimization2(PoseFrameView& F, const SemanticView& S, int* nSemNum = nullptr) {
        std::vector<float> obs, inv, kp_uv((size_t)F.N * 2 + 2);
        Optimizer::gather(F, obs, inv);
        for (int i = 0; i < F.N; i++) { kp_uv[(size_t)i * 2] = F.mvKeysUn[i].x; kp_uv[(size_t)i * 2 + 1] = F.mvKeysUn[i].y; }
        oslam_semantic_t sem;
        sem.nObj = S.nObj; sem.H = S.H; sem.W = S.W; sem.masks = S.masks; sem.nObjMp = S.nObjMp; sem.objmp_Xw = S.objmp_Xw; sem.objmp_obj = S.objmp_obj;
        sem.nJoint = S.nJoint; sem.joint_kp = S.joint_kp; sem.joint_obj = S.joint_obj; sem.kp_uv = kp_uv.data();
        sem.bounds[0] = S.mnMinX; sem.bounds[1] = S.mnMinY; sem.bounds[2] = S.mnMaxX; sem.bounds[3] = S.mnMaxY; sem.invSigma2_0 = F.mvInvLevelSigma2[0];
        const float K5[5] = {F.fx, F.fy, F.cx, F.cy, F.mbf};
        float Tout[16];
        int32_t n = 0, ns = 0;
        oslam::throw_on(oslam_pose_optimize2(Optimizer::pose_handle(F.N), F.N, F.mTcw, F.Xw, obs.data(), inv.data(), F.has_mp, K5, &sem, Tout, F.mvbOutlier, &n, &ns));
        memcpy(F.mTcw, Tout, sizeof(Tout));
        if (nSemNum) *nSemNum = ns;
        return n;
    }
};

// Flat views of what PnPsolver::PnPsolver(const Frame&, const vector<MapPoint*>&) reads (src/PnPsolver.cc:67-110)
struct PnPFrameView {
    int N;                                // mvKeysUn.size()
    const oslam::KeyPoint* mvKeysUn;
    const float* mvLevelSigma2; int nLevels;
    float fx, fy, cx, cy;
};
struct PnPMatchView {                     // vpMapPointMatches, one entry per keypoint
    const uint8_t* has_mp;                // vpMapPointMatches[i] != NULL
    const uint8_t* bad;                   // pMP->isBad() (may be NULL: none is bad)
    const float* Xw;                      // [N][3] pMP->GetWorldPos()
};

// ORB_SLAM2::PnPsolver (include/PnPsolver.h:62-72).  The reference returns the pose as a cv::Mat that is empty when there is none; here iterate / find
// return whether there is one and write it to Tcw (4 x 4 row-major float).  A solver is one shot (oslam_hip.h, "PnP solver"): the first iterate() runs the
// reference's whole interleaved loop, whatever nIterations says; later calls have nothing left to do and return no pose with bNoMore.
// `seed` stands for the clock-seeded DUtils::Random of the reference.
class PnPsolver {
public:
    PnPsolver(const PnPFrameView& F, const PnPMatchView& M, uint32_t seed = 0) : nKeys_(F.N), seed_(seed) {
        K_[0] = F.fx; K_[1] = F.fy; K_[2] = F.cx; K_[3] = F.cy;
        for (int i = 0; i < F.N; i++) {   // :78-101
            if (!M.has_mp[i] || (M.bad && M.bad[i])) continue;
            const oslam::KeyPoint& kp = F.mvKeysUn[i];
#ifdef OSLAM_ADAPTER_USE_OPENCV
            mvP2D.push_back(kp.pt.x); mvP2D.push_back(kp.pt.y);
#else
            mvP2D.push_back(kp.x); mvP2D.push_back(kp.y);
#endif
            if (kp.octave < 0 || kp.octave >= F.nLevels) throw std::runtime_error("PnPsolver: keypoint octave outside mvLevelSigma2");
            mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);
            mvP3Dw.push_back(M.Xw[3 * (size_t)i]); mvP3Dw.push_back(M.Xw[3 * (size_t)i + 1]); mvP3Dw.push_back(M.Xw[3 * (size_t)i + 2]);
            mvKeyPointIndices.push_back(i);
        }
        SetRansacParameters();
    }
    ~PnPsolver() { oslam_pnp_destroy(h_); }
    PnPsolver(const PnPsolver&) = delete;
    PnPsolver& operator=(const PnPsolver&) = delete;

    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4f, float th2 = 5.991f) {
        prm_.probability = probability; prm_.min_inliers = minInliers; prm_.max_iterations = maxIterations; prm_.min_set = minSet; prm_.epsilon = epsilon; prm_.th2 = th2;
        prm_.reserved = 0;
    }
    // mRansacMinInliers, mRansacEpsilon, mRansacMaxIts as SetRansacParameters leaves them (:134-152)
    oslam_pnp_ransac_t Adjusted() const {
        oslam_pnp_ransac_t r;
        oslam::throw_on(oslam_pnp_ransac_params((int)mvSigma2.size(), prm_.probability, prm_.min_inliers, prm_.max_iterations, prm_.min_set, prm_.epsilon, &r));
        return r;
    }
    bool find(std::vector<bool>& vbInliers, int& nInliers, float Tcw[16]) {
        bool bFlag;
        return iterate(prm_.max_iterations, bFlag, vbInliers, nInliers, Tcw);
    }
    // vbInliers is indexed by keypoint (:229-234) and empty when there is no pose
    bool iterate(int /*nIterations*/, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, float Tcw[16]) {
        bNoMore = false;
        vbInliers.clear();
        nInliers = 0;
        const int N = (int)mvSigma2.size();
        if (done_ || N == 0) { bNoMore = true; done_ = true; return false; }
        done_ = true;
        if (!h_) oslam::throw_on(oslam_pnp_create(&h_, 1, N, prm_.max_iterations));
        oslam_pnp_problem_t pr;
        pr.count = N; pr.offset = 0; pr.fx = K_[0]; pr.fy = K_[1]; pr.cx = K_[2]; pr.cy = K_[3]; pr.seed = seed_; pr.reserved = 0;
        std::vector<uint8_t> flags(N, 0);
        int32_t st[4] = {0, 0, 0, -1};
        oslam::throw_on(oslam_pnp_ransac_batch(h_, 1, &pr, N, mvP3Dw.data(), mvP2D.data(), mvSigma2.data(), &prm_, nullptr, Tcw, flags.data(), st, nullptr));
        mnIterations = st[2];
        if (st[0] != 1) bNoMore = true;   // :241-243
        if (st[0] <= 0) return false;
        nInliers = st[1];
        vbInliers.assign(nKeys_, false);
        for (int i = 0; i < N; i++)
            if (flags[i]) vbInliers[mvKeyPointIndices[i]] = true;
        return true;
    }
    int mnIterations = 0;                       // iterations run by the last iterate()
    std::vector<float> mvP2D, mvSigma2, mvP3Dw;   // the filtered correspondences (:87-93), packed
    std::vector<size_t> mvKeyPointIndices;

private:
    int nKeys_;
    uint32_t seed_;
    float K_[4];
    oslam_pnp_params_t prm_;
    oslam_pnp_t* h_ = nullptr;
    bool done_ = false;
};

// Flat views of what Sim3Solver::Sim3Solver(KeyFrame*, KeyFrame*, const vector<MapPoint*>&, bool) reads (src/Sim3Solver.cc:37-112)
struct Sim3KeyFrameView {
    int N;                                // mvKeysUn.size()
    const oslam::KeyPoint* mvKeysUn;
    const float* mvLevelSigma2; int nLevels;
    float fx, fy, cx, cy;                 // mK
    float Rcw[9], tcw[3];                 // GetRotation() (row-major), GetTranslation()
};
struct Sim3MatchView {                    // one entry per keypoint of KF1 (mN1 = vpMatched12.size())
    int N1;
    const uint8_t* matched;               // vpMatched12[i1] != NULL
    const uint8_t* has_mp1;               // pKF1->GetMapPointMatches()[i1] != NULL (may be NULL: every keypoint has one)
    const uint8_t* bad1; const uint8_t* bad2;   // pMP1->isBad(), pMP2->isBad() (may be NULL: none is bad)
    const int32_t* indexKF1; const int32_t* indexKF2;   // pMP1->GetIndexInKeyFrame(pKF1), pMP2->GetIndexInKeyFrame(pKF2)
    const float* Xw1; const float* Xw2;   // [N1][3] GetWorldPos() of both points
};

// ORB_SLAM2::Sim3Solver (include/Sim3Solver.h:38-62).  The reference returns the transform as a cv::Mat that is empty when there is none; here iterate /
// find return whether there is one and write it to T12 (4 x 4 row-major float).  The class keeps the state record of the operator (oslam_hip.h, "Sim3
// solver"), so repeated calls resume as the reference's do.  `seed` stands for the clock-seeded DUtils::Random of the reference.
class Sim3Solver {
public:
    Sim3Solver(const Sim3KeyFrameView& KF1, const Sim3KeyFrameView& KF2, const Sim3MatchView& M, bool bFixScale = true, uint32_t seed = 0) : mN1(M.N1), seed_(seed), fix_(bFixScale) {
        K_[0] = KF1.fx; K_[1] = KF1.fy; K_[2] = KF1.cx; K_[3] = KF1.cy; K_[4] = KF2.fx; K_[5] = KF2.fy; K_[6] = KF2.cx; K_[7] = KF2.cy;
        for (int i1 = 0; i1 < mN1; i1++) {   // :62-103
            if (!M.matched[i1]) continue;
            if (M.has_mp1 && !M.has_mp1[i1]) continue;
            if ((M.bad1 && M.bad1[i1]) || (M.bad2 && M.bad2[i1])) continue;
            const int indexKF1 = M.indexKF1[i1], indexKF2 = M.indexKF2[i1];
            if (indexKF1 < 0 || indexKF2 < 0) continue;
            if (indexKF1 >= KF1.N || indexKF2 >= KF2.N) throw std::runtime_error("Sim3Solver: keypoint index outside mvKeysUn");
            const int o1 = KF1.mvKeysUn[indexKF1].octave, o2 = KF2.mvKeysUn[indexKF2].octave;
            if (o1 < 0 || o1 >= KF1.nLevels || o2 < 0 || o2 >= KF2.nLevels) throw std::runtime_error("Sim3Solver: keypoint octave outside mvLevelSigma2");
            mvSigma2_1.push_back(KF1.mvLevelSigma2[o1]);
            mvSigma2_2.push_back(KF2.mvLevelSigma2[o2]);
            mvnIndices1.push_back((size_t)i1);
            to_camera(KF1, M.Xw1 + 3 * (size_t)i1, mvX3Dc1);   // Rcw1 * X3D1w + tcw1 (:94-98)
            to_camera(KF2, M.Xw2 + 3 * (size_t)i1, mvX3Dc2);
        }
        SetRansacParameters();
        reset_state();
    }
    ~Sim3Solver() { oslam_sim3_destroy(h_); }
    Sim3Solver(const Sim3Solver&) = delete;
    Sim3Solver& operator=(const Sim3Solver&) = delete;

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        if (h_ && maxIterations > prm_.max_iterations) { oslam_sim3_destroy(h_); h_ = nullptr; }   // (the handle's arena is sized by maxIterations)
        prm_.probability = probability; prm_.min_inliers = minInliers; prm_.max_iterations = maxIterations;
        st_.iterations_done = 0;   // mnIterations = 0 (:137); mnBestInliers and the best transform stay
    }
    // mRansacMaxIts as SetRansacParameters leaves it (:135), and whether iterate() gives up at once
    oslam_sim3_ransac_t Adjusted() const {
        oslam_sim3_ransac_t r;
        oslam::throw_on(oslam_sim3_ransac_params((int)mvSigma2_1.size(), prm_.probability, prm_.min_inliers, prm_.max_iterations, &r));
        return r;
    }
    bool find(std::vector<bool>& vbInliers12, int& nInliers, float T12[16]) {
        bool bFlag;
        return iterate(Adjusted().iterations, bFlag, vbInliers12, nInliers, T12);
    }
    // vbInliers has mN1 entries and is indexed by keypoint of KF1 (:143, :195-197)
    bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, float T12[16]) {
        bNoMore = false;
        vbInliers.assign((size_t)mN1, false);
        nInliers = 0;
        const int N = (int)mvSigma2_1.size();
        if (N == 0) { bNoMore = true; return false; }   // (N < mRansacMinInliers, or nothing to draw from)
        if (!h_) oslam::throw_on(oslam_sim3_create(&h_, 1, N, prm_.max_iterations));
        oslam_sim3_problem_t pr;
        pr.count = N; pr.offset = 0; pr.fx1 = K_[0]; pr.fy1 = K_[1]; pr.cx1 = K_[2]; pr.cy1 = K_[3]; pr.fx2 = K_[4]; pr.fy2 = K_[5]; pr.cx2 = K_[6]; pr.cy2 = K_[7];
        pr.seed = seed_; pr.fix_scale = fix_ ? 1 : 0;
        std::vector<uint8_t> flags((size_t)N, 0);
        int32_t st[4] = {0, 0, 0, 0};
        oslam::throw_on(oslam_sim3_iterate_batch(h_, 1, &pr, &st_, N, mvX3Dc1.data(), mvX3Dc2.data(), mvSigma2_1.data(), mvSigma2_2.data(), &prm_, nIterations < 0 ? 0 : nIterations,
                                                 nullptr, T12, flags.data(), st, nullptr, nullptr));
        bNoMore = st[3] != 0;
        if (st[0] != 1) return false;
        nInliers = st[1];
        for (int i = 0; i < N; i++)
            if (flags[i]) vbInliers[mvnIndices1[i]] = true;
        return true;
    }
    // GetEstimatedRotation (3 x 3 row-major) / Translation / Scale of the best hypothesis so far (:367-380)
    void GetEstimatedRotation(float R[9]) const { memcpy(R, st_.R, sizeof(st_.R)); }
    void GetEstimatedTranslation(float t[3]) const { memcpy(t, st_.t, sizeof(st_.t)); }
    float GetEstimatedScale() const { return st_.s; }
    int mnIterations() const { return st_.iterations_done; }
    int mnBestInliers() const { return st_.best_inliers; }

    int mN1;
    std::vector<float> mvX3Dc1, mvX3Dc2, mvSigma2_1, mvSigma2_2;   // the filtered correspondences (:84-98), packed
    std::vector<size_t> mvnIndices1;

private:
    static void to_camera(const Sim3KeyFrameView& KF, const float* Xw, std::vector<float>& out) {   // float, sums from left to right
        for (int i = 0; i < 3; i++) out.push_back(((KF.Rcw[3 * i] * Xw[0] + KF.Rcw[3 * i + 1] * Xw[1]) + KF.Rcw[3 * i + 2] * Xw[2]) + KF.tcw[i]);
    }
    void reset_state() { memset(&st_, 0, sizeof(st_)); st_.best_iteration = -1; }
    uint32_t seed_;
    bool fix_;
    float K_[8];
    oslam_sim3_params_t prm_;
    oslam_sim3_state_t st_;
    oslam_sim3_t* h_ = nullptr;
};

// Flat view of what Initializer reads of a Frame: mvKeysUn and mK (src/Initializer.cc:34-38, :49)
struct InitFrameView {
    int N;                                // mvKeysUn.size()
    const oslam::KeyPoint* mvKeysUn;
    float fx, fy, cx, cy;
};
#ifdef OSLAM_ADAPTER_USE_OPENCV
typedef cv::Point3f Point3f;
#else
struct Point3f { float x, y, z; };
#endif

// ORB_SLAM2::Initializer (include/Initializer.h:38-46) over oslam_init_* (oslam_hip.h, "Initializer").  R21 (3 x 3 row-major) and t21 are float arrays where
// the reference has cv::Mat; they, vP3D and vbTriangulated are written only when Initialize returns true.  `seed` stands for DUtils::Random, which the
// reference seeds with 0 (src/Initializer.cc:80).
class Initializer {
public:
    Initializer(const InitFrameView& ReferenceFrame, float sigma = 1.0, int iterations = 200, uint32_t seed = 0) : mSigma(sigma), mMaxIterations(iterations), seed_(seed) {
        K_[0] = ReferenceFrame.fx; K_[1] = ReferenceFrame.fy; K_[2] = ReferenceFrame.cx; K_[3] = ReferenceFrame.cy;
        keys1_ = pack(ReferenceFrame);
    }
    ~Initializer() { oslam_init_destroy(h_); }
    Initializer(const Initializer&) = delete;
    Initializer& operator=(const Initializer&) = delete;

    // Computes in parallel a fundamental matrix and a homography, selects a model and tries to recover the motion and the structure from motion
    bool Initialize(const InitFrameView& CurrentFrame, const std::vector<int>& vMatches12, float R21[9], float t21[3], std::vector<Point3f>& vP3D,
                    std::vector<bool>& vbTriangulated) {
        const int n1 = (int)(keys1_.size() / 2);
        if ((int)vMatches12.size() != n1) throw std::runtime_error("Initializer: vMatches12 must have one entry per key of the reference frame");
        const std::vector<float> keys2 = pack(CurrentFrame);
        const int n2 = CurrentFrame.N, cap = std::max(1, std::max(n1, n2));
        if (!h_ || cap > cap_) {
            oslam_init_destroy(h_);
            h_ = nullptr;
            oslam::throw_on(oslam_init_create(&h_, 1, cap, mMaxIterations));
            cap_ = cap;
        }
        oslam_init_problem_t pr;
        pr.n1 = n1; pr.off1 = 0; pr.n2 = n2; pr.off2 = 0; pr.fx = K_[0]; pr.fy = K_[1]; pr.cx = K_[2]; pr.cy = K_[3]; pr.sigma = mSigma; pr.seed = seed_;
        pr.reserved[0] = 0; pr.reserved[1] = 0;
        oslam_init_params_t prm;
        prm.max_iterations = mMaxIterations; prm.min_parallax = 1.0f; prm.min_triangulated = 50; prm.reserved = 0;   // (src/Initializer.cc:116-118)
        std::vector<int32_t> m12(vMatches12.begin(), vMatches12.end());
        std::vector<float> P3D(3 * (size_t)n1, 0.f);
        std::vector<uint8_t> tri(n1, 0);
        float R[9], t[3];
        oslam::throw_on(oslam_init_initialize_batch(h_, 1, &pr, n1, keys1_.data(), m12.data(), n2, keys2.data(), &prm, nullptr, R, t, P3D.data(), tri.data(), status, scores,
                                                    nullptr, nullptr, nullptr, nullptr));
        if (status[0] != 1) return false;
        for (int k = 0; k < 9; k++) R21[k] = R[k];
        for (int k = 0; k < 3; k++) t21[k] = t[k];
        vP3D.resize(n1);
        vbTriangulated.assign(n1, false);
        for (int i = 0; i < n1; i++) {
            vP3D[i].x = P3D[3 * (size_t)i]; vP3D[i].y = P3D[3 * (size_t)i + 1]; vP3D[i].z = P3D[3 * (size_t)i + 2];
            vbTriangulated[i] = tri[i] != 0;
        }
        return true;
    }
    int32_t status[8] = {0, 0, 0, 0, -1, -1, -1, 0};   // of the last Initialize: returned, model, N, nGood, motion, best H / F iteration, nsimilar / secondBestGood
    float scores[4] = {0, 0, 0, 0};                    // SH, SF, RH, parallax

private:
    static std::vector<float> pack(const InitFrameView& F) {
        std::vector<float> k(2 * (size_t)F.N);
        for (int i = 0; i < F.N; i++) {
#ifdef OSLAM_ADAPTER_USE_OPENCV
            k[2 * (size_t)i] = F.mvKeysUn[i].pt.x; k[2 * (size_t)i + 1] = F.mvKeysUn[i].pt.y;
#else
            k[2 * (size_t)i] = F.mvKeysUn[i].x; k[2 * (size_t)i + 1] = F.mvKeysUn[i].y;
#endif
        }
        return k;
    }
    float mSigma;
    int mMaxIterations;
    uint32_t seed_;
    float K_[4];
    std::vector<float> keys1_;
    oslam_init_t* h_ = nullptr;
    int cap_ = 0;
};

// Flat view of what KeyFrameDatabase reads of a KeyFrame: its id (the slot of the database on the device), its BowVector and, for the queries, the lists the
// reference asks the keyframe for.
struct KeyFrameDatabaseKeyFrameView {
    int mnId;
    const DBoW2::BowVector* mBowVec;
    std::vector<int32_t> vpBestCovisibles;   // GetBestCovisibilityKeyFrames(10), ids; read by add and by UpdateCovisibility
    std::vector<int32_t> spConnected;        // GetConnectedKeyFrames(), ids; read by DetectLoopCandidates
};

// ORB_SLAM2::KeyFrameDatabase (include/KeyFrameDatabase.h:41-71, src/KeyFrameDatabase.cc) for ONE database, over the oslam_kfdb_* functions of oslam_hip.h
// (see there for the restated semantics and the reloc_score normalisation).  The database lives on the device; keyframes are named by mnId, which must stay
// below maxKeyFrames.  The queries return ids where the reference returns KeyFrame pointers.
class KeyFrameDatabase {
public:
    // KeyFrameDatabase(const ORBVocabulary &voc); poolWords 0: room for every keyframe at maxWords
    explicit KeyFrameDatabase(const ORBVocabulary& voc, int maxKeyFrames = OSLAM_KFDB_MAX_KEYFRAMES, int maxWords = OSLAM_KFDB_MAX_WORDS, long long poolWords = 0) : mpVoc(&voc) {
        if (poolWords <= 0) poolWords = (long long)maxKeyFrames * ((maxWords + OSLAM_KFDB_CHUNK - 1) / OSLAM_KFDB_CHUNK) * OSLAM_KFDB_CHUNK;
        oslam::throw_on(oslam_kfdb_create(&h_, 1, maxKeyFrames, maxWords, poolWords, 0));
        cand_.resize(maxKeyFrames); acc_.resize(maxKeyFrames);
    }
    ~KeyFrameDatabase() { oslam_kfdb_destroy(h_); }
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

    // void add(KeyFrame* pKF)
    void add(const KeyFrameDatabaseKeyFrameView& KF) {
        flatten(*KF.mBowVec);
        const oslam_kfdb_add_t rec = {0, KF.mnId, 0, (int32_t)ids_.size()};
        oslam::throw_on(oslam_kfdb_add(h_, 1, &rec, (int)ids_.size(), ids_.data(), vals_.data()));
        UpdateCovisibility(KF);
    }
    // What the device keeps of KeyFrame::GetBestCovisibilityKeyFrames(10): call it when the keyframe's connections have changed (KeyFrame::UpdateConnections)
    void UpdateCovisibility(const KeyFrameDatabaseKeyFrameView& KF) {
        oslam_kfdb_covis_t rec = {0, KF.mnId, (int32_t)std::min<size_t>(KF.vpBestCovisibles.size(), OSLAM_KFDB_COVIS), {0}};
        for (int i = 0; i < OSLAM_KFDB_COVIS; i++) rec.ids[i] = i < rec.n ? KF.vpBestCovisibles[i] : -1;
        oslam::throw_on(oslam_kfdb_set_covisibility(h_, 1, &rec));
    }
    // void erase(KeyFrame* pKF)
    void erase(const KeyFrameDatabaseKeyFrameView& KF) {
        const oslam_kfdb_key_t rec = {0, KF.mnId};
        oslam::throw_on(oslam_kfdb_erase(h_, 1, &rec));
    }
    void clear() {
        const int32_t d = 0;
        oslam::throw_on(oslam_kfdb_clear(h_, 1, &d));
    }
    // std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore); connScores, if given, receives the score of pKF against every connected
    // keyframe that is in the database (-1 for the others): what DetectLoop computes minScore from
    std::vector<int32_t> DetectLoopCandidates(const KeyFrameDatabaseKeyFrameView& KF, float minScore, std::vector<float>* connScores = nullptr) {
        flatten(*KF.mBowVec);
        const oslam_kfdb_query_t q = {0, KF.mnId, 0, (int32_t)ids_.size(), 0, (int32_t)KF.spConnected.size(), minScore, 0};
        std::vector<float> cs(KF.spConnected.size());
        int32_t n = 0;
        oslam::throw_on(oslam_kfdb_detect_loop_candidates(h_, mpVoc->handle(), 1, &q, (int)ids_.size(), ids_.data(), vals_.data(), (int)KF.spConnected.size(),
                                                          KF.spConnected.data(), cand_.data(), acc_.data(), &n, diag_, cs.data()));
        if (connScores) *connScores = cs;
        return std::vector<int32_t>(cand_.begin(), cand_.begin() + n);
    }
    // std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F)
    std::vector<int32_t> DetectRelocalizationCandidates(int mnId, const DBoW2::BowVector& mBowVec) {
        flatten(mBowVec);
        const oslam_kfdb_query_t q = {0, mnId, 0, (int32_t)ids_.size(), 0, 0, 0.0f, 0};
        int32_t n = 0;
        oslam::throw_on(oslam_kfdb_detect_relocalization_candidates(h_, mpVoc->handle(), 1, &q, (int)ids_.size(), ids_.data(), vals_.data(), cand_.data(), acc_.data(), &n, diag_));
        return std::vector<int32_t>(cand_.begin(), cand_.begin() + n);
    }
    const float* accumulatedScores() const { return acc_.data(); }   // of the candidates the last query returned, in their order
    const int32_t* diagnostics() const { return diag_; }            // lKFsSharingWords.size(), maxCommonWords, minCommonWords, nscores, lScoreAndMatch.size()
    oslam_kfdb_t* handle() const { return h_; }                      // for LoopClosing below, which detects over this database
    const ORBVocabulary* vocabulary() const { return mpVoc; }
    int maxKeyFrames() const { return (int)cand_.size(); }

private:
    void flatten(const DBoW2::BowVector& v) {
        ids_.clear(); vals_.clear();
        for (const auto& e : v) { ids_.push_back(e.first); vals_.push_back(e.second); }   // (std::map order = word id ascending)
    }
    const ORBVocabulary* mpVoc;
    oslam_kfdb_t* h_ = nullptr;
    std::vector<uint32_t> ids_;
    std::vector<double> vals_;
    std::vector<int32_t> cand_;
    std::vector<float> acc_;
    int32_t diag_[5] = {0, 0, 0, 0, 0};
};

// ORB_SLAM2::KeyFrame's covisibility members (include/KeyFrame.h: AddConnection, EraseConnection, UpdateConnections, GetConnectedKeyFrames,
// GetVectorCovisibleKeyFrames, GetBestCovisibilityKeyFrames, GetCovisiblesByWeight, GetWeight, ChangeParent, GetParent), MapPoint's observation list
// (include/MapPoint.h: AddObservation, EraseObservation, SetBadFlag) and Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1496-1604) for ONE sequence: one
// graph of a covisibility handle of oslam_hip.h ("Covisibility graph": the restated semantics and its three normalisations).  Keyframes and points are ids
// where the reference has pointers; the graph lives on the device.  Bookkeeping calls are queued and sent, in order, before the next call that reads.
class KeyFrameGraph {
public:
    // a graph of its own: one handle with one graph
    KeyFrameGraph(int maxKeyFrames, int maxPoints, int obsCap = 16) : K_(maxKeyFrames), graph_(0), own_(true), overflow_(1) {
        oslam::throw_on(oslam_covis_create(&h_, 1, maxKeyFrames, maxPoints, obsCap, 0));
    }
    // graph `graph` of a handle of nGraphs graphs and maxKeyFrames keyframes that the caller keeps alive
    KeyFrameGraph(oslam_covis_t* h, int nGraphs, int graph, int maxKeyFrames) : h_(h), K_(maxKeyFrames), graph_(graph), own_(false), overflow_(nGraphs) {}
    ~KeyFrameGraph() { if (own_) oslam_covis_destroy(h_); }
    KeyFrameGraph(const KeyFrameGraph&) = delete;
    KeyFrameGraph& operator=(const KeyFrameGraph&) = delete;

    // void MapPoint::AddObservation(KeyFrame* pKF, size_t idx)
    void AddObservation(int pMP, int pKF, int idx) { push(OSLAM_COVIS_EV_OBS_ADD, pMP, pKF, idx); }
    // void MapPoint::EraseObservation(KeyFrame* pKF): the caller decides on nObs <= 2 and then calls SetBadFlag
    void EraseObservation(int pMP, int pKF) { push(OSLAM_COVIS_EV_OBS_ERASE, pMP, pKF, 0); }
    // void MapPoint::SetBadFlag()
    void SetBadFlag(int pMP) { push(OSLAM_COVIS_EV_POINT_BAD, pMP, 0, 0); }
    // void KeyFrame::AddConnection(KeyFrame* pKF, const int &weight) / EraseConnection(KeyFrame* pKF) / ChangeParent(KeyFrame* pKF); mbBad = true of a keyframe
    void AddConnection(int kf, int other, int weight) { push(OSLAM_COVIS_EV_CONN_ADD, kf, other, weight); }
    void EraseConnection(int kf, int other) { push(OSLAM_COVIS_EV_CONN_ERASE, kf, other, 0); }
    void ChangeParent(int kf, int parent) { push(OSLAM_COVIS_EV_PARENT_SET, kf, parent, 0); }
    void SetKeyFrameBad(int kf) { push(OSLAM_COVIS_EV_KF_BAD, kf, 0, 0); }
    // sends what is queued; throws when an observation list was full (normalisation 3)
    void Flush() {
        if (events_.empty()) return;
        const int rc = oslam_covis_apply(h_, (int)events_.size(), events_.data(), overflow_.data());
        events_.clear();
        oslam::throw_on(rc);
        if (overflow_[graph_] > 0) throw std::runtime_error("KeyFrameGraph: an observation list is full");
    }

    // void KeyFrame::UpdateConnections() of keyframe kf over vpMapPoints = its mvpMapPoints as point ids (-1 = NULL).  Returns false when the counter was
    // empty ("This should not happen", :323); mvNewLinks receives the keys of the row afterwards minus the ordered list before minus exclude.
    bool UpdateConnections(int kf, const std::vector<int32_t>& vpMapPoints, const std::vector<int32_t>& exclude = std::vector<int32_t>()) {
        std::vector<std::vector<int32_t> > links;
        const std::vector<int32_t> st = UpdateConnections(std::vector<int32_t>(1, kf), std::vector<std::vector<int32_t> >(1, vpMapPoints), exclude, &links);
        mvNewLinks = links[0];
        return st[0] == 0;
    }
    // the same for several keyframes in the order given, each leaving `exclude` out of its new links: one call.  Returns the status of each.
    std::vector<int32_t> UpdateConnections(const std::vector<int32_t>& kfs, const std::vector<std::vector<int32_t> >& pointsOfEach, const std::vector<int32_t>& exclude,
                                           std::vector<std::vector<int32_t> >* newLinks) {
        Flush();
        const size_t n = kfs.size();
        std::vector<oslam_covis_update_t> recs(n);
        std::vector<int32_t> pts;
        for (size_t i = 0; i < n; i++) {
            recs[i] = oslam_covis_update_t{graph_, kfs[i], (int32_t)pts.size(), (int32_t)pointsOfEach[i].size(), 0, (int32_t)exclude.size()};
            pts.insert(pts.end(), pointsOfEach[i].begin(), pointsOfEach[i].end());
        }
        std::vector<int32_t> status(n), ids(n * K_), ws(n * K_), nOrd(n), parent(n), links(n * K_), nLinks(n);
        oslam::throw_on(oslam_covis_update_connections(h_, (int)n, recs.data(), (int)pts.size(), pts.data(), (int)exclude.size(), exclude.data(), status.data(), ids.data(),
                                                       ws.data(), nOrd.data(), parent.data(), links.data(), nLinks.data()));
        if (newLinks) newLinks->clear();
        for (size_t i = 0; i < n; i++) {
            if (status[i] < 0) throw std::runtime_error("KeyFrame::UpdateConnections: an observation list it read had overflowed");
            if (newLinks) newLinks->push_back(std::vector<int32_t>(links.begin() + i * K_, links.begin() + i * K_ + nLinks[i]));
        }
        return status;
    }
    std::vector<int32_t> mvNewLinks;   // of the last single UpdateConnections

    // std::vector<KeyFrame*> KeyFrame::GetVectorCovisibleKeyFrames() / GetBestCovisibilityKeyFrames(const int &N) / GetCovisiblesByWeight(const int &w)
    std::vector<int32_t> GetVectorCovisibleKeyFrames(int kf) { return covisibles(kf, K_, 0); }
    std::vector<int32_t> GetBestCovisibilityKeyFrames(int kf, int N) { return covisibles(kf, N, 0); }
    std::vector<int32_t> GetCovisiblesByWeight(int kf, int w) { return covisibles(kf, K_, w); }
    const std::vector<int32_t>& orderedWeights() const { return weights_; }   // mvOrderedWeights of the entries the last of the three returned
    // std::set<KeyFrame*> KeyFrame::GetConnectedKeyFrames(), ascending: what LoopClosing::SetConnectedKeyFrames and KeyFrameDatabaseKeyFrameView::spConnected take
    std::vector<int32_t> GetConnectedKeyFrames(int kf) {
        Flush();
        const oslam_covis_key_t rec = {graph_, kf};
        std::vector<uint32_t> bits((K_ + 31) / 32);
        oslam::throw_on(oslam_covis_connected_rows(h_, 1, &rec, bits.data()));
        std::vector<int32_t> out;
        for (int i = 0; i < K_; i++)
            if ((bits[i >> 5] >> (i & 31)) & 1u) out.push_back(i);
        return out;
    }
    // int KeyFrame::GetWeight(KeyFrame* pKF)
    int GetWeight(int kf, int other) {
        Flush();
        std::vector<int32_t> w((size_t)K_ * K_);
        oslam::throw_on(oslam_covis_get_state(h_, graph_, w.data(), nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
        return w[(size_t)kf * K_ + other];
    }
    // KeyFrame* KeyFrame::GetParent(): -1 for NULL
    int GetParent(int kf) {
        Flush();
        std::vector<int32_t> p(K_);
        oslam::throw_on(oslam_covis_get_state(h_, graph_, nullptr, p.data(), nullptr, 0, nullptr, nullptr, nullptr, nullptr));
        return p[kf];
    }
    // void Tracking::UpdateLocalKeyFrames() for mCurrentFrame.mvpMapPoints = vpMapPoints (ids, -1 = NULL; the bad ones become -1, :1513).  Returns false when
    // the vote was empty (:1518: nothing else changes); otherwise mvpLocalKeyFrames is replaced and mpReferenceKF set when a keyframe won the vote.
    bool UpdateLocalKeyFrames(std::vector<int32_t>& vpMapPoints) {
        Flush();
        const oslam_covis_local_t rec = {graph_, 0, (int32_t)vpMapPoints.size()};
        std::vector<int32_t> list(K_);
        std::vector<uint8_t> null(vpMapPoints.size());
        int32_t n = 0, ref = -1;
        oslam::throw_on(oslam_covis_local_keyframes(h_, 1, &rec, (int)vpMapPoints.size(), vpMapPoints.data(), list.data(), &n, &ref, null.data()));
        if (n < -1) throw std::runtime_error("Tracking::UpdateLocalKeyFrames: an observation list it read had overflowed");
        for (size_t i = 0; i < null.size(); i++)
            if (null[i]) vpMapPoints[i] = -1;
        if (n < 0) return false;
        mvpLocalKeyFrames.assign(list.begin(), list.begin() + n);
        if (ref >= 0) mpReferenceKF = ref;
        return true;
    }
    std::vector<int32_t> mvpLocalKeyFrames;
    int mpReferenceKF = -1;

    oslam_covis_t* handle() const { return h_; }
    int graph() const { return graph_; }

private:
    void push(int32_t type, int32_t a, int32_t b, int32_t c) { events_.push_back(oslam_covis_event_t{graph_, type, a, b, c}); }
    std::vector<int32_t> covisibles(int kf, int maxN, int minW) {
        Flush();
        const oslam_covis_query_t rec = {graph_, kf, maxN, minW};
        std::vector<int32_t> ids(K_);
        weights_.assign(K_, 0);
        int32_t n = 0;
        oslam::throw_on(oslam_covis_covisibles(h_, 1, &rec, ids.data(), weights_.data(), &n));
        ids.resize(n); weights_.resize(n);
        return ids;
    }
    oslam_covis_t* h_ = nullptr;
    int K_;
    int32_t graph_;
    bool own_;
    std::vector<int32_t> overflow_;   // oslam_covis_apply answers for every graph of the handle
    std::vector<oslam_covis_event_t> events_;
    std::vector<int32_t> weights_;
};

// ORB_SLAM2::LoopClosing (include/LoopClosing.h, src/LoopClosing.cc) as far as DetectLoop (:104-230) goes, for ONE sequence: over one KeyFrameDatabase of this
// file and one detector of oslam_hip.h ("LoopClosing::DetectLoop": the restated consistency update and its normalisations).  The connected keyframes of every
// keyframe and mvConsistentGroups live on the device; candidates are ids where the reference has KeyFrame pointers.  pDB must outlive this object.
// The static ComputeScw, PropagateCorrection and UpdateMapAfterGlobalBA come from LoopClosingArithmetic.
class LoopClosing : public LoopClosingArithmetic {
public:
    // LoopClosing(Map*, KeyFrameDatabase* pDB, ORBVocabulary* pVoc, bool bFixScale): mnCovisibilityConsistencyTh = 3 (:44), mLastLoopKFid = 0 (:41)
    explicit LoopClosing(KeyFrameDatabase* pDB, int maxGroups = OSLAM_LOOPDET_MAX_GROUPS, int nCovisibilityConsistencyTh = 3) : mpKeyFrameDB(pDB) {
        oslam::throw_on(oslam_loopdet_create(&h_, pDB->handle(), maxGroups, nCovisibilityConsistencyTh));
        const size_t K = (size_t)pDB->maxKeyFrames();
        cand_.resize(K); acc_.resize(K); enough_.resize(K);
    }
    ~LoopClosing() { oslam_loopdet_destroy(h_); }
    LoopClosing(const LoopClosing&) = delete;
    LoopClosing& operator=(const LoopClosing&) = delete;

    // What the device keeps of KeyFrame::GetConnectedKeyFrames() of keyframe mnId: call it for both ends whenever a connection is added or erased
    // (KeyFrame::AddConnection / EraseConnection / UpdateConnections)
    void SetConnectedKeyFrames(int mnId, const std::vector<int32_t>& ids) {
        const oslam_loopdet_conn_t rec = {0, mnId, 0, (int32_t)ids.size()};
        oslam::throw_on(oslam_loopdet_set_connected(h_, 1, &rec, (int)ids.size(), ids.data()));
    }
    // bool DetectLoop() for mpCurrentKF = KF (its mBowVec, spConnected and, for the add, vpBestCovisibles): the gate (:115), minScore and the query
    // (:125-142), the consistency groups (:144-212), mpKeyFrameDB->add (:117, :147, :216); fills mvpEnoughConsistentCandidates
    bool DetectLoop(const KeyFrameDatabaseKeyFrameView& KF) {
        mvpEnoughConsistentCandidates.clear();
        mvpCandidateKFs.clear();
        if ((long)KF.mnId < (long)mLastLoopKFid + 10) {
            mpKeyFrameDB->add(KF);
            return false;
        }
        ids_.clear(); vals_.clear();
        for (const auto& e : *KF.mBowVec) { ids_.push_back(e.first); vals_.push_back(e.second); }
        const oslam_kfdb_query_t q = {0, KF.mnId, 0, (int32_t)ids_.size(), 0, (int32_t)KF.spConnected.size(), 0.0f, 0};
        std::vector<float> cs(KF.spConnected.size());
        int32_t n = 0, ne = 0, diag[5];
        oslam::throw_on(oslam_loopdet_detect(h_, mpKeyFrameDB->vocabulary()->handle(), 1, &q, (int)ids_.size(), ids_.data(), vals_.data(), (int)KF.spConnected.size(),
                                             KF.spConnected.data(), cand_.data(), acc_.data(), &n, diag, cs.data(), &mMinScore, enough_.data(), &ne, &mnGroups));
        if (ne < 0) throw std::runtime_error(ne == -3 ? "LoopClosing::DetectLoop: more consistent groups than the detector holds" : "LoopClosing::DetectLoop: refused");
        mvpCandidateKFs.assign(cand_.begin(), cand_.begin() + n);
        mvpEnoughConsistentCandidates.assign(enough_.begin(), enough_.begin() + ne);
        mpKeyFrameDB->add(KF);
        return !mvpEnoughConsistentCandidates.empty();
    }
    // The loop of CorrectLoop that collects LoopConnections (:547-565): for each pKFi of mvpCurrentConnectedKFs in order, UpdateConnections, then
    // GetConnectedKeyFrames() minus its previous neighbours minus mvpCurrentConnectedKFs.  pointsOfEach[i] = mvpMapPoints of connectedKFs[i] as point ids.
    // The result is what Optimizer::OptimizeEssentialGraph takes as LoopConnections.
    static std::map<int32_t, std::set<int32_t> > LoopConnections(KeyFrameGraph& graph, const std::vector<int32_t>& connectedKFs,
                                                                 const std::vector<std::vector<int32_t> >& pointsOfEach) {
        std::vector<std::vector<int32_t> > links;
        graph.UpdateConnections(connectedKFs, pointsOfEach, connectedKFs, &links);
        std::map<int32_t, std::set<int32_t> > out;
        for (size_t i = 0; i < connectedKFs.size(); i++) out[connectedKFs[i]] = std::set<int32_t>(links[i].begin(), links[i].end());
        return out;
    }
    std::vector<int32_t> mvpEnoughConsistentCandidates;   // ids
    std::vector<int32_t> mvpCandidateKFs;                 // vpCandidateKFs of the last DetectLoop that was not gated
    long unsigned int mLastLoopKFid = 0;                  // CorrectLoop sets it (:585)
    float minScore() const { return mMinScore; }          // of the last DetectLoop that was not gated
    int consistentGroups() const { return mnGroups; }     // mvConsistentGroups.size() after it

private:
    KeyFrameDatabase* mpKeyFrameDB;
    oslam_loopdet_t* h_ = nullptr;
    std::vector<uint32_t> ids_;
    std::vector<double> vals_;
    std::vector<int32_t> cand_, enough_;
    std::vector<float> acc_;
    float mMinScore = 1.0f;
    int32_t mnGroups = 0;
};

// ---- the object layer: what Tracking::TrackObject (src/Tracking.cc:1058-1076) and Tracking::UpdateCurrentObject (:1079-1207) read and write ----
struct MapPointView {                     // the members of a MapPoint the object layer reads; identity is the address, as in the reference
    float mWorldPos[3] = {0, 0, 0};
    bool mbBad = false;
    std::map<int, int> mLabelCnt;         // MapPoint::AddLabelCnt (src/MapPoint.cc:82-94)
    void AddLabelCnt(int label) { mLabelCnt[label]++; }
    bool isBad() const { return mbBad; }
};
struct Object2DView {                     // Object2D (include/ObjectTypes.h)
    int label = 0;
    float x = 0, y = 0, w = 0, h = 0;     // the 2-D box
    const uint8_t* mask = nullptr;        // CV_8UC1, the frame's size
    int mask_step = 0;
    std::vector<float> kps;               // per mvFrameKpIndices entry: mvKeysUn[i].pt.x, .pt.y, mvDepth[i] (> 0)
    float mHSVHistogram[OSLAM_OBJMATCH_BINS] = {};
    int track_id = -1;
    std::vector<int> mvFrameKpIndices;    // the frame's keypoints inside the detection (Object3D::Update, UpdateCurrentObject)
};
struct ObjectFrameView {                  // the members of a Frame the object layer touches
    const uint8_t* imRGB = nullptr;       // CV_8UC3, read as B, G, R
    int cols = 0, rows = 0, step = 0;
    float mRwc[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, mOw[3] = {0, 0, 0};
    float fx = 1, fy = 1, cx = 0, cy = 0;
    std::vector<Object2DView> mvObject2Ds;
    std::vector<int> mvpObject3Ds;        // per detection the Object3D's mTrackID, -1 = NULL
    std::vector<int> mvObject3DLabels;    // per detection that Object3D's mLabel (MatchTwoFrame reads pObj3D->mLabel of the previous frame)
    std::vector<MapPointView*> mvpMapPoints;   // per keypoint, NULL = none; with mvbOutlier what Object3D::Update and UpdateCurrentObject read
    std::vector<bool> mvbOutlier;
};
struct ObjectObservationView {            // ObjectObservation: ObjectCenterW and AppearanceVec (ObsCamPoseTcw only feeds the unused view vectors)
    float ObjectCenterW[3];
    float AppearanceVec[OSLAM_OBJMATCH_BINS];
};
struct Object3DView {
    int mTrackID = -1;
    int mLabel = 0;
    std::vector<ObjectObservationView> mvObservations;
};

// ORB_SLAM2::ObjectMatcher (include/ObjectMatcher.h): MatchTwoFrame (src/ObjectMatcher.cc:47-440) and MatchMapToFrame (:442-801), one problem per call.
class ObjectMatcher {
public:
    ObjectMatcher() {}
    ~ObjectMatcher() { oslam_objmatch_destroy(h_); }
    ObjectMatcher(const ObjectMatcher&) = delete;
    ObjectMatcher& operator=(const ObjectMatcher&) = delete;
    oslam_objmatch_params_t params = {0.8, 0.5, 0.3, 0.1};   // the literals of :430, :783 and :789

    // void MatchTwoFrame(Frame &PreF, Frame &CurF): CurF.mvpObject3Ds and the track_id of the claimed detections are written.
    void MatchTwoFrame(const ObjectFrameView& PreF, ObjectFrameView& CurF) {
        const int nPre = (int)PreF.mvObject2Ds.size(), nCur = (int)CurF.mvObject2Ds.size();
        if ((int)PreF.mvpObject3Ds.size() != nPre || (int)PreF.mvObject3DLabels.size() != nPre || (int)CurF.mvpObject3Ds.size() != nCur)
            throw std::runtime_error("MatchTwoFrame: mvpObject3Ds must have one entry per detection");
        ensure(1, 1, 1, 1, 1, std::max(nPre, nCur));
        std::vector<int32_t> plabel(nPre), pid(nPre), clabel(nCur), cid(nCur);
        std::vector<float> phist, pbox, chist, cbox;
        for (int i = 0; i < nPre; i++) {
            pid[i] = PreF.mvpObject3Ds[i]; plabel[i] = PreF.mvObject3DLabels[i];
            append(PreF.mvObject2Ds[i], phist, pbox);
        }
        for (int j = 0; j < nCur; j++) {
            cid[j] = CurF.mvpObject3Ds[j]; clabel[j] = CurF.mvObject2Ds[j].label;
            append(CurF.mvObject2Ds[j], chist, cbox);
        }
        oslam_objmatch_det_rows_t pre = {}, cur = {};
        pre.n_rows = nPre; pre.label = plabel.data(); pre.hist = phist.data(); pre.box = pbox.data(); pre.obj3d = pid.data();
        cur.n_rows = nCur; cur.label = clabel.data(); cur.hist = chist.data(); cur.box = cbox.data(); cur.obj3d = cid.data();
        oslam_objmatch_pair_problem_t pr = {};
        pr.n_pre = nPre; pr.n_cur = nCur;
        std::vector<float> sim((size_t)nPre * nCur), iou((size_t)nPre * nCur);
        int32_t n = 0, status = 0;
        oslam::throw_on(oslam_objmatch_match_two_frame(h_, 1, &pr, &pre, &cur, &params, nPre * nCur, sim.data(), iou.data(), &n, &status));
        if (status != OSLAM_OBJMATCH_DONE) throw std::runtime_error("MatchTwoFrame: the problem was refused");
        take_claims(CurF, cid);
    }

    // void MatchMapToFrame(vector<Object3D*> vpObject3Ds, Frame &F).  The reference's order is that of a std::set of pointers; pass ascending mTrackID.
    void MatchMapToFrame(const std::vector<Object3DView>& vpObject3Ds, ObjectFrameView& F) {
        const int nObj = (int)vpObject3Ds.size(), nCur = (int)F.mvObject2Ds.size();
        if ((int)F.mvpObject3Ds.size() != nCur) throw std::runtime_error("MatchMapToFrame: mvpObject3Ds must have one entry per detection");
        std::vector<int32_t> clabel(nCur), cid(nCur), koff(nCur), kn(nCur), oid(nObj), olabel(nObj), ooff(nObj), on(nObj);
        std::vector<float> chist, cbox, kps, ocen, ohist;
        for (int j = 0; j < nCur; j++) {
            const Object2DView& d = F.mvObject2Ds[j];
            cid[j] = F.mvpObject3Ds[j]; clabel[j] = d.label; koff[j] = (int)kps.size() / 3; kn[j] = (int)d.kps.size() / 3;
            append(d, chist, cbox);
            kps.insert(kps.end(), d.kps.begin(), d.kps.end());
        }
        for (int i = 0; i < nObj; i++) {
            const Object3DView& o = vpObject3Ds[i];
            oid[i] = o.mTrackID; olabel[i] = o.mLabel; ooff[i] = (int)ocen.size() / 3; on[i] = (int)o.mvObservations.size();
            for (const ObjectObservationView& ob : o.mvObservations) {
                ocen.insert(ocen.end(), ob.ObjectCenterW, ob.ObjectCenterW + 3);
                ohist.insert(ohist.end(), ob.AppearanceVec, ob.AppearanceVec + OSLAM_OBJMATCH_BINS);
            }
        }
        ensure(1, 1, nObj, (int)ocen.size() / 3, (int)kps.size() / 3, nCur);
        oslam_objmatch_det_rows_t cur = {};
        cur.n_rows = nCur; cur.label = clabel.data(); cur.hist = chist.data(); cur.obj3d = cid.data(); cur.kp_off = koff.data(); cur.kp_n = kn.data();
        cur.n_kps = (int)kps.size() / 3; cur.kps = kps.data();
        oslam_objmatch_obj_rows_t obj = {};
        obj.n_rows = nObj; obj.obj3d_id = oid.data(); obj.label = olabel.data(); obj.obs_off = ooff.data(); obj.obs_n = on.data();
        obj.n_obs = (int)ocen.size() / 3; obj.obs_center = ocen.data(); obj.obs_hist = ohist.data();
        oslam_objmatch_map_problem_t pr = {};
        pr.n_cur = nCur; pr.n_obj = nObj;
        std::memcpy(pr.Rwc, F.mRwc, sizeof pr.Rwc); std::memcpy(pr.Ow, F.mOw, sizeof pr.Ow);
        pr.fx = F.fx; pr.fy = F.fy; pr.cx = F.cx; pr.cy = F.cy;
        const size_t ns = (size_t)nObj * nCur;
        std::vector<float> sim(ns), mean(ns), mind(ns);
        int32_t bySim = 0, byDist = 0, status = 0;
        oslam::throw_on(oslam_objmatch_match_map_to_frame(h_, 1, &pr, &cur, &obj, &params, (int)ns, sim.data(), mean.data(), mind.data(), &bySim, &byDist, &status));
        if (status != OSLAM_OBJMATCH_DONE) throw std::runtime_error("MatchMapToFrame: the problem was refused (an object without observations, a detection without keypoints)");
        take_claims(F, cid);
    }

    // (used by ExtractHSVHistogramsFromMask below) the handle, grown to hold what a call needs
    oslam_objmatch_t* ensure(int w, int h, int nObj, int nObs, int nKps, int nDet) {
        if (nDet > OSLAM_OBJMATCH_MAX_DETECTIONS) throw std::runtime_error("ObjectMatcher: more than 32 detections in a frame");
        if (h_ && w <= cap_[0] && h <= cap_[1] && nObj <= cap_[2] && nObs <= cap_[3] && nKps <= cap_[4]) return h_;
        const int want[5] = {w, h, nObj, nObs, nKps}, least[5] = {640, 480, 64, 4096, 4096};
        for (int k = 0; k < 5; k++) cap_[k] = std::max(cap_[k], std::max(least[k], k < 2 ? want[k] : want[k] + want[k] / 2));
        oslam_objmatch_destroy(h_);
        h_ = nullptr;
        oslam::throw_on(oslam_objmatch_create(&h_, 1, cap_[0], cap_[1], OSLAM_OBJMATCH_MAX_DETECTIONS, cap_[2], cap_[3], cap_[4]));
        return h_;
    }

private:
    static void append(const Object2DView& d, std::vector<float>& hist, std::vector<float>& box) {
        hist.insert(hist.end(), d.mHSVHistogram, d.mHSVHistogram + OSLAM_OBJMATCH_BINS);
        const float b[4] = {d.x, d.y, d.w, d.h};
        box.insert(box.end(), b, b + 4);
    }
    static void take_claims(ObjectFrameView& F, const std::vector<int32_t>& cid) {
        for (size_t j = 0; j < cid.size(); j++) {
            if (cid[j] != F.mvpObject3Ds[j]) F.mvObject2Ds[j].track_id = cid[j];   // :433-434, :786-787, :792-793
            F.mvpObject3Ds[j] = cid[j];
        }
    }
    oslam_objmatch_t* h_ = nullptr;
    int cap_[5] = {0, 0, 0, 0, 0};
};

// cv::Mat Frame::ExtractHSVHistogramsFromMask(const cv::Mat &imRGB, cv::Mat &mask) (src/Frame.cc:388-414) for every detection of the frame at once: the image is
// read once, mHSVHistogram of every Object2D is written.
inline void ExtractHSVHistogramsFromMask(ObjectMatcher& matcher, ObjectFrameView& F) {
    const int n = (int)F.mvObject2Ds.size();
    if (n == 0) return;
    if (!F.imRGB || F.cols < 1 || F.rows < 1 || F.step < 3 * F.cols) throw std::runtime_error("ExtractHSVHistogramsFromMask: no image");
    oslam_objmatch_t* h = matcher.ensure(F.cols, F.rows, 1, 1, 1, n);
    std::vector<uint8_t> masks((size_t)n * F.rows * F.cols);
    for (int k = 0; k < n; k++) {
        const Object2DView& d = F.mvObject2Ds[k];
        if (!d.mask || d.mask_step < F.cols) throw std::runtime_error("ExtractHSVHistogramsFromMask: a detection without a mask");
        for (int y = 0; y < F.rows; y++) std::memcpy(masks.data() + ((size_t)k * F.rows + y) * F.cols, d.mask + (size_t)y * d.mask_step, F.cols);
    }
    const oslam_objmatch_frame_t fr = {n, 0};
    std::vector<int32_t> counts((size_t)n * OSLAM_OBJMATCH_BINS);
    std::vector<float> hist((size_t)n * OSLAM_OBJMATCH_BINS);
    oslam::throw_on(oslam_objmatch_hsv_histograms(h, 1, F.cols, F.rows, F.step, F.cols, F.imRGB, &fr, n, masks.data(), counts.data(), hist.data()));
    for (int k = 0; k < n; k++) std::memcpy(F.mvObject2Ds[k].mHSVHistogram, hist.data() + (size_t)k * OSLAM_OBJMATCH_BINS, sizeof(float) * OSLAM_OBJMATCH_BINS);
}

// ---- the object map: Object3D (include/ObjectTypes.h) and Map::ObjectMapRegularization (src/Map.cc:67-157) over oslam_hip.h's "Object map maintenance" ----
#define OSLAM_MIN_OBJ3DMP_NUM 5   // MIN_OBJ3DMP_NUM (include/ObjectTypes.h)

namespace objmap_detail {
// one handle for the process: the calls are one problem each, synchronous
inline oslam_objmap_t* handle() {
    struct Holder {
        oslam_objmap_t* h = nullptr;
        ~Holder() { oslam_objmap_destroy(h); }
    };
    static Holder holder;
    if (!holder.h) oslam::throw_on(oslam_objmap_create(&holder.h, 1, OSLAM_OBJMAP_MIN_CLUSTER_POINTS, OSLAM_OBJMAP_MAX_OBJECTS));
    return holder.h;
}
inline void positions(const std::vector<MapPointView*>& vpMps, std::vector<float>& pos) {
    pos.resize(3 * vpMps.size());
    for (size_t i = 0; i < vpMps.size(); i++) std::memcpy(pos.data() + 3 * i, vpMps[i]->mWorldPos, sizeof(float) * 3);
}
// the rejection of one list; vpMps is reduced to the kept points (ReduceVector).  Returns the result record.
inline oslam_objmap_result_t reject(std::vector<MapPointView*>& vpMps, int mode, int label) {
    const int n = (int)vpMps.size();
    std::vector<float> pos;
    positions(vpMps, pos);
    std::vector<int32_t> cnt(n, 0), sum(n, 0), cluster(n, -1);
    if (mode == OSLAM_OBJMAP_MODE_UPDATE)
        for (int i = 0; i < n; i++) {   // MapPoint::GetLabelProb (src/MapPoint.cc:109-137) as its two integers
            const std::map<int, int>& m = vpMps[i]->mLabelCnt;
            const auto it = m.find(label);
            cnt[i] = it == m.end() ? 0 : it->second;
            for (const auto& e : m) sum[i] += e.second;
        }
    std::vector<uint8_t> keep(n, 0);
    oslam_objmap_problem_t pr = {0, n, mode, 0};
    oslam_objmap_result_t res = {};
    oslam::throw_on(oslam_objmap_reject_outliers(handle(), 1, &pr, n, pos.data(), cnt.data(), sum.data(), keep.data(), cluster.data(), &res));
    if (res.status != OSLAM_OBJMAP_DONE) throw std::runtime_error("RejectOutliers: the problem was refused (more clustering points than the handle holds)");
    size_t j = 0;
    for (int i = 0; i < n; i++)
        if (keep[i]) vpMps[j++] = vpMps[i];
    vpMps.resize(j);
    return res;
}
}  // namespace objmap_detail

// The new-object path of Tracking::UpdateCurrentObject (src/Tracking.cc:1138-1199) on the detection's map points (:1120-1137): clustering, the shortcut, the
// two rules and ReduceVector.  Returns whether an Object3D is to be created from what vpCandidateMps holds afterwards.
inline bool RejectNewObjectOutliers(std::vector<MapPointView*>& vpCandidateMps) {
    if (vpCandidateMps.empty()) return false;
    const oslam_objmap_result_t res = objmap_detail::reject(vpCandidateMps, OSLAM_OBJMAP_MODE_NEW_OBJECT, 0);
    return res.path == OSLAM_OBJMAP_PATH_SHORTCUT || (int)vpCandidateMps.size() > OSLAM_MIN_OBJ3DMP_NUM;
}

class Object3D {
public:
    static int& nNextId() { static int n = 0; return n; }
    // Object3D(vector<MapPoint*> &vpObj3DMps, int Obj2DidxF, Frame* F) (src/ObjectTypes.cc:33-53); MapPoint::SetInsertedTime is bookkeeping nothing here reads
    Object3D(const std::vector<MapPointView*>& vpObj3DMps, int Obj2DidxF, ObjectFrameView& F) : mvpMapPoints(vpObj3DMps) {
        Object2DView& Obj2D = F.mvObject2Ds[Obj2DidxF];
        mTrackID = nNextId()++;
        mLabel = Obj2D.label;
        Obj2D.track_id = mTrackID;
        CalculateCenterAndSize();
        AddObservation(Obj2D);
    }
    // void Update(int Obj2DidxF, Frame *F) (:55-139)
    void Update(int Obj2DidxF, ObjectFrameView& F) {
        mUpdateCnt++;
        Object2DView& Obj2D = F.mvObject2Ds[Obj2DidxF];
        Obj2D.track_id = mTrackID;
        std::vector<MapPointView*> vpCandidateMps;
        for (int idx : Obj2D.mvFrameKpIndices) {   // :65-88
            MapPointView* pMp = F.mvpMapPoints[idx];
            if (!pMp || pMp->isBad() || F.mvbOutlier[idx]) continue;
            if (!std::count(mvpMapPoints.begin(), mvpMapPoints.end(), pMp)) vpCandidateMps.push_back(pMp);   // (a point twice in the detection is appended twice, as there)
        }
        for (MapPointView* p : vpCandidateMps) { mvpMapPoints.push_back(p); mnNewAddedMpNum++; }   // :89-97
        RejectOutliers();           // :117-124
        CalculateCenterAndSize();   // :130
        AddObservation(Obj2D);      // :131-132
        if (mUpdateCnt > 5 && mvpMapPoints.size() < 5) mbVaild = false;   // :135-138
    }
    // void RejectOutliers() (:152-162): RejectOutliersTEST5 above 3000 points, RejectOutliersTEST7 otherwise
    void RejectOutliers() {
        mnNewAddedMpNum = 0;
        if (mvpMapPoints.empty()) return;
        objmap_detail::reject(mvpMapPoints, OSLAM_OBJMAP_MODE_UPDATE, mLabel);
    }
    // void CalculateCenterAndSize() (:805-833); an empty list leaves the members as they are
    void CalculateCenterAndSize() {
        const int n = (int)mvpMapPoints.size();
        if (n == 0) return;
        std::vector<float> pos;
        objmap_detail::positions(mvpMapPoints, pos);
        oslam_objmap_problem_t pr = {0, n, 0, 0};
        oslam_objmap_result_t res = {};
        oslam::throw_on(oslam_objmap_center_and_size(objmap_detail::handle(), 1, &pr, n, pos.data(), &res));
        std::memcpy(mCenterW, res.center, sizeof mCenterW);
        mMaxXw = res.bbox[0]; mMaxYw = res.bbox[1]; mMaxZw = res.bbox[2]; mMinXw = res.bbox[3]; mMinYw = res.bbox[4]; mMinZw = res.bbox[5];
    }
    bool isVaild() const { return mbVaild; }
    Object3DView view() const {   // what ObjectMatcher::MatchMapToFrame reads
        Object3DView v;
        v.mTrackID = mTrackID; v.mLabel = mLabel; v.mvObservations = mvObservations;
        return v;
    }

    int mTrackID = -1, mLabel = 0, mUpdateCnt = 0, mnNewAddedMpNum = 0;
    bool mbVaild = true;
    float mCenterW[3] = {0, 0, 0};
    float mMaxXw = 0, mMaxYw = 0, mMaxZw = 0, mMinXw = 0, mMinYw = 0, mMinZw = 0;
    std::vector<MapPointView*> mvpMapPoints;
    std::vector<ObjectObservationView> mvObservations;
    Object3D* mpReplaced = nullptr;

private:
    void AddObservation(const Object2DView& Obj2D) {
        ObjectObservationView obs;
        std::memcpy(obs.ObjectCenterW, mCenterW, sizeof mCenterW);
        std::memcpy(obs.AppearanceVec, Obj2D.mHSVHistogram, sizeof obs.AppearanceVec);
        mvObservations.push_back(obs);
    }
};

// void Map::MergeObject(vector<Object3D*> vpObj3DtoMerge) (src/Map.cc:114-157) with the target the device named: the list surgery on the host
inline void MergeObject(const std::vector<Object3D*>& vpObj3DtoMerge, int target) {
    std::vector<MapPointView*> vpNewMapPoints;
    std::vector<ObjectObservationView> vNewObs;
    for (Object3D* pObj3D : vpObj3DtoMerge) {
        vpNewMapPoints.insert(vpNewMapPoints.end(), pObj3D->mvpMapPoints.begin(), pObj3D->mvpMapPoints.end());
        vNewObs.insert(vNewObs.end(), pObj3D->mvObservations.begin(), pObj3D->mvObservations.end());
    }
    Object3D* pTargetObj3D = vpObj3DtoMerge[target];
    pTargetObj3D->mvpMapPoints.swap(vpNewMapPoints);
    pTargetObj3D->mvObservations.swap(vNewObs);
    if (std::abs((int)pTargetObj3D->mvpMapPoints.size() - (int)vpNewMapPoints.size()) > 50) pTargetObj3D->RejectOutliers();
    pTargetObj3D->CalculateCenterAndSize();
    pTargetObj3D->mUpdateCnt++;
    for (size_t idx = 0; idx < vpObj3DtoMerge.size(); idx++)
        if ((int)idx != target) vpObj3DtoMerge[idx]->mpReplaced = pTargetObj3D;
}

// void Map::ObjectMapRegularization() (src/Map.cc:67-112) over GetAllObject3Ds() in the caller's order (the reference's is that of a std::set of pointers; pass
// ascending mTrackID): the merge sets on the device, MergeObject per set in set order on the host.  Objects that were replaced are taken out of vpObj3Ds
// (mspObject3Ds.erase) and returned; they stay alive, their mpReplaced names the target.
inline std::vector<Object3D*> ObjectMapRegularization(std::vector<Object3D*>& vpObj3Ds) {
    const int N = (int)vpObj3Ds.size();
    std::vector<Object3D*> erased;
    if (N < 2) return erased;
    if (N > OSLAM_OBJMAP_MAX_OBJECTS) throw std::runtime_error("ObjectMapRegularization: more than 128 objects in the map");
    std::vector<int32_t> label(N), track(N), target(N, -1);
    std::vector<float> bbox(6 * (size_t)N), ratio((size_t)N * N);
    std::vector<uint8_t> member((size_t)N * N, 0);
    for (int i = 0; i < N; i++) {
        const Object3D* o = vpObj3Ds[i];
        label[i] = o->mLabel; track[i] = o->mTrackID;
        const float b[6] = {o->mMaxXw, o->mMaxYw, o->mMaxZw, o->mMinXw, o->mMinYw, o->mMinZw};
        std::memcpy(bbox.data() + 6 * (size_t)i, b, sizeof b);
    }
    oslam_objmap_merge_problem_t pr = {N, 0, 0, 0};
    int32_t n_sets = 0, status = 0;
    oslam::throw_on(oslam_objmap_merge_sets(objmap_detail::handle(), 1, &pr, N, label.data(), track.data(), bbox.data(), 6, N * N, ratio.data(), member.data(), target.data(), &n_sets, &status));
    if (status != OSLAM_OBJMAP_DONE) throw std::runtime_error("ObjectMapRegularization: the problem was refused");
    std::set<Object3D*> gone;
    for (int s = 0; s < n_sets; s++) {
        std::vector<Object3D*> vpObj3DtoMerge;
        int t = -1;
        for (int i = 0; i < N; i++)
            if (member[(size_t)s * N + i]) {
                if (i == target[s]) t = (int)vpObj3DtoMerge.size();
                vpObj3DtoMerge.push_back(vpObj3Ds[i]);
            }
        MergeObject(vpObj3DtoMerge, t);
        for (size_t k = 0; k < vpObj3DtoMerge.size(); k++)
            if ((int)k != t) gone.insert(vpObj3DtoMerge[k]);
    }
    std::vector<Object3D*> left;
    for (Object3D* o : vpObj3Ds) (gone.count(o) ? erased : left).push_back(o);
    vpObj3Ds.swap(left);
    return erased;
}

}  // namespace ORB_SLAM2
