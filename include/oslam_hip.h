/*
 * oslam_hip.h — C ABI of the MI355X-native (gfx950) front-end + local-BA hot path of
 * yangliu9527/Object_SLAM (an ORB_SLAM2 fork).  Plain pointers and sizes only; no C++ / torch
 * types.  Every entry point returns 0 on success or a negative OSLAM_E_* code;
 * oslam_last_error() gives a thread-local message.  One handle per caller thread / HIP stream;
 * handles are not re-entrant (same contract as the reference classes, which own their buffers).
 *
 * Each declaration cites the reference interface (file:line under the reference tree) it
 * replaces.  INTEGRATION.md shows the adapter a maintainer adds on the reference side.
 */
#ifndef OSLAM_HIP_H
#define OSLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OSLAM_OK 0
#define OSLAM_E_INVALID (-1)   /* bad argument / unsupported shape */
#define OSLAM_E_HIP (-2)       /* HIP runtime error (no device, OOM, launch failure) */
#define OSLAM_E_CAPACITY (-3)  /* caller buffer or internal arena too small (never truncates silently) */
#define OSLAM_E_NUMERIC (-4)   /* solver failure */

#define OSLAM_MAX_LEVELS 16

/* cv::KeyPoint POD mirror (OpenCV 3.2 core/types.hpp; used at include/ORBextractor.h:59-61). */
typedef struct oslam_keypoint {
    float x, y;       /* pt */
    float size;
    float angle;      /* degrees [0,360) */
    float response;   /* FAST score */
    int32_t octave;
    int32_t class_id; /* -1 */
} oslam_keypoint_t;

const char* oslam_last_error(void);
/* Number of visible HIP devices (0 if none); never throws. */
int oslam_device_count(void);

/* ------------------------------------------------------------------------------------------
 * ORBextractor — replaces ORB_SLAM2::ORBextractor (include/ORBextractor.h:45-110,
 * src/ORBextractor.cc:410-470 ctor, :1043-1105 operator()).
 * The handle is created for one image geometry and a maximum batch of images per call;
 * batch > 1 is the batch-of-sequences mode (independent images, same arithmetic per image).
 * ---------------------------------------------------------------------------------------- */
typedef struct oslam_orb oslam_orb_t;

int oslam_orb_create(oslam_orb_t** out, int nfeatures, float scaleFactor, int nlevels, int iniThFAST,
                     int minThFAST, int width, int height, int max_batch, int device);
void oslam_orb_destroy(oslam_orb_t* h);

/* Getters of include/ORBextractor.h:63-83; each array has nlevels entries (any may be NULL). */
int oslam_orb_get_scale_tables(const oslam_orb_t* h, float* scaleFactors, float* invScaleFactors,
                               float* levelSigma2, float* invLevelSigma2, int* nFeaturesPerLevel);
/* cv::GaussianBlur column-pass rounding model (DESIGN.md "blur rounding"): 1 (default) = OpenCV 3.2
 * on x86 SSE2 (half-to-even for x < (w & ~3), half-up tail); 0 = scalar fixed point everywhere. */
int oslam_orb_set_blur_rounding(oslam_orb_t* h, int sse2);
/* Per image capacity of the keypoint / descriptor outputs (sum of per-level node caps). */
int oslam_orb_max_keypoints(const oslam_orb_t* h);

/* operator() drop-in (src/ORBextractor.cc:1043): host gray image in, host keypoints +
 * descriptors (n x 32 bytes, row-major) out.  Empty image -> *n_out = 0, returns 0 (the
 * reference returns silently, :1046).  cap < n -> OSLAM_E_CAPACITY with *n_out = n. */
int oslam_orb_extract(oslam_orb_t* h, const uint8_t* gray, int width, int height, int stride,
                      oslam_keypoint_t* keypoints, uint8_t* descriptors, int cap, int* n_out);

/* Batch mode, everything resident in HBM: d_gray holds `batch` images (row pitch `stride`
 * bytes, `image_stride` bytes between images).  Asynchronous on `stream` (a hipStream_t, may be
 * NULL = default stream); results stay on the device, see oslam_orb_results_device(). */
int oslam_orb_extract_batch_device(oslam_orb_t* h, const uint8_t* d_gray, int batch, int stride,
                                   size_t image_stride, void* stream);
/* Device pointers of the last batch: keypoints [batch][cap] (oslam_keypoint_t), descriptors
 * [batch][cap][32], counts [batch] (int32), cap = oslam_orb_max_keypoints().  status[0] != 0
 * after the stream has drained means an internal arena overflowed (OSLAM_E_CAPACITY). */
int oslam_orb_results_device(const oslam_orb_t* h, const oslam_keypoint_t** d_keypoints,
                             const uint8_t** d_descriptors, const int32_t** d_counts,
                             const int32_t** d_status);
/* Synchronise the stream and copy image b's results of the last batch to the host. */
int oslam_orb_fetch(oslam_orb_t* h, int b, oslam_keypoint_t* keypoints, uint8_t* descriptors, int cap,
                    int* n_out);

/* mvImagePyramid (public member, include/ORBextractor.h:85; read by Frame::ComputeStereoMatches,
 * src/Frame.cc:713,803,815): level image b of the last batch, host copy (w*h bytes, tight) or
 * device view. */
int oslam_orb_level_size(const oslam_orb_t* h, int level, int* width, int* height);
int oslam_orb_get_pyramid_level(oslam_orb_t* h, int b, int level, uint8_t* out);
int oslam_orb_pyramid_level_device(const oslam_orb_t* h, int b, int level, const uint8_t** d_ptr,
                                   int* pitch);

/* Stage outputs for parity tests (host copies; call after a batch has run). */
int oslam_orb_debug_get_blurred(oslam_orb_t* h, int b, int level, uint8_t* out);
/* FAST candidates of a level in reference order (x, y in region coords, response):
 * src/ORBextractor.cc:789-829.  out is [cap][3] int32; returns count in *n_out. */
int oslam_orb_debug_get_candidates(oslam_orb_t* h, int b, int level, int32_t* out, int cap, int* n_out);
/* Quad-tree survivors of a level in reference order (level coords): src/ORBextractor.cc:834-847. */
int oslam_orb_debug_get_level_keys(oslam_orb_t* h, int b, int level, int32_t* out, int cap, int* n_out);

/* Which kernel variants the last batch launched.  Every field is written where the library takes the
 * decision, from the value that selects the kernel (nothing is derived a second time), so a parity
 * test can assert that the variant it is meant to pin really ran.  big_cell and skipped_cells are fixed
 * when the handle is created (they go into the FAST cell records); everything else is per launch, and
 * per issued half when the batch is cut in two (n_halves 1 or 2). */
#define OSLAM_ORB_RESIZE_NONE 0    /* level 0, or nothing launched yet */
#define OSLAM_ORB_RESIZE_PLAIN 1   /* k_resize: byte loads */
#define OSLAM_ORB_RESIZE_WORDS 2   /* k_resize_words: quad tables, 4-byte aligned source rows */
#define OSLAM_ORB_RESIZE_LDS 3     /* k_resize_lds: quad tables, source tile staged in LDS, 16-byte aligned source rows */
typedef struct oslam_orb_plan {
    int32_t nlevels;
    int32_t batch;
    int32_t n_halves;
    int32_t half_nb[2];                               /* images of the half */
    int32_t half_kpw[2];                              /* keypoints per wavefront of its k_orient_describe */
    int32_t half_src_aligned4[2];                     /* level-0 rows of the half taken as 4-byte aligned (level-1 resize; FAST, blur and
                                                         k_orient_describe test the same pitch and pointer bits per image); -1 with one level */
    int32_t half_src_aligned16[2];                    /* ... as 16-byte aligned; -1 with one level */
    int32_t half_oct_nodes_hbm[2];                    /* 1: k_octree_hbm (node tables in HBM), 0: k_octree + k_octree_spill */
    int32_t half_big_cell_kernel[2];                  /* 1: k_fast_cells was launched beside k_fast_cells_wave */
    int32_t half_resize[2][OSLAM_MAX_LEVELS];         /* OSLAM_ORB_RESIZE_* per level */
    int32_t big_cell[OSLAM_MAX_LEVELS];               /* 1: the level's cells exceed the per-wavefront kernel and are left to k_fast_cells */
    int32_t skipped_cells[OSLAM_MAX_LEVELS];          /* cells of the level recorded as empty (valid == 2) */
} oslam_orb_plan_t;
int oslam_orb_debug_get_plan(const oslam_orb_t* h, oslam_orb_plan_t* out);

/* Kernel-group timing with HIP events recorded on the launch stream (bench.py's roofline leg).
 * Groups: 0 pyramid (K1 x (nlevels-1)), 1 FAST cells (K2/K3), 2 blur (K6 x nlevels), 3 quad-tree (K4),
 * 4 orientation + descriptors (K5/K7).  get_profile returns accumulated milliseconds since
 * set_profiling(h, 1) and the number of batches / images they cover. */
int oslam_orb_set_profiling(oslam_orb_t* h, int on);
int oslam_orb_get_profile(oslam_orb_t* h, double ms[5], long long* batches, long long* images);

/* Phase cycle counters of profiling builds (-DOSLAM_FAST_PROFILE); zeros otherwise. */
int oslam_orb_debug_counters(oslam_orb_t* h, unsigned long long out[16], int reset);

/* Work model of one extract call: algorithmic bytes per image. */
/* Synchronous device-to-host copy (tests and tools read the *_results_device arrays with it). */
int oslam_memcpy_from_device(void* dst, const void* d_src, size_t bytes);
int64_t oslam_orb_algorithmic_bytes(const oslam_orb_t* h, int n_keypoints);

/* ------------------------------------------------------------------------------------------
 * ORBmatcher — replaces the projection searches of ORB_SLAM2::ORBmatcher (include/ORBmatcher.h:41-83)
 * and the Frame grid they query (src/Frame.cc:455-470 AssignFeaturesToGrid, :567-620
 * GetFeaturesInArea, :622-632 PosInGrid).  Constants TH_HIGH=100, TH_LOW=50, HISTO_LENGTH=30
 * (src/ORBmatcher.cc:37-39).
 * ---------------------------------------------------------------------------------------- */
typedef struct oslam_matcher oslam_matcher_t;

/* One projected map point: what SearchByProjection reads from the MapPoint (mTrackProjX/Y/XR,
 * mnTrackScaleLevel, GetDescriptor(), Observations()) or computes from the last frame. 64 bytes. */
typedef struct oslam_proj_query {
    float u, v;            /* mTrackProjX, mTrackProjY (src/ORBmatcher.cc:67) / projection (:1370-1371) */
    float ur;              /* mTrackProjXR (:93) / u - mbf*invzc (:1411) */
    float radius;          /* r*mvScaleFactors[level] (:67) / th*mvScaleFactors[octave] (:1381) */
    int32_t minLevel, maxLevel; /* GetFeaturesInArea level gate (src/Frame.cc:567) */
    int32_t flags;         /* bit0: searched (mbTrackInView && !isBad()); bit1: Observations()>0 (blocks
                              later candidates, src/ORBmatcher.cc:87-89) */
    float angle;           /* LastFrame.mvKeysUn[i].angle for the rotation histogram (:1432) */
    uint8_t desc[32];      /* pMP->GetDescriptor() */
} oslam_proj_query_t;

/* Frame side of a search, batch of frames in HBM (device pointers), fixed per-frame stride. */
typedef struct oslam_match_frames {
    const oslam_keypoint_t* keysUn; /* mvKeysUn [batch][kp_stride] */
    int kp_stride;                  /* 1 <= kp_stride <= max_keypoints of the handle (OSLAM_E_CAPACITY above it, nothing is launched) */
    const float* uRight;            /* mvuRight [batch][kp_stride], NULL = monocular (-1) */
    const uint8_t* desc;            /* mDescriptors [batch][kp_stride][32] */
    const uint8_t* blocked;         /* [batch][kp_stride]: mvpMapPoints[i] && Observations()>0 before the call; NULL = none */
    const int32_t* n_kps;           /* [batch] (device) or NULL -> n_kps_const */
    int n_kps_const;
    float minX, minY, maxX, maxY;   /* mnMinX.. (src/Frame.cc:691-702) */
} oslam_match_frames_t;

/* Last-frame side of SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1328). */
typedef struct oslam_match_last {
    const float* Xw;                /* [batch][kp_stride][3] pMP->GetWorldPos() */
    const uint8_t* has_mp;          /* bit0: mvpMapPoints[i] && !mvbOutlier[i]; bit1: Observations()>0 */
    const oslam_keypoint_t* keys;   /* LastFrame.mvKeysUn (octave, angle) */
    const uint8_t* mp_desc;         /* [batch][kp_stride][32] pMP->GetDescriptor() */
    int kp_stride;
    const int32_t* n_kps;           /* [batch] (device) or NULL -> n_kps_const */
    int n_kps_const;
} oslam_match_last_t;

typedef struct oslam_camera { float fx, fy, cx, cy, bf, b; } oslam_camera_t;

/* max_keypoints <= 2400: one frame's keypoints, descriptors and 64x48 grid live in 160 KiB of LDS. */
int oslam_matcher_create(oslam_matcher_t** out, int max_batch, int max_keypoints, int max_queries, int device);
void oslam_matcher_destroy(oslam_matcher_t* h);

/* Windowed Hamming search with the reference's sequential claim order (a later query skips a keypoint
 * claimed by an earlier observed map point).  use_ratio=1, check_ori=0: SearchByProjection(Frame&,
 * vector<MapPoint*>&, th) (src/ORBmatcher.cc:45-129).  use_ratio=0: the search half of
 * SearchByProjection(Cur, Last) (:1394-1467).  d_queries NULL = the handle's internal query buffer
 * (filled by oslam_match_project_last_batch_device).  Asynchronous on `stream`. */
int oslam_match_search_batch_device(oslam_matcher_t* h, const oslam_match_frames_t* frames,
                                    const oslam_proj_query_t* d_queries, int q_stride, const int32_t* d_n_queries,
                                    int n_queries_const, int batch, float nnratio, int use_ratio, int check_ori,
                                    int th_high, void* stream);
/* Projection half of SearchByProjection(Cur, Last) (src/ORBmatcher.cc:1338-1392): fills the internal
 * query buffer (stride last->kp_stride) from the last frame's map points. d_Tcw/d_Tlw: [batch][16]
 * row-major float (cv::Mat CV_32F mTcw). */
int oslam_match_project_last_batch_device(oslam_matcher_t* h, const oslam_match_last_t* last, const float* d_Tcw,
                                          const float* d_Tlw, const oslam_camera_t* cam,
                                          const oslam_match_frames_t* cur, const float* scaleFactors, int nlevels,
                                          float th, int bMono, int batch, void* stream);
/* Device results of the last search: q_match/q_dist [batch][q_stride] (keypoint index or -1, Hamming
 * distance), kp_match [batch][kp_stride] (the strides of that search's arguments, frames->kp_stride <=
 * max_keypoints; query index now held in mvpMapPoints[k]; -1 untouched; -2 set to NULL by the rotation
 * check), nmatches [batch] (return value of the reference call).  Entries beyond a frame's counts are
 * unspecified.  queries / n_queries: the internal query buffer [batch][last->kp_stride] and counts [batch]
 * that oslam_match_project_last_batch_device filled (pass n_queries as d_n_queries of the search that
 * follows it with d_queries NULL). */
int oslam_match_results_device(const oslam_matcher_t* h, const int32_t** q_match, const int32_t** q_dist,
                               const int32_t** kp_match, const int32_t** nmatches,
                               const oslam_proj_query_t** queries, const int32_t** n_queries);
int oslam_match_fetch(oslam_matcher_t* h, int b, int q_stride, int n_queries, int kp_stride, int n_kps,
                      int32_t* q_match, int32_t* q_dist, int32_t* kp_match, int32_t* nmatches,
                      int32_t* iterations, void* stream);

/* Host drop-ins (one frame, host buffers in and out). bounds = {mnMinX, mnMinY, mnMaxX, mnMaxY}. */
int oslam_match_search_by_projection(oslam_matcher_t* h, int N, const oslam_keypoint_t* keysUn,
                                     const float* uRight, const uint8_t* desc, const uint8_t* blocked,
                                     const float bounds[4], const oslam_proj_query_t* queries, int M,
                                     float nnratio, int use_ratio, int check_ori, int32_t* q_match,
                                     int32_t* q_dist, int32_t* kp_match, int32_t* nmatches);
int oslam_match_project_last_frame(oslam_matcher_t* h, int N, const oslam_keypoint_t* keysUn, const float* uRight,
                                   const uint8_t* desc, const uint8_t* blocked, const float bounds[4], int Nlast,
                                   const float* Xw, const uint8_t* has_mp, const oslam_keypoint_t* last_keys,
                                   const uint8_t* mp_desc, const float Tcw[16], const float Tlw[16],
                                   const oslam_camera_t* cam, const float* scaleFactors, int nlevels, float th,
                                   int bMono, int check_ori, int32_t* q_match, int32_t* q_dist,
                                   int32_t* kp_match, int32_t* nmatches);
/* Search half of ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:888-947):
 * KeyFrame::GetFeaturesInArea window (src/KeyFrame.cc:569-608), level gate [minLevel, maxLevel] =
 * [nPredictedLevel-1, nPredictedLevel], chi2 reprojection gate (7.8 if mvuRight>=0 else 5.99) with
 * mvInvLevelSigma2, best Hamming <= TH_LOW.  q_match[i] = keypoint to fuse map point i with (or -1).
 * The per-point projection / distance / viewing-angle gates (:851-886) fill the queries and the
 * Replace / AddObservation surgery (:950-970) is applied by the caller in query order. */
int oslam_match_fuse_search(oslam_matcher_t* h, int N, const oslam_keypoint_t* keysUn, const float* uRight,
                            const uint8_t* desc, const float bounds[4], const oslam_proj_query_t* queries, int M,
                            const float* invLevelSigma2, int nlevels, int32_t* q_match, int32_t* q_dist,
                            int32_t* n_fused);
int oslam_match_fuse_batch_device(oslam_matcher_t* h, const oslam_match_frames_t* frames,
                                  const oslam_proj_query_t* d_queries, int q_stride, const int32_t* d_n_queries,
                                  int n_queries_const, int batch, const float* invLevelSigma2, int nlevels,
                                  void* stream);
/* Descriptor pairs compared (256-bit XOR + popcount) by the first pass of the last search over `batch` frames — the work unit of the
 * matching roofline; synchronises the device. */
int oslam_match_hamming_pairs(oslam_matcher_t* h, int batch, int64_t* total);
/* Phase wall-clock counters (100 MHz ticks) of frame 0, profiling builds (-DOSLAM_MATCH_PROFILE); zeros otherwise. */
int oslam_match_debug_counters(oslam_matcher_t* h, long long out[8], int reset);
int oslam_match_debug_get_queries(oslam_matcher_t* h, int b, int q_stride, int n, oslam_proj_query_t* out);

/* ------------------------------------------------------------------------------------------
 * BoW-guided matchers: ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (src/ORBmatcher.cc:159-288)
 * and ORBmatcher::SearchForTriangulation (:657-823).  The DBoW2::FeatureVector of each side (node id -> keypoint indices) is an INPUT
 * (oslam_voc_transform_device + oslam_voc_vectors below build it from a loaded vocabulary).  Side 1 is the flat list the
 * reference iterates (std::map order: node ascending, indices in vector order); side 2 is CSR over its sorted,
 * unique node ids.  Host pointers, one pair per call.
 * SearchByBoW: side1.flag[i] = pKF map point exists && !isBad(); match_f[k] = keyframe keypoint whose map point is
 *   written to vpMapPointMatches[k] (-1 none, -2 removed by the rotation check); nmatches = return value.
 *   The claim order (:211-212: a frame keypoint matched by an earlier keyframe keypoint is skipped) is reproduced.
 * SearchForTriangulation: side1.flag[i] = pKF1->GetMapPoint(i) != NULL (skipped); side2.has_mp likewise;
 *   F12 row-major 3x3 (cv::Mat CV_32F), (ex, ey) = epipole in image 2 (:663-670); match12[i] = keypoint of KF2 or -1.
 *   (vbMatched2 is never set in the reference, :722 — queries are independent and so they are here.)
 * SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (:522-655), what LoopClosing::ComputeSim3 begins with for every
 *   candidate (src/LoopClosing.cc:266, ORBmatcher(0.75, true)): side1.flag[i] = pMP1 && !pMP1->isBad(); side2.has_mp[k] = pMP2 && !pMP2->isBad()
 *   (NULL = none: no candidate, zero matches).  It differs from the (KeyFrame*, Frame&) overload in this: a side-2 keypoint is a candidate only if
 *   has_mp[k] is set and no earlier query, in side-1 list order, has been accepted on it (vbMatched2, :576, set at :603: the sequential claim is
 *   reproduced as above); acceptance is bestDist1 < TH_LOW, strict (:598; <= at :240); the ratio test is (float)bestDist1 < nnratio *
 *   (float)bestDist2; the rotation histogram bins by idx1 with both angles from mvKeysUn; vbMatched2 of a match that the rotation check removes stays
 *   set (nothing reads it afterwards).  match12 [s1.N]: the side-2 keypoint whose map point goes to vpMatches12[idx1], -1 none, -2 removed by the
 *   rotation check; nmatches = the return value (what :268 compares with 20).
 * ---------------------------------------------------------------------------------------- */
typedef struct oslam_bow oslam_bow_t;
typedef struct oslam_bow_side1 {
    int32_t N; const oslam_keypoint_t* keys; const uint8_t* desc; const float* uRight /* NULL = all -1 */; const uint8_t* flag;
    int32_t nq; const int32_t* q_idx; const uint32_t* q_node;
} oslam_bow_side1_t;
typedef struct oslam_bow_side2 {
    int32_t N; const oslam_keypoint_t* keys; const uint8_t* desc; const float* uRight /* NULL = all -1 */; const uint8_t* has_mp /* NULL = none */;
    int32_t nNodes; const uint32_t* nodes; const int32_t* start; const int32_t* items;
} oslam_bow_side2_t;
int oslam_bow_create(oslam_bow_t** out, int max_keypoints /* <= 2400 */, int device);
void oslam_bow_destroy(oslam_bow_t* h);
int oslam_match_search_by_bow(oslam_bow_t* h, const oslam_bow_side1_t* kf, const oslam_bow_side2_t* frame, float nnratio,
                              int checkOri, int32_t* match_f, int32_t* nmatches);
int oslam_match_search_for_triangulation(oslam_bow_t* h, const oslam_bow_side1_t* kf1, const oslam_bow_side2_t* kf2,
                                         const float F12[9], float ex, float ey, const float* scaleFactors,
                                         const float* levelSigma2, int nlevels, int bOnlyStereo, int checkOri,
                                         int32_t* match12, int32_t* nmatches);
int oslam_match_search_by_bow_kf(oslam_bow_t* h, const oslam_bow_side1_t* kf1, const oslam_bow_side2_t* kf2, float nnratio, int checkOri,
                                 int32_t* match12, int32_t* nmatches);

/* Batch of independent pairs, one workgroup each in one launch (the batch-of-sequences layout).  triangulation == 0: SearchByBoW, match
 * [s2.N]; == 2: SearchByBoW(KeyFrame*, KeyFrame*), match [s1.N]; any other value: SearchForTriangulation (bOnlyStereo = false), match [s1.N].
 * nmatches is written per job; jobs of all three modes may share a launch.  oracle/'s operator table knows modes 0 and 1 only: mode 2 is checked
 * against the Python restatement of tests/loop_closing_common.py. */
typedef struct oslam_bow_job {
    oslam_bow_side1_t s1; oslam_bow_side2_t s2;
    int32_t triangulation;
    float nnratio; int32_t checkOri;
    float F12[9]; float ex, ey;
    int32_t* match;
    int32_t nmatches;
} oslam_bow_job_t;
int oslam_match_bow_batch(oslam_bow_t* h, int n, oslam_bow_job_t* jobs, const float* scaleFactors, const float* levelSigma2, int nlevels);
/* The same with device-resident copies of the keypoint (mvKeysUn), descriptor and mvuRight arrays of either side: res[i] members that are NULL fall back to
 * the host arrays of jobs[i] (which are then packed and uploaded as above).  The resident arrays must be complete when the call is made. */
typedef struct oslam_bow_resident {
    const oslam_keypoint_t* d_keys1; const uint8_t* d_desc1; const float* d_uRight1;
    const oslam_keypoint_t* d_keys2; const uint8_t* d_desc2; const float* d_uRight2;
} oslam_bow_resident_t;
int oslam_match_bow_batch_resident(oslam_bow_t* h, int n, oslam_bow_job_t* jobs, const oslam_bow_resident_t* res, const float* scaleFactors,
                                   const float* levelSigma2, int nlevels);

/* ------------------------------------------------------------------------------------------
 * Frame::ComputeStereoMatches (src/Frame.cc:706-880): row-band Hamming search of left keypoints in the
 * right image (levels +-1, u in [uL - bf/b, uL], best < (TH_HIGH+TH_LOW)/2), 11-shift 11x11 SAD on the
 * left keypoint's pyramid level, parabola sub-pixel fit, depth = bf/disparity, rejection of matches
 * with SAD >= 1.5*1.4*median.  Reads the pyramids of the two extractor handles' last batch
 * (mvImagePyramid, include/ORBextractor.h:85).  Outputs mvuRight / mvDepth (-1 = no match).
 * Window reads that would leave the image (unchecked in the reference) are skipped.
 * ---------------------------------------------------------------------------------------- */
typedef struct oslam_stereo oslam_stereo_t;
int oslam_stereo_create(oslam_stereo_t** out, int max_batch, int max_keypoints /* <= 2400; level-0 image height <= 4096 */, int device);
void oslam_stereo_destroy(oslam_stereo_t* h);
int oslam_stereo_match(oslam_stereo_t* h, oslam_orb_t* orbL, oslam_orb_t* orbR, int N, const oslam_keypoint_t* keysL,
                       const uint8_t* descL, int Nr, const oslam_keypoint_t* keysR, const uint8_t* descR, int nlevels,
                       float bf, float b, float* uRight, float* depth);
int oslam_stereo_match_batch_device(oslam_stereo_t* h, oslam_orb_t* orbL, oslam_orb_t* orbR, int batch, int kp_stride,
                                    const oslam_keypoint_t* d_kpL, const uint8_t* d_descL, const int32_t* d_nL,
                                    int nL_const, const oslam_keypoint_t* d_kpR, const uint8_t* d_descR,
                                    const int32_t* d_nR, int nR_const, int nlevels, float bf, float b, void* stream);
/* Device results of the last batch: d_uRight / d_depth [batch][kp_stride] (the stride of that call; entries beyond a pair's left count are
 * unspecified), d_n_matched [batch] = left keypoints that had a match BEFORE the median-SAD cut (the size of vDistIdx, src/Frame.cc:866; the cut then
 * resets some of them to -1), or -1 when the kernel rejected the pair (a negative device count, or one above kp_stride: the pair owns kp_stride rows
 * of the input arrays and of the results); the uRight / depth rows of a rejected pair are not written. */
int oslam_stereo_results_device(const oslam_stereo_t* h, const float** d_uRight, const float** d_depth,
                                const int32_t** d_n_matched);

/* ------------------------------------------------------------------------------------------
 * Optimizer::PoseOptimization — motion-only BA (include/Optimizer.h:46, src/Optimizer.cc:239-451):
 * 4 rounds x optimize(10) of g2o Levenberg-Marquardt on one SE3 vertex, Huber(sqrt(5.991) mono,
 * sqrt(7.815) stereo) dropped after round index 2, chi2 re-classification after every round, every
 * round restarted from the input pose.  State is float32 at the boundary (cv::Mat CV_32F), fp64
 * inside (Converter::toSE3Quat / toCvMat, src/Converter.cc:38-72).
 * Per keypoint i: has_mp[i] = pFrame->mvpMapPoints[i] != NULL, Xw = pMP->GetWorldPos(),
 * obs = (mvKeysUn[i].pt.x, .pt.y, mvuRight[i]) with mvuRight < 0 => monocular edge,
 * invSigma2 = mvInvLevelSigma2[mvKeysUn[i].octave].  K5 = {fx, fy, cx, cy, mbf}.
 * Outputs: pose (pFrame->SetPose), outlier[i] = mvbOutlier[i], n_inliers = return value
 * (nInitialCorrespondences - nBad; 0 and pose untouched if < 3 correspondences).
 * ---------------------------------------------------------------------------------------- */
typedef struct oslam_poseopt oslam_poseopt_t;
int oslam_poseopt_create(oslam_poseopt_t** out, int max_batch, int max_points /* <= 11000 (chi2 + level per edge slot live in LDS) */, int device);
void oslam_poseopt_destroy(oslam_poseopt_t* h);
int oslam_pose_optimize(oslam_poseopt_t* h, int N, const float Tcw_in[16], const float* Xw, const float* obs,
                        const float* invSigma2, const uint8_t* has_mp, const float K5[5], float Tcw_out[16],
                        uint8_t* outlier, int32_t* n_inliers, int32_t stats[2] /* LM iterations, trials; may be NULL */);
/* Test hook: record the Levenberg-Marquardt trials of frame 0 of the calls that follow (cap > 0; cap == 0 stops), and read them back as
 * out[cap][6] = (F before the trial, F of the trial, rho, lambda of the trial, accepted, first trial of a round); *n = trials seen since the last read.  The parity
 * tests compare this sequence with the oracle's (g2o OptimizationAlgorithmLevenberg::solve, replaced at src/Optimizer.cc:407-409). */
int oslam_poseopt_trace(oslam_poseopt_t* h, int cap);
int oslam_poseopt_trace_read(oslam_poseopt_t* h, double* out, int32_t* n);
/* Batch of independent frames in HBM (device pointers, per-frame stride in points). Asynchronous. */
int oslam_pose_optimize_batch_device(oslam_poseopt_t* h, int batch, int stride, const int32_t* d_n, int n_const,
                                     const float* d_Tcw, const float* d_Xw, const float* d_obs,
                                     const float* d_invSigma2, const uint8_t* d_has_mp, const float K5[5],
                                     void* stream);
int oslam_poseopt_results_device(const oslam_poseopt_t* h, const float** d_Tcw_out, const uint8_t** d_outlier,
                                 const int32_t** d_n_inliers, const int32_t** d_stats);

/* ObjectOptimizer::PoseOptimization2 (include/ObjectOptimizer.h:23, src/ObjectOptimizer.cc:624-1240), the
 * pose optimisation Tracking::TrackLocalMap calls (src/Tracking.cc:1022): PoseOptimization plus
 * semantic reprojection edges to the nearest object-mask pixel.  Host pointers.  The object layer
 * (association, out of scope) supplies: the Object2D masks of the matched objects (uint8 {0,255},
 * [nObj][H][W], tight), the world positions of every matched Object3D's map points (object-major),
 * and the M_joint set (:721-726): keypoints whose map point belongs to object joint_obj[j] while
 * mvObjectKpIndices[kp].first != that object.  Nearest pixel = exact NN under FLANN's float squared
 * L2, ties -> first pixel in row-major order.  n_semantic = the reference's nSemNum (:1232). */
typedef struct oslam_semantic {
    int32_t nObj, H, W;
    const uint8_t* masks;
    int32_t nObjMp; const float* objmp_Xw; const int32_t* objmp_obj;
    int32_t nJoint; const int32_t* joint_kp; const int32_t* joint_obj;
    const float* kp_uv;      /* [N][2] mvKeysUn[i].pt */
    float bounds[4];         /* mnMinX, mnMinY, mnMaxX, mnMaxY */
    float invSigma2_0;       /* mvInvLevelSigma2[0] */
} oslam_semantic_t;
int oslam_pose_optimize2(oslam_poseopt_t* h, int N, const float Tcw_in[16], const float* Xw, const float* obs,
                         const float* invSigma2, const uint8_t* has_mp, const float K5[5], const oslam_semantic_t* sem,
                         float Tcw_out[16], uint8_t* outlier, int32_t* n_inliers, int32_t* n_semantic);

/* Batch form (Tracking::TrackLocalMap of several sequences, src/Tracking.cc:1022): device pointers, asynchronous on `stream`.  The base arrays are those
 * of oslam_pose_optimize_batch_device.  Frame b uses masks d_mask_ptrs[obj0 .. obj0 + nObj) (device pointers to uint8 {0,255} images of H x W, rows
 * mask_pitch bytes apart: nothing is copied), object map points objmp0 .. objmp0 + nObjMp of the pools (objmp_obj = object index INSIDE the frame)
 * and M_joint entries joint0 .. joint0 + nJoint; mvKeysUn[kp].pt is read from the frame's obs rows.  n_semantic per frame through
 * oslam_poseopt_semantic_results_device; a frame with fewer than 3 correspondences reports 0. */
typedef struct oslam_sem_frame { int32_t nObj, obj0, nObjMp, objmp0, nJoint, joint0; } oslam_sem_frame_t;
int oslam_pose_optimize2_batch_device(oslam_poseopt_t* h, int batch, int stride, const int32_t* d_n, const float* d_Tcw, const float* d_Xw, const float* d_obs,
                                      const float* d_invSigma2, const uint8_t* d_has_mp, const float K5[5], const oslam_sem_frame_t* d_frames, int total_obj,
                                      const uint8_t* const* d_mask_ptrs, int H, int W, int mask_pitch, int total_objmp, const float* d_objmp_Xw,
                                      const int32_t* d_objmp_obj, int total_joint, const int32_t* d_joint_kp, const int32_t* d_joint_obj, const float bounds[4],
                                      float invSigma2_0, void* stream);
int oslam_poseopt_semantic_results_device(const oslam_poseopt_t* h, const int32_t** d_n_semantic);
/* One-bit-per-pixel form of n instance masks (device pointers, rows `pitch` bytes apart): d_bits [n][H][ceil(W / 64)] uint64, bit i of word w = pixel
 * 64 w + i == 255 (the test of src/Frame.cc:266 and of the pcl cloud at src/ObjectOptimizer.cc:699-710).  One pass over the mask bytes; the keypoint test
 * (oslam_frame_object_kp_test_bits_batch_device, same semantics as the byte form below) and the boundary lists of the next
 * oslam_pose_optimize2_batch_device call (oslam_poseopt_use_mask_bits: pooled object o = bitmap d_bits_index[o]) then read words. */
int oslam_mask_bits_device(const uint8_t* const* d_mask_ptrs, int n, int H, int W, int pitch, uint64_t* d_bits, void* stream);
int oslam_poseopt_use_mask_bits(oslam_poseopt_t* h, const uint64_t* d_bits, const int32_t* d_bits_index);
int oslam_frame_object_kp_test_bits_batch_device(const oslam_keypoint_t* d_keysUn, int kp_stride, const int32_t* d_n_kps, int batch, const uint64_t* d_bits,
                                                 const int32_t* d_mask0, const int32_t* d_n_masks, int H, int W, uint8_t* d_out, void* stream);
/* Frame::BuildObject2DsRGBD / BuildObject2DsStereo keypoint test (src/Frame.cc:262-272, :336-346): bit o of d_out[b][k] is set iff every pixel
 * (int)(kpUn.y + row), (int)(kpUn.x + col), row / col in [-10, 10), of mask d_mask_ptrs[d_mask0[b] + o] equals 255 (a pixel outside the image fails: the
 * reference reads out of bounds there); at most 8 masks per frame.  The depth gate and the sequential assignment (:273-301) stay with the caller. */
int oslam_frame_object_kp_test_batch_device(const oslam_keypoint_t* d_keysUn, int kp_stride, const int32_t* d_n_kps, int batch, const uint8_t* const* d_mask_ptrs,
                                            const int32_t* d_mask0, const int32_t* d_n_masks, int H, int W, int mask_pitch, uint8_t* d_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer::LocalBundleAdjustment (include/Optimizer.h:45, src/Optimizer.cc:453-778) after the
 * covisibility gather (:456-504, pointer-graph walk, stays with the caller):
 * g2o Levenberg-Marquardt + BlockSolver_6_3 Schur complement, optimize(5) with Huber, chi2 (5.991 /
 * 7.815) and depth gating (:672-702), optimize(10) without robust kernel, erase list (:711-743).
 * poses [nKF][16] Tcw float32; fixed[k]: 0 local keyframe (free), 1 fixed camera (lFixedCameras),
 * 2 local keyframe with mnId==0 (setFixed(true) at :529 yet written back at :762-768);
 * points [nP][3]; one edge per observation: (keyframe, point, kpUn.pt.x, kpUn.pt.y, mvuRight (<0 mono),
 * mvInvLevelSigma2[octave]).  K5 = {fx, fy, cx, cy, mbf}.
 * Outputs: poses / points rounded to float32 like Converter::toCvMat, erase[e] = 1 for observations
 * the reference erases.  pbStopFlag (:517-518): oslam_lba_stop_flag() returns a pinned, device-visible
 * int the caller may set from another thread (LocalMapping::InterruptBA, src/LocalMapping.cc:628-631);
 * it is polled at the points g2o polls its force-stop flag when use_stop_flag != 0.
 * ---------------------------------------------------------------------------------------- */
typedef struct oslam_lba oslam_lba_t;
int oslam_lba_create(oslam_lba_t** out, int max_batch, int max_keyframes /* per window, fixed cameras included; at most 128 of them free */, int max_points,
                     int max_edges, int device);
void oslam_lba_destroy(oslam_lba_t* h);
volatile int32_t* oslam_lba_stop_flag(oslam_lba_t* h);
/* 1 (default): a single problem is spread over the whole GPU (multi-kernel LM, device-side control);
 * 2: one workgroup per problem, the whole LM schedule in ONE launch with the reduced camera system resident in LDS (the batch-of-windows layout of the
 *    driver; a window whose reduced system and poses exceed the CU's LDS — roughly 30 free keyframes — runs in mode 1 beside the others);
 * 0: the round-1 one-workgroup-per-problem kernel (reduced system in global memory), kept as an A/B layout.  Same arithmetic in all three. */
int oslam_lba_set_mode(oslam_lba_t* h, int wide);
/* Schur complement of mode 1: 0 = gather, per pair of a 6x6 block, of the two 32-byte edge records plus the landmark's 48-byte inverse (one wavefront per block), 1 = on chip by tiles of points staged in LDS (one
 * coalesced read of the per-edge blocks per trial), 2 = chosen per call from the mean window size.  Same results to rounding.  The pair lists of mode 0 (the
 * default) are built on the device once per call (k_w_pair_*); 3 = mode 0 with the lists built by the host (the round-2 path): bit-identical results. */
int oslam_lba_set_schur(oslam_lba_t* h, int mode);
/* Kernel timing for bench.py's roofline: HIP events on the handle's stream around the solve kernels of every later call.
 * Returns and clears the accumulated milliseconds / kernel launches, then sets the switch to `enable`. */
int oslam_lba_kernel_time(oslam_lba_t* h, int enable, double* ms_out, long long* launches_out);
/* Test hook, as oslam_poseopt_trace: the LM trials of window 0 of the wide-mode calls that follow (g2o's OptimizationAlgorithmLevenberg::solve as
 * driven from src/Optimizer.cc:659-660,706-707); field 5 = first trial of a stage.  Process-wide: one handle traces at a time. */
int oslam_lba_trace(oslam_lba_t* h, int cap);
int oslam_lba_trace_read(oslam_lba_t* h, double* out, int32_t* n);
/* Reduced-camera-system solver of the wide mode: 0 (default) = the LDS-resident scalar kernel when EVERY system of the call has at most 132 unknowns
 * (6 x free keyframes), otherwise matrix cores (v_mfma_f64_16x16x4_f64 trailing updates, 16-wide panels): with the system resident in LDS up to 186 unknowns
 * (k_w_chol_lds_mfma: the windows of the driver's steady state), in global memory beyond; 1 = the global-memory matrix-core kernel for every size; 2 = no
 * matrix cores; 3 = the round-3 choice (scalar packed LDS kernel up to 192 unknowns, global-memory matrix cores beyond), kept as an A/B. */
int oslam_lba_set_solver(oslam_lba_t* h, int mode);
int oslam_lba_debug_stats(oslam_lba_t* h, int32_t out[16]);   /* [0..3] stats, [8..15] per-phase kilo-cycles in profiling builds */
int oslam_lba_optimize(oslam_lba_t* h, int nKF, const float* poses, const uint8_t* fixed, int nP,
                       const float* points, int nE, const int32_t* edge_kf, const int32_t* edge_pt,
                       const float* edge_obs, const float* edge_invSigma2, const float K5[5], int use_stop_flag,
                       float* poses_out, float* points_out, uint8_t* erase,
                       int32_t stats[4] /* iterations/trials of stage 1 and 2; may be NULL */);

/* Batch of independent local-BA problems (one workgroup each, ONE launch): the batch-of-sequences layout. */
typedef struct oslam_lba_problem {
    int32_t nKF; const float* poses; const uint8_t* fixed;
    int32_t nP; const float* points;
    int32_t nE; const int32_t* edge_kf; const int32_t* edge_pt; const float* edge_obs; const float* edge_invSigma2;
    float* poses_out; float* points_out; uint8_t* erase; int32_t* stats;   /* stats may be NULL */
} oslam_lba_problem_t;
/* A window of the batch that the solver refuses (an index out of range, a duplicate observation, more free keyframes than the bound ...) fails ALONE when it has
 * a stats array: stats = {-1, OSLAM_E_* code, 0, 0}, poses_out / points_out = the inputs, erase = 0, and the other windows are solved (return value OSLAM_OK).
 * Without a stats array such a window fails the call, as in rounds 1-4. */
int oslam_lba_optimize_batch(oslam_lba_t* h, int n, const oslam_lba_problem_t* probs, const float K5[5]);

/* Optimizer::BundleAdjustment (include/Optimizer.h:38, src/Optimizer.cc:49-237) on the same flattened graph:
 * one optimize(nIterations), Huber sqrt(5.99) / sqrt(7.815) only if bRobust, no gating, no erase list.
 * fixed[k] = 1 for the keyframe with mnId == 0 (:79). */
int oslam_ba_optimize(oslam_lba_t* h, int nKF, const float* poses, const uint8_t* fixed, int nP, const float* points, int nE,
                      const int32_t* edge_kf, const int32_t* edge_pt, const float* edge_obs, const float* edge_invSigma2,
                      const float K5[5], int nIterations, int bRobust, int use_stop_flag, float* poses_out, float* points_out);

/* ---------------- MapPoint maintenance + Frame::isInFrustum ----------------
 * Batched over map points. Observations of point p are rows obs_start[p] .. obs_start[p+1]-1 of the obs_* tables,
 * in the iteration order of the reference's std::map<KeyFrame*,size_t> (the caller keeps that order). */
typedef struct oslam_mappoint oslam_mappoint_t;
int oslam_mappoint_create(oslam_mappoint_t** out, int device);
void oslam_mappoint_destroy(oslam_mappoint_t* h);
/* Device time of the batched SearchByBoW / SearchForTriangulation kernel (oslam_match_bow_batch) and of the batched triangulation kernel
 * (oslam_mp_triangulate_pairs), HIP events on the handles' own streams: what accumulated since the last call, then the switch is set to `enable`. */
int oslam_bow_kernel_time(oslam_bow_t* h, int enable, double* ms_out, long long* launches_out);
int oslam_mappoint_kernel_time(oslam_mappoint_t* h, int enable, double* ms_out, long long* launches_out);

/* MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:345-410): for each point the observation whose
 * median Hamming distance to the others (sorted row, element int(0.5*(N-1))) is the first strict minimum.
 * best_idx[p] = index inside the point's list (-1 if it has no observation; out_desc row then zero). */
int oslam_mp_distinctive_descriptors(oslam_mappoint_t* h, int P, const int32_t* obs_start, const uint8_t* obs_desc /*[total][32]*/,
                                     int32_t* best_idx /*[P]*/, uint8_t* out_desc /*[P][32]*/);

/* MapPoint::UpdateNormalAndDepth (reference src/MapPoint.cc:433-474). obs_Ow = camera centres of the observing
 * keyframes, OwRef = reference keyframe centre, levelScaleFactor[p] = mvScaleFactors[level of the point in the
 * reference keyframe], lastScaleFactor = mvScaleFactors[nLevels-1].
 * out[p] = {normal.x, normal.y, normal.z, mfMaxDistance, mfMinDistance}. */
int oslam_mp_update_normal_depth(oslam_mappoint_t* h, int P, const float* Pos /*[P][3]*/, const int32_t* obs_start, const float* obs_Ow /*[total][3]*/,
                                 const float* OwRef /*[P][3]*/, const float* levelScaleFactor /*[P]*/, float lastScaleFactor, float* out /*[P][5]*/);

/* Resident map-point table: d_tab[slot] = device array of 64-byte records indexed by map-point id — float pos[3], normal[3], minDistance, maxDistance, then the
 * 32 descriptor bytes (mWorldPos, mNormalVector, mfMinDistance, mfMaxDistance, mDescriptor of include/MapPoint.h:116-141).  After a MapPoint update of P points
 * (the two functions below) this writes its results into the records d_items[i] = (slot, id): position (d_Pos) + normal / distances (d_out5) when do_normal,
 * the descriptor when do_desc and the point's descriptor list (d_desc_start) is not empty; a point without observations (culled) keeps its record except
 * for the position, which the caller may have changed before culling it (local BA). */
/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:345-430) and / or UpdateNormalAndDepth (:432-474) for P points in ONE launch, for the driver's small
 * updates: the descriptors of the observations are read from resident keyframe records (d_rec = (record, keypoint) per entry of the descriptor list d_desc_start,
 * d_rec_desc[record] = that keyframe's descriptor array), the results go to o_best / o_desc / o_out5 — any device-accessible memory, e.g. pinned host memory — and,
 * with d_tab, into the points' resident records like oslam_mp_table_write_device.  Same results as the separate functions.  At most 128 observations per point:
 * a point with a longer descriptor list gets o_best = -2 and no descriptor (neither in o_desc nor in its record) — use oslam_mp_distinctive_descriptors for it. */
int oslam_mp_update_fused_device(int P, int do_desc, int do_normal, const int32_t* d_obs_start, const int32_t* d_desc_start, const int32_t* d_rec, const uint8_t* const* d_rec_desc,
                                 const float* d_obs_Ow, const float* d_Pos, const float* d_OwRef, const float* d_lsf, float lastScale, const int32_t* d_items, uint8_t* const* d_tab,
                                 int32_t* o_best, uint8_t* o_desc, float* o_out5, void* stream);
/* MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:432-474) for P points of solved local-BA windows, as Optimizer::LocalBundleAdjustment's write-back calls it
 * per point (src/Optimizer.cc:769-776), from the windows' own arrays (include/oslam_slam.h oslam_job_mp_window_t, flattened over the windows of a call): point j
 * has the edges d_e0[j] .. d_e0[j] + d_ne[j] of d_edge_kf / d_erase (window keyframe index, erased flag), its window's camera centres start at row d_kbase[j] of
 * d_Ow, d_ref[j] = window index of its reference keyframe, d_lsf[j] = that observation's level scale factor, d_skip[j] != 0 = position only.  Results as
 * oslam_mp_update_normal_depth in d_out5; with d_tab the resident records (d_items[2 j], d_items[2 j + 1]) are updated in the same pass. */
int oslam_mp_update_windows_device(int P, const int32_t* d_items, uint8_t* const* d_tab, const int32_t* d_e0, const int32_t* d_ne, const int32_t* d_kbase, const int32_t* d_ref,
                                   const float* d_lsf, const uint8_t* d_skip, const float* d_Pos, const int32_t* d_edge_kf, const uint8_t* d_erase, const float* d_Ow, float lastScale,
                                   float* d_out5, void* stream);
int oslam_mp_table_write_device(int P, const int32_t* d_items, uint8_t* const* d_tab, const int32_t* d_obs_start, const int32_t* d_desc_start, const float* d_Pos,
                                const float* d_out5, const uint8_t* d_out_desc, int do_desc, int do_normal, void* stream);
/* Inputs of Optimizer::PoseOptimization (src/Optimizer.cc:258-340) for a batch of frames that are still on the device: frame b is frame d_slots[b] of the
 * keypoint arrays d_keysUn / d_uRight ([.][kp_stride]) with d_n[b] keypoints; d_ids[b][i] = map point of keypoint i (record of d_tab[d_slots[b]]) or -1.
 * Writes Xw, obs = (x, y, uRight), invSigma2 = invLevelSigma2[octave] and has_mp in the [batch][stride] layout of oslam_pose_optimize_batch_device. */
int oslam_pose_inputs_gather_device(int batch, int stride, const int32_t* d_slots, const int32_t* d_n, const int32_t* d_ids, uint8_t* const* d_tab,
                                    const oslam_keypoint_t* d_keysUn, const float* d_uRight, int kp_stride, const float* invLevelSigma2, int nLevels,
                                    float* d_Xw, float* d_obs, float* d_invSigma2, uint8_t* d_has_mp, void* stream);
/* Position and descriptor of the map points d_ids[b][i] (records of d_tab[b]; -1 = none: zeros) into the [batch][stride] arrays that
 * oslam_match_project_last_batch_device reads (the last frame's mvpMapPoints of ORBmatcher::SearchByProjection(Cur, Last), src/ORBmatcher.cc:1338-1366). */
/* The projection gates of ORBmatcher::Fuse (src/ORBmatcher.cc:840-890) for n (keyframe, candidate list) jobs from the resident map-point records: job b has
 * d_M[b] candidates d_ids[b][i] (records of d_tab[d_slots[b]]; excluded when d_ids < 0 or d_excl != 0), keyframe pose d_Tcw[b] / centre d_Ow[b]; writes the
 * query of every candidate (inactive = flags 0) in candidate order into d_q[b][.] for oslam_match_fuse_batch_device. */
int oslam_fuse_queries_device(int n, int stride, const int32_t* d_slots, const int32_t* d_M, const int32_t* d_ids, const uint8_t* d_excl, uint8_t* const* d_tab,
                              const float* d_Tcw, const float* d_Ow, const float K5[5], const float bounds[4], float th, float logScaleFactor,
                              const float* scaleFactors, int nLevels, oslam_proj_query_t* d_q, void* stream);
/* Fuse against RESIDENT keyframes.  KeyFrame::mGrid is fixed at construction (src/KeyFrame.cc:44-52), so the grid of a registered keyframe is built ONCE:
 * oslam_kf_grid_build_device sorts the keypoints of job i (the d_counts[slot] keypoints at `keys` / `uRight`) by cell — cells in the (x, y) nesting of
 * Frame::mGrid, index order inside a cell (src/Frame.cc:455-470) — into cell_end[3072] (end of every cell in the sorted list) and cand[N][4] =
 * (x, y, uRight, bit pattern of octave << 16 | keypoint index).  *d_status is set to 1 if a count exceeds max_keypoints (never truncated silently).
 * oslam_fuse_search_device = oslam_fuse_queries_device + the window search of ORBmatcher::Fuse (src/ORBmatcher.cc:890-947: GetFeaturesInArea, level gate,
 * chi2 gates, best Hamming distance <= TH_LOW) with one candidate per thread, straight from those arrays: d_q_match[b][i] = keypoint index or -1, the same
 * values oslam_match_fuse_batch_device returns for the queries of oslam_fuse_queries_device (tests/test_mp_table_gpu.py). */
typedef struct oslam_kf_grid_job { const oslam_keypoint_t* keys; const float* uRight; uint16_t* cell_end; float* cand; int32_t slot; int32_t pad_; } oslam_kf_grid_job_t;
typedef struct oslam_kf_grid_ref { const uint16_t* cell_end; const float* cand; const uint8_t* desc; } oslam_kf_grid_ref_t;
int oslam_kf_grid_build_device(int n, const oslam_kf_grid_job_t* d_jobs, const int32_t* d_counts, const float bounds[4], int max_keypoints, int32_t* d_status, void* stream);
int oslam_fuse_search_device(int n, int stride, const oslam_kf_grid_ref_t* d_kfs, const int32_t* d_slots, const int32_t* d_M, const int32_t* d_ids, const uint8_t* d_excl,
                             uint8_t* const* d_tab, const float* d_Tcw, const float* d_Ow, const float K5[5], const float bounds[4], float th, float logScaleFactor,
                             const float* scaleFactors, const float* invLevelSigma2, int nLevels, int32_t* d_q_match, void* stream);
/* The arrays of Tracking::SearchLocalPoints for n frames from the resident records: job i = {slot, M, byte offset of its ids (int32 [M]) and of its
 * Observations() > 0 flags (uint8 [M]) inside d_stage}; writes position, normal, distances, flags and descriptor of every point into the [.][stride] arrays
 * at row `slot` (the layout oslam_frame_is_in_frustum_batch_resident_device reads). */
typedef struct oslam_local_gather { int32_t slot, M; uint32_t ids_off, obs_off; } oslam_local_gather_t;
int oslam_mp_table_local_gather_device(int n, int maxM, const oslam_local_gather_t* d_jobs, const uint8_t* d_stage, uint8_t* const* d_tab, int stride, float* d_Pw,
                                       float* d_Pn, float* d_maxDist, float* d_minDist, uint8_t* d_obs_gt0, uint8_t* d_mp_desc, void* stream);
/* Positions of n map points named by (d_slots[i], d_ids[i]) into d_Xw[n][3] (the object map points of ObjectOptimizer::PoseOptimization2). */
int oslam_mp_table_positions_device(int n, const int32_t* d_slots, const int32_t* d_ids, uint8_t* const* d_tab, float* d_Xw, void* stream);
int oslam_mp_table_gather_device(int batch, int stride, const int32_t* d_n, const int32_t* d_ids, uint8_t* const* d_tab, float* d_Xw, uint8_t* d_desc, void* stream);
/* device-pointer forms (asynchronous on `stream`); d_out_desc rows of points without observations are left untouched (zero-fill them first), their
 * d_best_idx is -1 and their d_out row is five zeros.  Nothing outside d_best_idx [P], d_out_desc [P][32] and d_out [P][5] is written. */
int oslam_mp_distinctive_descriptors_device(int P, const int32_t* d_obs_start, const uint8_t* d_obs_desc, int32_t* d_best_idx, uint8_t* d_out_desc, void* stream);
int oslam_mp_update_normal_depth_device(int P, const float* d_Pos, const int32_t* d_obs_start, const float* d_obs_Ow, const float* d_OwRef,
                                        const float* d_levelScaleFactor, float lastScaleFactor, float* d_out, void* stream);

/* Frame::isInFrustum (reference src/Frame.cc:509-565) + MapPoint::PredictScale (src/MapPoint.cc:505-521) + the window
 * radius of ORBmatcher::SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:57-67, RadiusByViewingCos :93-99),
 * for M map points against one frame pose. Tcw row-major 4x4; K5 = fx,fy,cx,cy,bf; bounds = mnMinX,mnMinY,mnMaxX,mnMaxY;
 * maxDist/minDist = the raw mfMaxDistance/mfMinDistance (the 1.2/0.8 invariance factors are applied inside);
 * obs_gt0[i] = pMP->Observations() > 0. Writes one oslam_proj_query_t per point, ready for
 * oslam_match_search_by_projection: flags bit0 = mbTrackInView, bit1 = obs>0, angle = mTrackViewCos,
 * minLevel = nPredictedLevel-1, maxLevel = nPredictedLevel, desc = the point's descriptor. Points outside the frustum get flags=0. */
int oslam_frame_is_in_frustum(oslam_mappoint_t* h, int M, const float* Pw /*[M][3]*/, const float* Pn /*[M][3]*/, const float* maxDist, const float* minDist,
                              const uint8_t* obs_gt0, const uint8_t* mp_desc /*[M][32]*/, const float Tcw[16], const float K5[5], const float bounds[4],
                              float viewingCosLimit, float logScaleFactor, const float* scaleFactors, int nLevels, float th, oslam_proj_query_t* out);
/* same, all per-point arrays and the output in device memory, asynchronous on `stream` (hipStream_t) */
int oslam_frame_is_in_frustum_device(int M, const float* d_Pw, const float* d_Pn, const float* d_maxDist, const float* d_minDist, const uint8_t* d_obs_gt0,
                                     const uint8_t* d_mp_desc, const float Tcw[16], const float K5[5], const float bounds[4], float viewingCosLimit,
                                     float logScaleFactor, const float* scaleFactors, int nLevels, float th, oslam_proj_query_t* d_out, void* stream);

/* batch of frames (Tracking::SearchLocalPoints for several sequences): per-point arrays [batch][stride], d_M[b] points of frame b are
 * tested against pose d_Tcw[b] (16 floats) with radius factor d_th[b]; d_out [batch][stride] feeds oslam_match_search_batch_device
 * (q_stride = stride); d_in_view [batch][stride] = mbTrackInView (may be NULL).  Entries i >= d_M[b] of d_out and d_in_view are left untouched
 * (pass d_M as d_n_queries of the search: it never reads them). */
int oslam_frame_is_in_frustum_batch_device(int batch, int stride, const int32_t* d_M, const float* d_Pw, const float* d_Pn, const float* d_maxDist,
                                           const float* d_minDist, const uint8_t* d_obs_gt0, const uint8_t* d_mp_desc, const float* d_Tcw, const float* d_th,
                                           const float K5[5], const float bounds[4], float viewingCosLimit, float logScaleFactor, const float* scaleFactors,
                                           int nLevels, oslam_proj_query_t* d_out, uint8_t* d_in_view, void* stream);

/* same with the per-point arrays at their own stride ([batch][stride_in], a table that keeps the local points of every sequence resident) while the
 * queries, in_view and the optional skip flags are [batch][stride_out], stride_out <= stride_in.  d_skip[b][i] != 0: point i of frame b already carries
 * mnLastFrameSeen == the frame's id and is not projected (src/Tracking.cc:1413-1427): inactive query, in_view 0. */
int oslam_frame_is_in_frustum_batch_resident_device(int batch, int stride_in, int stride_out, const int32_t* d_M, const float* d_Pw, const float* d_Pn,
                                                    const float* d_maxDist, const float* d_minDist, const uint8_t* d_obs_gt0, const uint8_t* d_mp_desc,
                                                    const uint8_t* d_skip, const float* d_Tcw, const float* d_th, const float K5[5], const float bounds[4],
                                                    float viewingCosLimit, float logScaleFactor, const float* scaleFactors, int nLevels,
                                                    oslam_proj_query_t* d_out, uint8_t* d_in_view, void* stream);

/* LocalMapping::CreateNewMapPoints, per-match numeric core (reference src/LocalMapping.cc:291-432):
 * parallax test, 4x4 DLT by cv::SVD (one-sided Jacobi) or KeyFrame::UnprojectStereo (src/KeyFrame.cc:615-631),
 * cheirality, chi2 reprojection gates (5.991 / 7.8 x sigma2[octave]; the second view uses the CURRENT keyframe's mbf
 * like the reference, :399) and the scale-consistency gate.  kf1 = mpCurrentKeyFrame, kf2[p] = the neighbours that
 * passed the baseline test (:246-263), matches of pair p = rows pair_start[p] .. pair_start[p+1]-1 of idx1/idx2
 * (SearchForTriangulation output order).  Map insertion (:408-430) stays with the caller. */
typedef struct oslam_tri_kf {
    float Tcw[16];   /* row-major 4x4: GetRotation / GetTranslation */
    float Twc[16];   /* row-major 4x4: Rwc = Rcw.t(), column 3 = GetCameraCenter */
    float fx, fy, cx, cy, invfx, invfy, mbf, mb;
    const oslam_keypoint_t* keysUn;   /* mvKeysUn */
    const oslam_keypoint_t* keys;     /* mvKeys (UnprojectStereo reads the raw keypoint) */
    const float* uRight;              /* mvuRight */
    const float* depth;               /* mvDepth */
    int32_t n_kps;
} oslam_tri_kf_t;
int oslam_mp_triangulate(oslam_mappoint_t* h, const oslam_tri_kf_t* kf1, int nPairs, const oslam_tri_kf_t* kf2, const int32_t* pair_start,
                         const int32_t* idx1, const int32_t* idx2, const float* scaleFactors, const float* levelSigma2, int nLevels,
                         float ratioFactor /* 1.5f*mfScaleFactor */, uint8_t* ok /*[M]*/, float* x3D /*[M][3]*/, int32_t* nnew);

/* Same numeric core for nPairs independent (current keyframe, neighbour) pairs, e.g. one pair per sequence of a batch: pair p = (kf1[p], kf2[p]).  Host
 * pointers, synchronous (the handle's own stream).  ok [M] and x3D [M][3] with M = pair_start[nPairs] are written, x3D = 0 where ok = 0; a pair may be empty. */
int oslam_mp_triangulate_pairs(oslam_mappoint_t* h, int nPairs, const oslam_tri_kf_t* kf1, const oslam_tri_kf_t* kf2, const int32_t* pair_start,
                               const int32_t* idx1, const int32_t* idx2, const float* scaleFactors, const float* levelSigma2, int nLevels,
                               float ratioFactor, uint8_t* ok /*[M]*/, float* x3D /*[M][3]*/);

/* ---------------- Frame construction between the extractor and the grid / matchers ----------------
 * Frame::UndistortKeyPoints (reference src/Frame.cc:644-675: cv::undistortPoints(mat, mat, mK, mDistCoef, Mat(), mK), OpenCV 3.2
 * cvUndistortPoints: fp64, 5 fixed-point iterations), Frame::ComputeImageBounds (:677-704) and Frame::ComputeStereoFromRGBD
 * (:883-904).  K4 = fx, fy, cx, cy (mK, CV_32F); dist = mDistCoef (k1, k2, p1, p2[, k3]; ndist 0 or dist[0] == 0 -> mvKeysUn = mvKeys,
 * bounds = the image rectangle).  The *_batch_device forms work on the extractor's device arrays ([batch][stride] keypoints,
 * counts per frame or n_const) and are asynchronous on `stream`; `image_stride` of the depth batch is in floats.
 * oslam_frame_undistort_batch_device leaves the slots i >= count of a row untouched; the oslam_frame_stereo_from_rgbd_batch* forms write the whole
 * [batch][stride] block of d_uRight / d_mvDepth, -1 in the slots i >= count.  *d_status is OR-ed with 1 when a keypoint lies outside the depth image
 * (the caller zeroes it first; 0 afterwards = every keypoint was inside). */
typedef struct oslam_frame oslam_frame_t;
int oslam_frame_create(oslam_frame_t** out, int device);
void oslam_frame_destroy(oslam_frame_t* h);
int oslam_frame_undistort_keypoints(oslam_frame_t* h, int n, const oslam_keypoint_t* keys, const float K4[4], const float* dist, int ndist,
                                    oslam_keypoint_t* keysUn);
int oslam_frame_undistort_batch_device(const oslam_keypoint_t* d_keys, oslam_keypoint_t* d_keysUn, const int32_t* d_counts, int n_const, int stride,
                                       int batch, const float K4[4], const float* dist, int ndist, void* stream);
/* bounds = mnMinX, mnMinY, mnMaxX, mnMaxY (the order every matcher entry point takes) */
int oslam_frame_image_bounds(oslam_frame_t* h, int cols, int rows, const float K4[4], const float* dist, int ndist, float bounds[4]);
/* depth = imDepth after the mDepthMapFactor scaling (CV_32F, `pitch` floats per row); keys = mvKeys (raw pixel, truncated to
 * the depth pixel like Mat::at<float>(v,u)), keysUn = mvKeysUn; uRight / mvDepth = -1 where depth <= 0.  A keypoint outside the
 * depth image is an error (the reference would read out of bounds). */
int oslam_frame_stereo_from_rgbd(oslam_frame_t* h, int n, const oslam_keypoint_t* keys, const oslam_keypoint_t* keysUn, const float* depth, int rows,
                                 int cols, int pitch, float mbf, float* uRight, float* mvDepth);
/* n images given by a table of device pointers (rows src_pitch bytes apart) gathered into one contiguous batch [n][rows][dst_pitch]: the extractor's input
 * layout, in one launch.  Only the first row_bytes bytes of a destination row are written (the padding up to dst_pitch and between images is left as it was). */
int oslam_frame_gather_images_device(const void* const* d_src_ptrs, int n, int src_pitch, int row_bytes, int rows, void* d_dst, size_t dst_image_stride, int dst_pitch,
                                     void* stream);
/* Device-to-device helpers of the driver's resident keyframe store: n segments {const void* src; void* dst; uint32 bytes; uint32 pad} copied in one launch;
 * d_out[i] = the 32-byte descriptor number d_rec[i][1] of the array d_desc_base[d_rec[i][0]] (d_rec is int32 [n][2]; d_out and the descriptor arrays 4-byte
 * aligned).  Segments may have any byte count (0 included) and any alignment; exactly `bytes` bytes are written per segment. */
int oslam_copy_segments_device(const void* d_segs, int n, void* stream);
int oslam_gather_descriptors_device(const uint8_t* const* d_desc_base, const int32_t* d_rec, int n, uint8_t* d_out, void* stream);
int oslam_frame_stereo_from_rgbd_batch_device(const oslam_keypoint_t* d_keys, const oslam_keypoint_t* d_keysUn, const int32_t* d_counts, int n_const,
                                              int stride, int batch, const float* d_depth, int rows, int cols, int pitch, size_t image_stride,
                                              float mbf, float* d_uRight, float* d_mvDepth, int32_t* d_status, void* stream);

/* Frame::ComputeStereoFromRGBD with the depth images where they are: image b = d_depth_ptrs[b] (device table of device pointers), rows `pitch` floats apart. */
int oslam_frame_stereo_from_rgbd_batch_ptrs_device(const oslam_keypoint_t* d_keys, const oslam_keypoint_t* d_keysUn, const int32_t* d_counts, int n_const,
                                                   int stride, int batch, const float* const* d_depth_ptrs, int rows, int cols, int pitch, float mbf,
                                                   float* d_uRight, float* d_mvDepth, int32_t* d_status, void* stream);

/* The same on RAW 16-bit depth images (what System::TrackRGBD receives, include/System.h:75): a value is scaled on lookup by depth_factor = mDepthMapFactor
 * as imDepth.convertTo(CV_32F, mDepthMapFactor) scales the whole image (reference src/Tracking.cc:98-102,262): (float)d16 * depth_factor in float arithmetic. */
int oslam_frame_stereo_from_rgbd_batch_ptrs_u16_device(const oslam_keypoint_t* d_keys, const oslam_keypoint_t* d_keysUn, const int32_t* d_counts, int n_const,
                                                       int stride, int batch, const uint16_t* const* d_depth16_ptrs, int rows, int cols, int pitch, float depth_factor,
                                                       float mbf, float* d_uRight, float* d_mvDepth, int32_t* d_status, void* stream);

/* Two-level nearest-centre descent over 256-bit descriptors (the node assignment of a DBoW2-style vocabulary tree with branching 10, depth 2):
 * d_out[i][k] = 11 + 10 b1 + b2 for descriptor k of array d_desc_ptrs[i] (d_counts[i] of them, at most `stride`), first minimum on ties. */
int oslam_bow_nodes_device(const uint8_t* const* d_desc_ptrs, const int32_t* d_counts, int n, int stride, const uint64_t* d_top, const uint64_t* d_sub,
                           uint32_t* d_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * ORB vocabulary: the DBoW2 tree the reference loads with mpVocabulary->loadFromTextFile (src/System.cc:64-76) and applies with
 * mpORBvocabulary->transform(desc, mBowVec, mFeatVec, 4) (src/Frame.cc:635-642, src/KeyFrame.cc:59-68, src/ObjectTypes.cc:27-32).
 * DBoW2 is not in the reference tree; format and algorithms are restated from its published TemplatedVocabulary (ORB-SLAM2 fork,
 * FORB: 32-byte descriptors, Hamming distance).  Parity with DBoW2 itself is not pinned by a test.
 * Text format: line 1 `k L scoring weighting` (0 <= k <= 20, 1 <= L <= 10, scoring 0 L1_NORM 1 L2_NORM 2 CHI_SQUARE 3 KL 4 BHATTACHARYYA
 *   5 DOT_PRODUCT, weighting 0 TF_IDF 1 TF 2 IDF 3 BINARY); node 0 is the root and has no line; file line i + 1 is node id i:
 *   `parent_id is_leaf b0 .. b31 weight`, appended to the children of parent_id in file order; a line with is_leaf > 0 is a word whose id is the
 *   number of leaf lines before it.  Trees may be irregular.  Refused with OSLAM_E_INVALID and a message that names the file line: a short or
 *   over-long line, parent_id that is not an earlier node, a byte outside 0..255, an inner node without children, a leaf with children, more
 *   than k children, no node line.  Blank lines at the end of the file are ignored.
 * transform of one descriptor (levelsup): from the root, repeatedly the child at the smallest Hamming distance — children in file order, first
 *   minimum — until a leaf: word id and weight of that leaf; node id = the node passed at depth L - levelsup (0, the root, when that is <= 0).
 *   Normalisation: when the leaf lies above that depth DBoW2 leaves the node id unset; here it is the leaf's own node id.
 * ---------------------------------------------------------------------------------------- */
typedef struct oslam_voc oslam_voc_t;
/* Host only.  oslam_voc_create takes the same tree from arrays: entry j describes node id j + 1 (n_nodes excludes the root). */
int oslam_voc_load_text(oslam_voc_t** out, const char* path);
int oslam_voc_create(oslam_voc_t** out, int k, int L, int scoring, int weighting, int n_nodes, const int32_t* parent, const uint8_t* is_leaf,
                     const uint8_t* desc /* [n_nodes][32] */, const double* weight);
void oslam_voc_destroy(oslam_voc_t* voc);
/* out = k, L, scoring, weighting, nodes (without the root), words, depth of the deepest node, most children of one node */
int oslam_voc_info(const oslam_voc_t* voc, int32_t out[8]);
/* The nodes as they were read, by node id - 1 (any pointer may be NULL); word_id = -1 for inner nodes. */
int oslam_voc_get_nodes(const oslam_voc_t* voc, int32_t* parent, uint8_t* is_leaf, uint8_t* desc, double* weight, int32_t* word_id);
/* Copies the tree to `device` (centres of one node's children contiguous, breadth first).  oslam_voc_transform_device does it at its first call on a
 * device otherwise — that call then allocates and synchronises. */
int oslam_voc_upload(const oslam_voc_t* voc, int device);
/* transform of the descriptors of n arrays on the current device, in the batch layout of oslam_bow_nodes_device: array i = d_desc_ptrs[i] with
 * d_counts[i] <= stride descriptors; outputs [n][stride] (entries beyond a count are not written; any output may be NULL, not all).  A gfx950
 * kernel: 16 lanes per descriptor, one child centre per lane, DPP row minimum, top levels of the tree in LDS. */
int oslam_voc_transform_device(const oslam_voc_t* voc, const uint8_t* const* d_desc_ptrs, const int32_t* d_counts, int n, int stride, int levelsup,
                               uint32_t* d_word, uint32_t* d_node, double* d_weight, void* stream);
/* The same for ONE host array desc [n][32] with host outputs (any may be NULL): upload, the kernel above, download, synchronous.  Calls on one vocabulary
 * are serialised. */
int oslam_voc_transform(const oslam_voc_t* voc, const uint8_t* desc, int n, int levelsup, uint32_t* word, uint32_t* node, double* weight);
/* The same descent on the host for n descriptors desc [n][32].  Not a fallback of the call above (which fails without a device): it is what the
 * tracking driver uses over an operator table that has no device, and for the rare frames whose Frame::ComputeBoW runs on the host. */
int oslam_voc_transform_host(const oslam_voc_t* voc, const uint8_t* desc, int n, int levelsup, uint32_t* word, uint32_t* node, double* weight);
/* transform(features, BowVector&, FeatureVector&, levelsup) from the per-feature outputs of one feature set, features in index order.  A feature
 * whose word weight is <= 0 enters neither vector.  BowVector (word id ascending, capacity n): TF_IDF and TF add the weights of a word, IDF and
 * BINARY keep the first; then L1-normalised for scoring 0, L2-normalised for scoring 1; for the other scorings TF_IDF / TF values are divided by the
 * number of entries.  FeatureVector as CSR over its ascending node ids (fv_nodes [n], fv_start [n + 1], fv_items [n]): the form of
 * oslam_bow_side2_t; fv_items is also q_idx of oslam_bow_side1_t, with q_node[j] = fv_nodes[r] for fv_start[r] <= j < fv_start[r + 1]. */
int oslam_voc_vectors(const oslam_voc_t* voc, int n, const uint32_t* word, const uint32_t* node, const double* weight, uint32_t* bow_ids, double* bow_vals,
                      int32_t* n_bow, uint32_t* fv_nodes, int32_t* fv_start, int32_t* fv_items, int32_t* n_fv);
/* score(a, b) of two BowVectors for L1_NORM, the scoring of the reference's vocabulary: -0.5 * sum over common words of (|a - b| - |a| - |b|).
 * The other five scorings are not implemented: *rc = OSLAM_E_INVALID with a message (rc may be NULL), return value 0. */
double oslam_voc_score(const oslam_voc_t* voc, int na, const uint32_t* ids_a, const double* vals_a, int nb, const uint32_t* ids_b, const double* vals_b, int* rc);

/* ------------------------------------------------------------------------------------------
 * PnP solver — ORB_SLAM2::PnPsolver (include/PnPsolver.h, src/PnPsolver.cc: EPnP inside RANSAC), the numerical operator of
 * Tracking::Relocalization (src/Tracking.cc:1650-1676), for batches of independent problems (one per lost frame and candidate keyframe).
 * The tracking driver does not call it: a sequence that is LOST stays LOST (oslam_slam.h).
 *
 * A problem is `count` correspondences (P3Dw, P2D = mvKeysUn[i].pt, sigma2 = mvLevelSigma2[octave], all float: :87-93) at `offset` of the packed
 * arrays, the intrinsics and a seed.  Problems of one call must not share correspondences.
 * SetRansacParameters (:121-157) is restated with its mixed arithmetic (oslam_pnp_ransac_params).  iterate (:165-258): its loop condition
 * `mnIterations < mRansacMaxIts || nCurrentIterations < nIterations` makes the first call run to mRansacMaxIts, so a solver is one shot and one call
 * per problem reproduces the reference's interleaved loop.  Per iteration: four indices by the swap-with-back rule (:188-201), compute_pose
 * (:477-525, fp64), CheckInliers (:308-339: Xc, Yc, invZc, distX, distY, error2 float, ue, ve double, strict comparison with sigma2 * th2); a count
 * >= minInliers that is strictly above every earlier one becomes the best (:209-224), then Refine (:260-305: EPnP over the best set, CheckInliers,
 * success when the count is strictly above minInliers) and a success returns at once.  Refine depends on the best set alone, so the result is the first
 * RECORD iteration (count >= minInliers and above every earlier count) whose Refine succeeds — status kind 1 — otherwise the last record, unrefined
 * (:241-255, bNoMore) — kind 2 — otherwise none — kind 0.  Tcw is converted from fp64 where the reference calls convertTo(CV_32F) (:219-223, :296-300).
 *
 * Normalisations:
 *  1. DUtils::Random is not in the reference tree and is seeded from the clock.  Here the four indices of an iteration either are the caller's
 *     (`samples`: four distinct correspondence indices of the problem; anything else makes that hypothesis count zero) or come from a counter-based
 *     generator: mix(x) = { x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16 } on uint32,
 *     hash(seed, iteration, draw) = mix(mix(seed + 0x9E3779B9 * (iteration + 1)) ^ (0x85EBCA6B * (draw + 1))), and draw k = 0..3 takes
 *     randi = (hash * (N - k)) >> 32 (64-bit product) from the list of remaining indices, whose entry randi is then replaced by its last entry.
 *     oslam_pnp_draw evaluates it on the host.
 *  2. For the minimal set of four points MtM has rank 8: the hypothesis depends on the null-space basis the eigen-solver returns (cvSVD in the
 *     reference, cyclic Jacobi here), so single hypotheses are not comparable with any CPU restatement; what is determined (the refined pose, the
 *     inlier set, the control flow) is.  For n >= 6 points compute_pose agrees with a CPU restatement to rounding.
 *  3. min_set other than 4 is refused with OSLAM_E_INVALID.
 *  4. cvSolve(CV_SVD) of the beta initialisations is the least-squares solution by the Householder QR of qr_solve; cvInvert(CV_SVD) of the control-point
 *     matrix uses its known factors (orthonormal PCA axes times their scales); a singular qr_solve leaves its step at zero (the reference leaves it unset).
 *     A hypothesis whose pose is not finite counts zero inliers.  pow and log of the iteration count are the device's in the kernels and the host's in
 *     oslam_pnp_ransac_params.
 *  5. Input validation: a problem with a coordinate, observation, sigma2 or intrinsic that is not finite gets kind 0 with 0 iterations run.
 *  6. The sign of a PCA axis of choose_control_points is cvSVD's choice in the reference; with noisy observations it moves compute_pose's result at
 *     the 1e-3 level (the control points, and with them the algebraic error EPnP minimises, change).  Here the component of largest magnitude of each
 *     axis (the first of equals) is positive.
 * ---------------------------------------------------------------------------------------- */
typedef struct oslam_pnp oslam_pnp_t;
typedef struct oslam_pnp_params {   /* the arguments of SetRansacParameters (:121); the reference's call is (0.99, 10, 300, 4, 0.5, 5.991) */
    double probability;
    int32_t min_inliers, max_iterations, min_set;
    float epsilon, th2;
    int32_t reserved;
} oslam_pnp_params_t;
typedef struct oslam_pnp_problem {
    int32_t count, offset;   /* correspondences offset .. offset + count - 1 of the packed arrays */
    float fx, fy, cx, cy;
    uint32_t seed;
    int32_t reserved;
} oslam_pnp_problem_t;
typedef struct oslam_pnp_ransac {   /* what SetRansacParameters leaves in mRansacMinInliers, mRansacEpsilon, mRansacMaxIts */
    int32_t min_inliers;
    float epsilon;
    int32_t iterations;   /* 0 when no_more */
    int32_t no_more;      /* N < min_inliers: iterate() returns no pose and bNoMore at once (:173-177) */
} oslam_pnp_ransac_t;
/* Host only, needs no device. */
int oslam_pnp_ransac_params(int N, double probability, int min_inliers, int max_iterations, int min_set, float epsilon, oslam_pnp_ransac_t* out);
/* The four indices iteration `iteration` of a problem with N >= 4 correspondences draws from `seed` (normalisation 1).  Host only. */
int oslam_pnp_draw(uint32_t seed, int iteration, int N, int32_t idx[4]);
/* max_iterations bounds params.max_iterations of the calls (the work arena holds one pose per problem and iteration).  OSLAM_E_HIP without a device. */
int oslam_pnp_create(oslam_pnp_t** out, int max_problems, int max_correspondences_total, int max_iterations);
void oslam_pnp_destroy(oslam_pnp_t* h);
/* Host pointers; one upload, two launches, one download, synchronous.  P3Dw [n_corr][3], P2D [n_corr][2], sigma2 [n_corr];
 * samples NULL or [n_problems][params.max_iterations][4] int32.  Outputs: Tcw [n_problems][16] float (row-major 4 x 4), inliers [n_corr] bytes (by
 * correspondence), status [n_problems][4] int32 = kind (0 none, 1 refined, 2 best unrefined), nInliers, iterations run, the iteration whose set gave
 * the result or -1; iter_inliers NULL or [n_problems][params.max_iterations] int32 = the CheckInliers count of every hypothesis of the problem's
 * iteration count (also of those after an early success), -1 beyond it.  A problem with kind 0 (count 0 or below minInliers included) keeps the caller's Tcw and inlier bytes; nothing is written
 * beyond a problem's count.  More problems, correspondences or iterations than the handle was created for: OSLAM_E_CAPACITY before anything is launched. */
int oslam_pnp_ransac_batch(oslam_pnp_t* h, int n_problems, const oslam_pnp_problem_t* problems, int n_corr, const float* P3Dw, const float* P2D, const float* sigma2,
                           const oslam_pnp_params_t* params, const int32_t* samples, float* Tcw, uint8_t* inliers, int32_t* status, int32_t* iter_inliers);
/* The same over device arrays (the problem records with their counts included; `params` is a host pointer), asynchronous on `stream`, no host
 * synchronisation.  d_iter_inliers entries beyond a problem's iteration count are left as they were.  A problem record that does not lie inside the
 * n_corr correspondences gets kind -1 and nothing else. */
int oslam_pnp_ransac_batch_device(oslam_pnp_t* h, int n_problems, const oslam_pnp_problem_t* d_problems, int n_corr, const float* d_P3Dw, const float* d_P2D,
                                  const float* d_sigma2, const oslam_pnp_params_t* params, const int32_t* d_samples, float* d_Tcw, uint8_t* d_inliers,
                                  int32_t* d_status, int32_t* d_iter_inliers, void* stream);
/* compute_pose (:477-525) alone — the device code Refine runs — for n_sets sets of counts[s] >= 4 correspondences at offsets[s]; K4 = fx, fy, cx, cy.
 * R [n_sets][9], t [n_sets][3] and err [n_sets] (the mean reprojection error compute_pose returns) are fp64.  Host pointers, synchronous. */
int oslam_pnp_epnp(oslam_pnp_t* h, int n_sets, const int32_t* counts, const int32_t* offsets, int n_corr, const float* P3Dw, const float* P2D, const float K4[4], double* R,
                   double* t, double* err);

/* ------------------------------------------------------------------------------------------
 * Sim3 solver — ORB_SLAM2::Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc: Horn's closed form inside RANSAC), the numerical operator of
 * LoopClosing::ComputeSim3 (src/LoopClosing.cc:232-343), for batches of independent problems (one per loop candidate of every sequence): one round of
 * ComputeSim3's while loop — iterate(5) of every live solver — is one call.  The driver does not close loops and does not call it.  What follows a
 * returned Sim3 there: ORBmatcher::SearchBySim3 is the next section and Optimizer::OptimizeSim3 the one after it.
 *
 * A problem is `count` correspondences at `offset` of the packed arrays — X3Dc1, X3Dc2 (the two map points in the frames of their own cameras,
 * :94-98) and sigma2_1, sigma2_2 (mvLevelSigma2[octave] of the two keypoints, :84-85), all float — the intrinsics of both cameras (mK1, mK2), a seed
 * and bFixScale.  Problems of one call must not share correspondences.  The operator derives mvP1im1 / mvP2im2 (FromCameraToImage, :405-423) and the
 * thresholds itself: mvnMaxError1/2 are std::vector<size_t> (Sim3Solver.h:78-79), so the double product 9.210 * sigmaSquare is TRUNCATED when pushed
 * (:87-88: 9 for sigma2 = 1, 13 for 1.44) and CheckInliers compares the float error with that integer converted to float, strictly, on both sides
 * (:356).  A sigma2 <= 0 gives the threshold 0.
 * SetRansacParameters (:114-138): epsilon = (float)minInliers / N, nIterations = ceil(log(1 - p) / log(1 - pow(epsilon, 3))) in double, 1 when
 * minInliers == N, clamped to [1, maxIterations] (oslam_sim3_ransac_params).  The constructor's call is (0.99, 6, 300), LoopClosing's (0.99, 20, 300).
 * iterate(nIterations) (:140-207) is incremental — its loop condition is `mnIterations < mRansacMaxIts && nCurrentIterations < nIterations` — and the
 * solver keeps mnIterations, mnBestInliers and the best transform between calls: that is the state record, input and output of every call.  N <
 * minInliers gives bNoMore at once.  Per iteration: three indices by the swap-with-back rule (:163-177), ComputeSim3 (:226-337: centroids, M = Pr2
 * Pr1^T, the 4 x 4 matrix N, the eigenvector of its largest eigenvalue as a quaternion, angle-axis, Rodrigues, the scale Pr1 . P3 / sum P3^2 or 1
 * with bFixScale, t = O1 - s R O2, T12 = [sR | t], T21 = [(1 / s) R^T | -(1 / s) R^T t], everything stored as CV_32F), CheckInliers / Project
 * (:340-403, all float: invz = 1 / z, fx * x + cx).  A count >= mnBestInliers (not strict) becomes the best; if it is also > mRansacMinInliers
 * (strict) the call returns mBestT12 at once with the inlier flags, and bNoMore stays false even on the last iteration.  After the loop bNoMore =
 * mnIterations >= mRansacMaxIts.  A later call resumes where the last one stopped.
 *
 * Normalisations:
 *  1. The generator: as normalisation 1 of the PnP solver, with three draws (`samples`: three distinct correspondence indices of the problem; anything
 *     else makes that hypothesis count zero and never the best).  oslam_sim3_draw evaluates it on the host.
 *  2. cv::eigen on the float matrix N is a cyclic Jacobi in fp64 here.  Horn is computed in fp64 from the float inputs; R, then s (from the rounded R),
 *     then t (from the rounded R and s) are rounded to float where the reference stores CV_32F, and T12, T21 and the projections are formed in
 *     float, one rounding per operator, sums from left to right.  The sign of the eigenvector does not matter: q and -q give the same rotation through
 *     the atan2 / Rodrigues route.  A hypothesis is undetermined when the two largest eigenvalues of N coincide (a collinear or coincident sample).
 *  3. A hypothesis whose R, t or s is not finite counts zero inliers and never becomes the best (in the reference a zero count can become the best
 *     while mnBestInliers is 0; a finite hypothesis with a zero count still can).
 *  4. Input validation: a problem with a coordinate, sigma2 or intrinsic that is not finite gets no_more with 0 iterations; so does N < 3, where the
 *     reference would draw from an empty list.
 *  5. log and pow of the iteration count are the device's in the kernels and the host's in oslam_sim3_ransac_params.
 * ---------------------------------------------------------------------------------------- */
typedef struct oslam_sim3 oslam_sim3_t;
typedef struct oslam_sim3_params {   /* the arguments of SetRansacParameters (:114) */
    double probability;
    int32_t min_inliers, max_iterations;
} oslam_sim3_params_t;
typedef struct oslam_sim3_problem {
    int32_t count, offset;   /* correspondences offset .. offset + count - 1 of the packed arrays */
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;   /* mK1, mK2 */
    uint32_t seed;
    int32_t fix_scale;       /* bFixScale */
} oslam_sim3_problem_t;
typedef struct oslam_sim3_state {   /* what a solver keeps between iterate() calls; zeroed with best_iteration = -1 = a fresh solver */
    int32_t iterations_done;        /* mnIterations */
    int32_t best_inliers;           /* mnBestInliers */
    int32_t best_iteration;         /* the iteration that gave the best, or -1 */
    float R[9], t[3], s;            /* GetEstimatedRotation (row-major) / Translation / Scale */
} oslam_sim3_state_t;
typedef struct oslam_sim3_ransac {
    int32_t iterations;   /* mRansacMaxIts as SetRansacParameters leaves it; 0 when no_more */
    int32_t no_more;      /* N < min_inliers (:146-150) or N < 3 (normalisation 4) */
} oslam_sim3_ransac_t;
/* Host only, needs no device. */
int oslam_sim3_ransac_params(int N, double probability, int min_inliers, int max_iterations, oslam_sim3_ransac_t* out);
/* The three indices iteration `iteration` of a problem with N >= 3 correspondences draws from `seed` (normalisation 1).  Host only. */
int oslam_sim3_draw(uint32_t seed, int iteration, int N, int32_t idx[3]);
/* max_iterations bounds params.max_iterations of the calls (the work arena holds one hypothesis per problem and iteration).  OSLAM_E_HIP without a device. */
int oslam_sim3_create(oslam_sim3_t** out, int max_problems, int max_correspondences_total, int max_iterations);
void oslam_sim3_destroy(oslam_sim3_t* h);
/* iterate(n_iterations) of every problem.  Host pointers; one upload, two launches, one download, synchronous.  X3Dc1, X3Dc2 [n_corr][3], sigma2_1,
 * sigma2_2 [n_corr]; states [n_problems], read and always written; samples NULL or [n_problems][params.max_iterations][3] int32, indexed by absolute
 * iteration.  Iterations iterations_done .. min(iterations_done + n_iterations, iterations) - 1 are evaluated and iterate()'s control flow is applied
 * in order.  status [n_problems][4] int32 = returned (1: there is a Sim3), nInliers, iterations run in this call, no_more.  On a return T12
 * [n_problems][16] float (row-major 4 x 4) and the problem's bytes of inliers [n_corr] (by correspondence) are written; otherwise the caller's bytes
 * are left as they are.  iter_inliers NULL or [n_problems][params.max_iterations] int32: the CheckInliers counts of the iterations run in this call
 * (up to a returning one), untouched elsewhere; hypotheses NULL or [n_problems][params.max_iterations][13] float: R (row-major), t, s of those
 * iterations.  OSLAM_E_CAPACITY, before anything is launched, for more problems, correspondences or iterations (params.max_iterations) than the
 * handle was created for; OSLAM_E_INVALID for min_inliers < 0 or n_iterations < 0. */
int oslam_sim3_iterate_batch(oslam_sim3_t* h, int n_problems, const oslam_sim3_problem_t* problems, oslam_sim3_state_t* states, int n_corr, const float* X3Dc1,
                             const float* X3Dc2, const float* sigma2_1, const float* sigma2_2, const oslam_sim3_params_t* params, int n_iterations, const int32_t* samples,
                             float* T12, uint8_t* inliers, int32_t* status, int32_t* iter_inliers, float* hypotheses);
/* The same over device arrays (problem and state records included; `params` is a host pointer), asynchronous on `stream`, no host synchronisation.
 * A problem record that does not lie inside the n_corr correspondences, or a state record with iterations_done < 0, gets returned = -1 and nothing
 * else is written for it. */
int oslam_sim3_iterate_batch_device(oslam_sim3_t* h, int n_problems, const oslam_sim3_problem_t* d_problems, oslam_sim3_state_t* d_states, int n_corr, const float* d_X3Dc1,
                                    const float* d_X3Dc2, const float* d_sigma2_1, const float* d_sigma2_2, const oslam_sim3_params_t* params, int n_iterations,
                                    const int32_t* d_samples, float* d_T12, uint8_t* d_inliers, int32_t* d_status, int32_t* d_iter_inliers, float* d_hypotheses,
                                    void* stream);

/* ------------------------------------------------------------------------------------------
 * SearchBySim3 — ORBmatcher::SearchBySim3 (include/ORBmatcher.h:72, src/ORBmatcher.cc:1102-1326), called by LoopClosing::ComputeSim3 on every Sim3 a
 * solver returns (src/LoopClosing.cc:324, th = 7.5), for batches of independent keyframe pairs (KF1 = the current keyframe, KF2 = a loop candidate):
 * one call is that step of every candidate of every sequence.  An operator: the driver does not close loops and does not call it.
 *
 * Keyframes are rows of flat per-keypoint arrays (oslam_sim3_match_rows_t); a pair names n1 rows at off1 and n2 rows at off2, so several pairs may
 * share the rows of the current keyframe.  Per row: mvKeysUn, mDescriptors, whether the keypoint's map point exists and is not bad (:1150-1156), and of
 * that map point GetWorldPos, GetDescriptor, mfMaxDistance and mfMinDistance (the raw members, not the 1.2f / 0.8f getters).  One camera (the
 * reference projects both directions with KF1's fx, fy, cx, cy, :1105-1108), one bounds[4] = mnMinX, mnMinY, mnMaxX, mnMaxY, mvScaleFactors,
 * mnScaleLevels and mfLogScaleFactor per call.  The pair carries the Sim3 (s12, R12 row-major, t12), both poses (T1w, T2w: row-major 4 x 4 float,
 * rows 0-2 read) and th.
 * matched_in (vpMatches12 on entry), at out_off .. out_off + n1 - 1: -1 = NULL; anything else = a map point, the value being its GetIndexInKeyFrame(pKF2)
 * (:1138), which sets vbAlreadyMatched2 only when 0 <= value < n2 (:1139); -2 stands for "matched, not in KF2".  NULL = nothing matched.
 * match12, at the same rows: the keypoint index of KF2 where the reference writes vpMatches12[i1] = vpMapPoints2[idx2] (:1319), -1 elsewhere (also
 * where matched_in had a match: -1 means "no new match").  n_found [n_pairs] is the reference's return value.
 *
 * Direction 1 -> 2 (:1148-1225), every keypoint of KF1 with a map point that is not already matched: p3Dc1 = R1w Xw + t1w, p3Dc2 = sR21 p3Dc1 + t21;
 * skipped on z < 0.0 (z == +0 gives inf / NaN projections, which IsInImage rejects; there is no special case); invz = 1.0 / z; u = fx x invz + cx;
 * KeyFrame::IsInImage (src/KeyFrame.cc:610: >= on the minimum, < on the maximum, false for NaN); dist3D = cv::norm(p3Dc2) kept when 0.8f mfMinDistance
 * <= dist3D <= 1.2f mfMaxDistance (src/MapPoint.cc:476-486); level = MapPoint::PredictScale (src/MapPoint.cc:488-503: ceil(log(mfMaxDistance /
 * dist3D) / mfLogScaleFactor) clamped to [0, nlevels - 1]); radius = th * mvScaleFactors[level]; KeyFrame::GetFeaturesInArea
 * (src/KeyFrame.cc:569-608: floor / ceil cell bounds, strict fabs(d) < r; the grid is assigned by round, src/Frame.cc:455-470, :623-632); octave in
 * [level - 1, level]; DescriptorDistance of the map point's descriptor against mDescriptors; the first strictly smaller distance wins in the order
 * cell column ix, cell row iy, keypoint index inside a cell; accepted when bestDist <= TH_HIGH = 100.  Direction 2 -> 1 (:1228-1305) is the mirror with
 * sR12, t12 and KF1's grid.  Agreement (:1308-1323): match12[i1] = idx2 iff vnMatch1[i1] == idx2 and vnMatch2[idx2] == i1.
 *
 * Roundings (float = IEEE binary32, one rounding per operator unless stated; no contraction, no fast-math):
 *  - sR12 = s12 * R12 and sR21 = (1.0 / s12) * R12^T (:1119-1120): each element is the double product (1.0 / s12 in double) rounded once to float
 *    (for sR12 that is the float product; an implementation of the scaled copy that narrows the factor 1.0 / s12 to float first differs from
 *    this by at most one unit in the last place of an element of sR21);
 *    t21 = -sR21 * t12 (:1121): the three float products summed in float from left to right, negated (a gemm with alpha = -1).
 *  - a 3 x 3 * 3 x 1 + 3 x 1 cv::Mat expression: the three float products summed in float from left to right, then `+ c` in double, rounded once
 *    (gemm_row of csrc/matcher.hip).
 *  - invz = 1.0 / z in double, rounded to float; x = X invz, u = fx x + cx in float.
 *  - cv::norm: the squares accumulated in double from left to right, an fp64 square root, rounded to float.
 *  - 1.2f * mfMaxDistance, 0.8f * mfMinDistance, mfMaxDistance / dist3D, the division by mfLogScaleFactor and th * scale in float; log is the fp64
 *    log of the float ratio rounded to float (the convention of csrc/mappoint.hip:172-173); a quotient whose ceil is NaN or does not fit an int gives
 *    level 0 (what the x86 conversion of the reference build gives, INT_MIN, clamps to).
 *  - (u - mnMinX - r) * mfGridElementWidthInv in float, mfGridElementWidthInv = 64.f / (mnMaxX - mnMinX) (src/Frame.cc:160-161).
 * Refusals: more pairs than the handle's max_pairs, a pair with more keypoints than max_keypoints, or a negative count: OSLAM_E_CAPACITY, nothing is
 * launched (rows outside the arrays: OSLAM_E_INVALID).  The device entry point cannot read the pair records: there such a record gets n_found = -2 and
 * nothing else of it is written.  A pair whose s12, R12, t12, T1w or T2w is not finite, or whose s12 <= 0, gets n_found = -1 and its match12 rows all
 * -1; the other pairs of the call are not affected.  Point data that is not finite falls out through the reference's own comparisons.  Pairs of one
 * call must not share output rows.
 * ---------------------------------------------------------------------------------------- */
typedef struct oslam_sim3_match oslam_sim3_match_t;
typedef struct oslam_sim3_pair {
    int32_t n1, off1, n2, off2;   /* KF1 = rows off1 .. off1 + n1 - 1, KF2 = rows off2 .. off2 + n2 - 1 */
    int32_t out_off;              /* matched_in and match12 rows out_off .. out_off + n1 - 1 */
    float s12, R12[9], t12[3];
    float T1w[16], T2w[16];
    float th;
} oslam_sim3_pair_t;
typedef struct oslam_sim3_match_rows {   /* n_rows entries each; the device entry point takes device pointers, desc and mp_desc 16-byte aligned */
    int32_t n_rows;
    const oslam_keypoint_t* keysUn;
    const uint8_t* desc;          /* [n_rows][32] mDescriptors */
    const uint8_t* has_mp;        /* pMP && !pMP->isBad() */
    const float* Xw;              /* [n_rows][3] */
    const uint8_t* mp_desc;       /* [n_rows][32] pMP->GetDescriptor() */
    const float* maxDistance;     /* mfMaxDistance */
    const float* minDistance;     /* mfMinDistance */
} oslam_sim3_match_rows_t;
/* max_keypoints <= 2400 (one keyframe is staged in LDS).  OSLAM_E_HIP without a device: there is no CPU fallback. */
int oslam_sim3_match_create(oslam_sim3_match_t** out, int max_pairs, int max_keypoints, int device);
void oslam_sim3_match_destroy(oslam_sim3_match_t* h);
/* Host pointers, staged through one pinned / device block pair: one upload, one launch, one download, synchronous.  matched_in may be NULL; match12
 * [n_out] and n_found [n_pairs] are read and written (rows no pair owns keep what they held). */
int oslam_match_search_by_sim3_batch(oslam_sim3_match_t* h, int n_pairs, const oslam_sim3_pair_t* pairs, const oslam_sim3_match_rows_t* rows, int n_out,
                                     const int32_t* matched_in, const oslam_camera_t* cam, const float bounds[4], const float* scaleFactors, int nlevels,
                                     float logScaleFactor, int32_t* match12, int32_t* n_found);
/* The same over device arrays (`rows` is a host struct of device pointers; cam, bounds and scaleFactors are host pointers), one launch, asynchronous
 * on `stream`, no host synchronisation. */
int oslam_match_search_by_sim3_batch_device(oslam_sim3_match_t* h, int n_pairs, const oslam_sim3_pair_t* d_pairs, const oslam_sim3_match_rows_t* rows, int n_out,
                                            const int32_t* d_matched_in, const oslam_camera_t* cam, const float bounds[4], const float* scaleFactors, int nlevels,
                                            float logScaleFactor, int32_t* d_match12, int32_t* d_n_found, void* stream);

/* ------------------------------------------------------------------------------------------
 * OptimizeSim3 — Optimizer::OptimizeSim3 (include/Optimizer.h, src/Optimizer.cc:1046-1241), called by LoopClosing::ComputeSim3 with th2 = 10 on the
 * matches SearchBySim3 has completed (src/LoopClosing.cc:327), for batches of independent problems: one call is that step of every candidate of every
 * sequence, and its return value is what the `nInliers >= 20` decision (:330) reads.  An operator: the driver does not close loops and does not call it.
 *
 * A problem is `count` correspondences at `offset` of the packed arrays, one row per pair that passed :1101-1114 (both map points exist, neither is
 * bad, the second has an index in KF2): X3Dc1 = R1w Xw1 + t1w and X3Dc2 = R2w Xw2 + t2w (:1118, :1126: the float cv::Mat expressions), obs1, obs2 (the
 * two undistorted keypoints) and invSigma2_1, invSigma2_2 (mvInvLevelSigma2 of their octaves), all float; both cameras' fx, fy, cx, cy; the Sim3 as
 * the floats LoopClosing builds gScm from (s12, R12 row-major, t12, :326); th2 and bFixScale.  Everything is fp64 from there on.
 *
 * Graph (:1068-1178): one VertexSim3Expmap (S12) and per correspondence two fixed points and two edges with a 2 x 2 information invSigma2 * I and
 * a Huber kernel of delta = (double)sqrtf(th2):
 *   EdgeSim3ProjectXYZ          e12 = obs1 - cam_map1(project(S12.map(X3Dc2)))
 *   EdgeInverseSim3ProjectXYZ   e21 = obs2 - cam_map2(project(S12.inverse().map(X3Dc1)))
 * with map(x) = s (r x) + t, inverse() = (r*, r* ((-1 / s) t), 1 / s), project(v) = v.xy / v.z, cam_map(v) = v f + c; there is no depth test.
 * Flow (:1181-1240): optimize(5); every pair with e12.chi2() > th2 || e21.chi2() > th2 is cleared and removed (nBad); with nCorrespondences - nBad < 10
 * the call returns 0 and g2oS12 stays as it was (the cleared entries stay cleared); otherwise optimize(nBad > 0 ? 10 : 5) on the rest, the same test
 * again (it clears entries and counts nIn, it removes nothing), g2oS12 := the estimate, return nIn.  chi2() is error . information . error of the
 * edge's stored _error, not robustified: after an optimize() whose last trial was rejected that is the rejected trial's error (the estimate is popped,
 * the errors are not recomputed).
 *
 * The g2o pieces, restated from the published ORB_SLAM2 Thirdparty/g2o sources (types_seven_dof_expmap, sim3.h, base_binary_edge.hpp,
 * optimization_algorithm_levenberg.cpp, linear_solver_dense.h) in the way csrc/se3_math.h restates the SE3 ones:
 *  - both edges' linearizeOplus are commented out there, so the Jacobian is BaseBinaryEdge's numeric one: per dimension d of the Sim3 vertex push,
 *    oplus(+delta e_d), computeError, pop, the same with -delta, delta = 1e-9; the column is scalar * (e+ - e-) with scalar = 1.0 / (2 delta) — a
 *    product with the reciprocal, where a description from memory may say a quotient; the points are fixed and get none.
 *  - VertexSim3Expmap::oplusImpl: update[6] = 0 with _fix_scale, estimate = Sim3(update) * estimate.
 *  - Sim3(Vector7d) with (omega, upsilon, sigma): s = exp(sigma), eps = 1e-5, four branches on |sigma| < eps and theta < eps; R = I + Omega + Omega^2
 *    for theta < eps, Rodrigues otherwise; t = (A Omega + B Omega^2 + C I) upsilon; r = Quaterniond(R), not normalised.  In the branch |sigma| >= eps,
 *    theta < eps the published text has B = ((sigma^2 / 2 - sigma + 1) s) / sigma^3 (the series of that branch would subtract 1 in the numerator); it
 *    is kept as published.
 *  - Sim3 product r = r1 r2, t = s1 (r1 t2) + t1, s = s1 s2; Eigen's matrix-to-quaternion, quaternion product and quaternion-times-vector.
 *  - OptimizationAlgorithmLevenberg: lambda = 1e-5 max |H_jj| and ni = 2 at iteration 0 of EVERY optimize call; per trial solve (H + lambda I) x = b,
 *    oplus, F' = the robustified chi2 of the live edges (DBL_MAX after a failed solve, with x = 0), rho = (F - F') / (x . (lambda x + b) + 1e-3);
 *    rho > 0 and F' finite accepts: lambda *= max(1 / 3, min(1 - (2 rho - 1)^3, 2 / 3)), ni = 2; otherwise lambda *= ni, ni *= 2 and the estimate is
 *    popped; trials repeat while rho < 0, ten at most; the call stops on the tenth trial or rho == 0.
 *  - BlockSolverX over LinearSolverDense with one 7 x 7 block: H = sum J^T (w Omega) J, b = -sum J^T (w Omega) e, w = Huber's rho[1].  With bFixScale
 *    column 6 of every J is exactly zero (both perturbed estimates are the same), so row and column 6 of H hold lambda alone and x[6] = 0.
 *
 * Normalisations:
 *  1. The order of the sums over edges is this implementation's own: lane l of a 64-lane wavefront adds its correspondences l, l + 64, ... in order
 *     (e12 before e21), then the xor butterfly 32, 16, 8, 4, 2, 1.  It is fixed, does not depend on what else is in the batch and is the same from
 *     run to run: results are bit-identical between calls, batch orders and entry points.
 *  2. An unpivoted 7 x 7 LDL^T in fp64 stands in for Eigen's pivoted one; a pivot that is not positive and finite is a failed solve.
 *  3. (2 rho - 1)^3 is two products, not pow (as csrc/pose_opt.hip); exp, sin and cos are the device's.
 *  4. Invalid inputs: a problem with a point, observation, information, intrinsic, th2 or Sim3 that is not finite, or with s12 <= 0, gets status -1
 *     and its inlier bytes are all 0; the other problems of the call are not affected.
 *  5. count == 0 returns 0 without optimising.  1 <= count < 10 still runs the first optimize and the first chi2 pass — the cleared entries are an
 *     output — and then returns 0.
 *
 * Outputs: S12 [n_problems][13] double = R (row-major, r.toRotationMatrix()), t, s, written only where the reference writes g2oS12 (otherwise the
 * caller's bytes stay); inliers [n_corr] uint8, 1 where vpMatches1[i] survives (a problem's bytes are always written; bytes no problem owns stay);
 * status [n_problems][4] int32 = the return value (or -1, -2), nCorrespondences, nBad of the first pass, 256 * LM iterations + LM trials of both
 * optimize calls together.  trace / trace_n: NULL, or [n_problems][OSLAM_SIM3_OPT_TRACE_ROWS][6] double and [n_problems] int32: per trial F before,
 * F of the trial, rho, lambda of the trial, accepted, first trial of an optimize call (the fields of oslam_poseopt_trace) and the number of trials.
 * Refusals: more problems or correspondences than the handle was created for: OSLAM_E_CAPACITY, before anything is launched.  A record that does not
 * lie inside the n_corr correspondences: OSLAM_E_INVALID from the host entry point; the device entry point cannot read the records, there such a
 * record gets status[0] = -2 and nothing else of it is written.  Problems of one call must not share correspondences.
 * ---------------------------------------------------------------------------------------- */
#define OSLAM_SIM3_OPT_TRACE_ROWS 150   /* (5 + 10) iterations of at most 10 trials */
typedef struct oslam_sim3_opt oslam_sim3_opt_t;
typedef struct oslam_sim3_opt_problem {
    int32_t count, offset;   /* correspondences offset .. offset + count - 1 of the packed arrays */
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;   /* pKF1->mK, pKF2->mK */
    float s12, R12[9], t12[3];   /* the Sim3 on entry */
    float th2;
    int32_t fix_scale;       /* bFixScale */
} oslam_sim3_opt_problem_t;
/* OSLAM_E_HIP without a device: there is no CPU fallback. */
int oslam_sim3_opt_create(oslam_sim3_opt_t** out, int max_problems, int max_correspondences_total, int device);
void oslam_sim3_opt_destroy(oslam_sim3_opt_t* h);
/* Host pointers, staged through one pinned / device block pair: one upload, one launch, one download, synchronous.  X3Dc1, X3Dc2 [n_corr][3], obs1,
 * obs2 [n_corr][2], invSigma2_1, invSigma2_2 [n_corr]; S12, inliers and status are read and written; trace and trace_n may both be NULL. */
int oslam_optimize_sim3_batch(oslam_sim3_opt_t* h, int n_problems, const oslam_sim3_opt_problem_t* problems, int n_corr, const float* X3Dc1, const float* X3Dc2, const float* obs1,
                              const float* obs2, const float* invSigma2_1, const float* invSigma2_2, double* S12, uint8_t* inliers, int32_t* status, double* trace,
                              int32_t* trace_n);
/* The same over device arrays (the problem records included), one launch, asynchronous on `stream`, no host synchronisation. */
int oslam_optimize_sim3_batch_device(oslam_sim3_opt_t* h, int n_problems, const oslam_sim3_opt_problem_t* d_problems, int n_corr, const float* d_X3Dc1, const float* d_X3Dc2,
                                     const float* d_obs1, const float* d_obs2, const float* d_invSigma2_1, const float* d_invSigma2_2, double* d_S12, uint8_t* d_inliers,
                                     int32_t* d_status, double* d_trace, int32_t* d_trace_n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sim3 projection — ORBmatcher::SearchByProjection(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, vector<MapPoint*>& vpMatched, int th)
 * (src/ORBmatcher.cc:290-403), called by LoopClosing::ComputeSim3 over mvpLoopMapPoints after the winning candidate (src/LoopClosing.cc:353-376, th = 10;
 * the loop is accepted when nTotalMatches >= 40, :379-386), and ORBmatcher::Fuse(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, float th,
 * vector<MapPoint*>& vpReplacePoint) (src/ORBmatcher.cc:977-1100), called by LoopClosing::SearchAndFuse once per corrected keyframe over the same points
 * (src/LoopClosing.cc:588-614, th = 4).  For batches of independent problems: one per sequence for the search, one per connected keyframe of every
 * sequence for Fuse.  Operators: the driver does not close loops and does not call them.
 *
 * A problem (oslam_sim3_proj_problem_t) is one keyframe (n_kp rows at kp_off of oslam_sim3_proj_kf_rows_t), one Scw (row-major 4 x 4 float, rows 0-2
 * read), one list of candidate map points (n_pts rows at pt_off of oslam_sim3_proj_pt_rows_t; several problems may name the same point rows, as every
 * Fuse call of one loop does) and th.  Per keyframe row: mvKeysUn, mDescriptors and one state byte (search: vpMatched[idx] != NULL on entry; Fuse: 0 =
 * GetMapPoint(idx) is NULL, 1 = a point that is not bad, 2 = a bad one).  Per point row: GetWorldPos, GetNormal, GetDescriptor, mfMaxDistance and
 * mfMinDistance (the raw members, as in SearchBySim3).  skip [n_pt_out], at pt_out_off .. pt_out_off + n_pts - 1: pMP->isBad() ||
 * spAlreadyFound.count(pMP) (:317 / :1005), per problem and point because the already-found set differs per keyframe; NULL = nothing is skipped.  One
 * camera, bounds[4], mvScaleFactors, mnScaleLevels and mfLogScaleFactor per call, as in SearchBySim3.
 *
 * Per point, both functions (:312-365 / :1000-1054): skipped when skip is set; p3Dc = Rcw Xw + tcw, skipped on z < 0.0 (no special case for z == +0:
 * the projection is inf or NaN and IsInImage rejects it); u, v; KeyFrame::IsInImage; dist = cv::norm(Xw - Ow) kept when 0.8f mfMinDistance <= dist <=
 * 1.2f mfMaxDistance; skipped when PO.dot(Pn) < 0.5 * dist; level = PredictScale(dist); radius = th * mvScaleFactors[level]; GetFeaturesInArea; octave in
 * [level - 1, level]; DescriptorDistance, the first strictly smaller distance wins in the order cell column, cell row, keypoint index; accepted when
 * bestDist <= TH_LOW = 50.
 * Search (:367-398): bestDist starts at 256; a keypoint whose vpMatched entry is not NULL is no candidate, and an accepted point writes vpMatched[bestIdx]
 * at once, so point i sees the claims of every point j < i.  Reproduced exactly by a fixpoint (every point takes its best among the keypoints no
 * lower-indexed point claimed in the previous pass; passes repeat until no claim changes; point i is final after pass i + 1).  matched [n_kp_out], at
 * kp_out_off .. kp_out_off + n_kp - 1: the index within the problem's list of the point that claimed the keypoint, -1 where nothing new was written (also
 * where the keypoint was matched on entry).  n_matches [n_problems] is the reference's return value; n_passes (may be NULL) the passes the fixpoint took.
 * Fuse (:1056-1097): bestDist starts at INT_MAX, no keypoint is excluded, one pass.  The surgery is reported, not performed: fused_kp [n_pt_out] at
 * pt_out_off + i is bestIdx of an accepted point, or -1; replace at the same row is -1 when vpReplacePoint[i] stays NULL and nothing is added (no match,
 * or a bad occupant, which still counts in nFused, :1087-1095), OSLAM_FUSE_ADDED for the AddObservation / AddMapPoint branch, OSLAM_FUSE_OCCUPANT when
 * vpReplacePoint[i] is the keyframe's own point at fused_kp, and p >= 0 when vpReplacePoint[i] is list point p: the keypoint was NULL on entry and p,
 * the lowest-indexed accepted point with the same bestIdx, was added there earlier in this call (later ones do not displace it).  n_fused [n_problems]
 * is the reference's return value.  Fuse does not read kp_out_off.
 *
 * Roundings: those of SearchBySim3 where the expression is the same — the 3 x 3 * 3 x 1 + 3 x 1 product (gemm_row), invz, x = X invz, u = fx x + cx,
 * cv::norm, the 0.8f / 1.2f gates, PredictScale (level 0 for a quotient that is not finite), th * scale and the grid arithmetic.  New here:
 *  - scw = sqrt(sRcw.row(0).dot(sRcw.row(0))) (:300): the products and their sum from left to right in double, an fp64 square root, rounded once to float.
 *  - Rcw = sRcw / scw and tcw = t / scw (:301-302): each element is the double product with 1.0 / scw (in double), rounded once, as for sR21 above.
 *  - Ow = -Rcw.t() * tcw (:303): the three float products summed in float from left to right, negated (a gemm with alpha = -1, as t21 above).
 *  - PO = p3Dw - Ow in float; PO.dot(Pn): the products and their sum from left to right in double, compared in double with 0.5 * dist.
 *  - `1 / z` (:331) and `1.0 / z` (:1019) are the same float: the first is a float quotient, the second a double quotient narrowed to float, and
 *    rounding a quotient of two floats first to 53 and then to 24 bits gives the correctly rounded float quotient (double rounding is innocuous for
 *    division when the wide format has at least 2 * 24 + 2 bits).
 * OpenCV is not built here: these are declared normalisations, as row (c) of VERDICT.md says of the earlier sections, not pinned facts.
 * Refusals: more problems than max_problems, a keyframe above max_keypoints, more point rows or skip / output rows than max_points_total, or a negative
 * count: OSLAM_E_CAPACITY, nothing is launched (rows outside the arrays: OSLAM_E_INVALID).  The device entry points cannot read the records: there such a
 * record gets count -2 and nothing else of it is written.  A problem whose Scw (rows 0-2) is not finite, or whose scw is not positive, gets count -1 and
 * its output rows all -1; the other problems are not affected.  Point data that is not finite falls out through the reference's own comparisons.
 * Problems of one call must not share output rows.
 * ---------------------------------------------------------------------------------------- */
#define OSLAM_FUSE_OCCUPANT (-2)
#define OSLAM_FUSE_ADDED (-3)
typedef struct oslam_sim3_proj oslam_sim3_proj_t;
typedef struct oslam_sim3_proj_problem {
    int32_t n_kp, kp_off;         /* the keyframe = rows kp_off .. kp_off + n_kp - 1 */
    int32_t n_pts, pt_off;        /* the candidate points = rows pt_off .. pt_off + n_pts - 1 */
    int32_t kp_out_off;           /* matched rows kp_out_off .. kp_out_off + n_kp - 1 (search) */
    int32_t pt_out_off;           /* skip, fused_kp and replace rows pt_out_off .. pt_out_off + n_pts - 1 */
    float Scw[16];
    float th;
} oslam_sim3_proj_problem_t;
typedef struct oslam_sim3_proj_kf_rows {   /* n_rows entries each; the device entry points take device pointers, desc 16-byte aligned */
    int32_t n_rows;
    const oslam_keypoint_t* keysUn;
    const uint8_t* desc;          /* [n_rows][32] mDescriptors */
    const uint8_t* state;         /* search: vpMatched[idx] != NULL; Fuse: 0 NULL, 1 a good point, 2 a bad point */
} oslam_sim3_proj_kf_rows_t;
typedef struct oslam_sim3_proj_pt_rows {   /* n_rows entries each; desc 16-byte aligned on the device */
    int32_t n_rows;
    const float* Xw;              /* [n_rows][3] GetWorldPos */
    const float* normal;          /* [n_rows][3] GetNormal */
    const uint8_t* desc;          /* [n_rows][32] GetDescriptor */
    const float* maxDistance;     /* mfMaxDistance */
    const float* minDistance;     /* mfMinDistance */
} oslam_sim3_proj_pt_rows_t;
/* max_keypoints <= 2400 (the keyframe is staged in LDS); max_points_total bounds the point rows and the skip / output rows of one call (the handle
 * keeps 32 bytes of device memory per row).  OSLAM_E_HIP without a device: there is no CPU fallback. */
int oslam_sim3_proj_create(oslam_sim3_proj_t** out, int max_problems, int max_keypoints, int max_points_total, int device);
void oslam_sim3_proj_destroy(oslam_sim3_proj_t* h);
/* Host pointers, staged through one pinned / device block pair: one upload, one launch, one download, synchronous.  skip and n_passes may be NULL; the
 * outputs are read and written (rows no problem owns keep what they held). */
int oslam_match_search_by_projection_sim3_batch(oslam_sim3_proj_t* h, int n_problems, const oslam_sim3_proj_problem_t* problems, const oslam_sim3_proj_kf_rows_t* kf,
                                                const oslam_sim3_proj_pt_rows_t* pts, int n_pt_out, const uint8_t* skip, int n_kp_out, const oslam_camera_t* cam,
                                                const float bounds[4], const float* scaleFactors, int nlevels, float logScaleFactor, int32_t* matched, int32_t* n_matches,
                                                int32_t* n_passes);
int oslam_match_fuse_sim3_batch(oslam_sim3_proj_t* h, int n_problems, const oslam_sim3_proj_problem_t* problems, const oslam_sim3_proj_kf_rows_t* kf,
                                const oslam_sim3_proj_pt_rows_t* pts, int n_pt_out, const uint8_t* skip, const oslam_camera_t* cam, const float bounds[4],
                                const float* scaleFactors, int nlevels, float logScaleFactor, int32_t* fused_kp, int32_t* replace, int32_t* n_fused);
/* The same over device arrays (kf and pts are host structs of device pointers; cam, bounds and scaleFactors are host pointers), one launch, asynchronous
 * on `stream`, no host synchronisation.  Calls on one handle must not overlap on the device: the search keeps per-point state in the handle. */
int oslam_match_search_by_projection_sim3_batch_device(oslam_sim3_proj_t* h, int n_problems, const oslam_sim3_proj_problem_t* d_problems, const oslam_sim3_proj_kf_rows_t* kf,
                                                       const oslam_sim3_proj_pt_rows_t* pts, int n_pt_out, const uint8_t* d_skip, int n_kp_out, const oslam_camera_t* cam,
                                                       const float bounds[4], const float* scaleFactors, int nlevels, float logScaleFactor, int32_t* d_matched,
                                                       int32_t* d_n_matches, int32_t* d_n_passes, void* stream);
int oslam_match_fuse_sim3_batch_device(oslam_sim3_proj_t* h, int n_problems, const oslam_sim3_proj_problem_t* d_problems, const oslam_sim3_proj_kf_rows_t* kf,
                                       const oslam_sim3_proj_pt_rows_t* pts, int n_pt_out, const uint8_t* d_skip, const oslam_camera_t* cam, const float bounds[4],
                                       const float* scaleFactors, int nlevels, float logScaleFactor, int32_t* d_fused_kp, int32_t* d_replace, int32_t* d_n_fused,
                                       void* stream);

/* ------------------------------------------------------------------------------------------
 * Relocalisation projection — ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, const float th,
 * const int ORBdist) (src/ORBmatcher.cc:1472-1599), which Tracking::Relocalization calls twice per candidate whose optimised pose has 10 to 49 inliers
 * (src/Tracking.cc:1717 with th = 10, ORBdist = 100; :1731 with th = 3, ORBdist = 64), for batches of independent problems: one per (lost frame,
 * candidate keyframe).  Relocalization rewrites all of mvpMapPoints before each use (:1694-1703), so the problems of a call do not see each other.  One
 * launch, one workgroup per problem.  An operator: the driver does not relocalise and does not call it.
 *
 * A problem (oslam_reloc_proj_problem_t) is one frame (n_kp rows at kp_off of oslam_reloc_proj_frame_rows_t), its pose Tcw (row-major 4 x 4 float, rows
 * 0-2 read: Rcw and tcw as they are, no scale is divided out), the map-point slots of one keyframe (n_pts rows at pt_off of oslam_reloc_proj_pt_rows_t),
 * th and ORBdist.  Per frame row: mvKeysUn (x, y, octave and angle are read), mDescriptors and has_mp = (CurrentFrame.mvpMapPoints[i] != NULL) on entry.
 * Per point row (slot i of pKF->GetMapPointMatches()): GetWorldPos, GetDescriptor, mfMaxDistance and mfMinDistance (the raw members) and kf_angle =
 * pKF->mvKeysUn[i].angle; the rows of a slot that is skipped are not read.  skip [n_pt_out], at pt_out_off .. pt_out_off + n_pts - 1: pMP == NULL ||
 * pMP->isBad() || sAlreadyFound.count(pMP) (:1492-1494), per problem and point; NULL = nothing is skipped.  One camera (fx, fy, cx, cy read), bounds[4] =
 * mnMinX, mnMinY, mnMaxX, mnMaxY, mvScaleFactors, mnScaleLevels, mfLogScaleFactor and check_orientation (mbCheckOrientation) per call.
 *
 * Per slot i in index order (:1488-1575): skipped when skip is set; x3Dc = Rcw Xw + tcw; invzc = 1.0 / zc; u = fx * xc * invzc + cx, v likewise; rejected
 * when u < mnMinX || u > mnMaxX || v < mnMinY || v > mnMaxY (both bounds inclusive, unlike IsInImage); there is NO test of the sign of z: a point behind
 * the camera that projects inside the bounds is searched like any other, and z == 0 gives an infinite u (rejected by the bounds) or a NaN; dist3D =
 * cv::norm(Xw - Ow) kept when 0.8f mfMinDistance <= dist3D <= 1.2f mfMaxDistance; level = PredictScale(dist3D, &CurrentFrame) (src/MapPoint.cc:505-520);
 * radius = th * mvScaleFactors[level]; Frame::GetFeaturesInArea(u, v, radius, level - 1, level + 1) (src/Frame.cc:567-620): the cells of the window, the
 * octave gate level - 1 <= octave <= level + 1 (bCheckLevels is always true here: maxLevel >= 1), the strict window fabs(dx) < r && fabs(dy) < r; a frame
 * keypoint whose mvpMapPoints entry is not NULL (has_mp on entry, or claimed earlier in this call) is no candidate; bestDist starts at 256 and the first
 * strictly smaller DescriptorDistance wins in the order cell column, cell row, keypoint index; accepted when bestDist <= ORBdist.  mvpMapPoints[bestIdx2]
 * is written at once, so slot i sees the claims of every slot j < i.  Reproduced exactly by the fixpoint of the Sim3 projection section (every slot takes
 * its best among the keypoints no lower slot claimed in the previous pass; passes repeat until no claim changes; slot i is final after pass i + 1, and
 * the loop is cut after n_pts + 2 passes whatever the data).
 * After the loop, with check_orientation (:1577-1596): per accepted slot rot = kf_angle[i] - frame.angle[bestIdx2] in float, + 360.0f when rot < 0.0;
 * bin = round(rot * (1.0f / 30)) (the reference's factor 1 / HISTO_LENGTH, half away from zero); bin == 30 becomes 0; ComputeThreeMaxima (:1601-1642) over
 * the sizes of the 30 bins (the first of equal sizes keeps its rank; max2 < 0.1f * (float)max1 drops ind2 and ind3, else max3 < 0.1f * (float)max1 drops
 * ind3); every match whose bin is none of the three is removed.  A removed match has still blocked later slots during the loop: the fixpoint runs on
 * the claims, the histogram once afterwards.
 * Outputs: matched [n_kp_out], at kp_out_off .. kp_out_off + n_kp - 1: the slot i the call wrote to the frame keypoint and the histogram left there, -1
 * elsewhere (also where the keypoint held a point on entry).  n_matches [n_problems]: the reference's return value.  n_removed [n_problems] (may be
 * NULL): the matches the histogram took away.  n_passes [n_problems] (may be NULL): the passes of the fixpoint.
 *
 * Roundings: those of the Sim3 projection section where the expression is the same — the 3 x 3 * 3 x 1 + 3 x 1 product (gemm_row), Ow = -Rcw.t() * tcw,
 * PO = Xw - Ow, cv::norm, the 0.8f / 1.2f gates, PredictScale (level 0 for a quotient that is not finite or does not fit an int), th * scale and the grid
 * arithmetic (mfGridElementWidthInv = 64 / (mnMaxX - mnMinX) in float, floor and ceil of the float expressions).  New here:
 *  - invzc = 1.0 / zc: a double quotient narrowed to float (the correctly rounded float quotient).
 *  - u = fx * xc * invzc + cx: float, multiplied left to right ((fx * xc) * invzc), then the sum; not fx * (xc * invzc) as in the Sim3 section.
 *  - rot, rot * factor and the comparison 0.1f * (float)max in float; round() half away from zero.
 * Normalisations (declared, not pinned facts):
 *  - A slot whose u or v is not finite has no candidates.  (A NaN passes the reference's bounds test and reaches GetFeaturesInArea, where
 *    (int)floor(NaN) is INT_MIN on x86 and the function returns nothing; an infinity fails the bounds test.)
 *  - Angles are degrees in [0, 360], as for oslam_match_project_last_frame, which makes 0 <= bin <= 12.  The reference asserts 0 <= bin < 30 and is
 *    undefined beyond; here a match whose bin is outside 0 .. 29 (an angle outside the contract, or a NaN) is counted in no bin and removed.
 *  - ORBdist outside 0 .. 255 is refused: with every candidate claimed bestDist stays 256, and a larger ORBdist would make the reference write
 *    mvpMapPoints[-1].
 *  - th is finite and not negative (the reference passes 10 and 3), and th * mvScaleFactors[level] small enough for the cell coordinates of
 *    GetFeaturesInArea to fit an int.  Beyond that the reference's float-to-int conversions overflow (INT_MIN on x86: it finds nothing); the kernel's
 *    conversions saturate instead, the walk stays inside the 64 x 48 cells and the strict window test decides.  The Sim3 projection section is alike.
 * Refusals: more problems than max_problems, a frame above max_keypoints, more point rows or skip rows than max_points_total, or a negative count:
 * OSLAM_E_CAPACITY, nothing is launched; rows outside the arrays, or an ORBdist outside 0 .. 255: OSLAM_E_INVALID.  The device entry point cannot read
 * the records: there such a record gets count -2 and nothing else of it is written.  A problem whose Tcw (rows 0-2) is not finite gets count -1, its
 * matched rows all -1 and n_removed = n_passes = 0; the other problems are not affected.  Point data that is not finite falls out through the
 * reference's own comparisons and the normalisation above.  Problems of one call must not share output rows.
 * ---------------------------------------------------------------------------------------- */
typedef struct oslam_reloc_proj oslam_reloc_proj_t;
typedef struct oslam_reloc_proj_problem {
    int32_t n_kp, kp_off;         /* the frame = rows kp_off .. kp_off + n_kp - 1 */
    int32_t n_pts, pt_off;        /* the keyframe's map-point slots = rows pt_off .. pt_off + n_pts - 1 */
    int32_t kp_out_off;           /* matched rows kp_out_off .. kp_out_off + n_kp - 1 */
    int32_t pt_out_off;           /* skip rows pt_out_off .. pt_out_off + n_pts - 1 */
    float Tcw[16];                /* CurrentFrame.mTcw */
    float th;
    int32_t ORBdist;
} oslam_reloc_proj_problem_t;
typedef struct oslam_reloc_proj_frame_rows {   /* n_rows entries each; the device entry point takes device pointers, desc 16-byte aligned */
    int32_t n_rows;
    const oslam_keypoint_t* keysUn;   /* CurrentFrame.mvKeysUn */
    const uint8_t* desc;              /* [n_rows][32] CurrentFrame.mDescriptors */
    const uint8_t* has_mp;            /* CurrentFrame.mvpMapPoints[i] != NULL on entry */
} oslam_reloc_proj_frame_rows_t;
typedef struct oslam_reloc_proj_pt_rows {      /* n_rows entries each; desc 16-byte aligned on the device */
    int32_t n_rows;
    const float* Xw;              /* [n_rows][3] GetWorldPos */
    const uint8_t* desc;          /* [n_rows][32] GetDescriptor */
    const float* maxDistance;     /* mfMaxDistance */
    const float* minDistance;     /* mfMinDistance */
    const float* kf_angle;        /* pKF->mvKeysUn[i].angle */
} oslam_reloc_proj_pt_rows_t;
/* max_keypoints <= 2400, the cap of the Sim3 projection handle: the frame is staged in LDS with the same 51 bytes per keypoint, and the angles the
 * histogram needs are read from global memory, so this kernel needs no more.  max_points_total bounds the point rows and the skip rows of one call (the
 * handle keeps 32 bytes of device memory per row).  OSLAM_E_HIP without a device: there is no CPU fallback. */
int oslam_reloc_proj_create(oslam_reloc_proj_t** out, int max_problems, int max_keypoints, int max_points_total, int device);
void oslam_reloc_proj_destroy(oslam_reloc_proj_t* h);
/* Host pointers, staged through one pinned / device block pair: one upload, one launch, one download, synchronous.  skip, n_removed and n_passes may be
 * NULL; the outputs are read and written (rows no problem owns keep what they held). */
int oslam_match_search_by_projection_reloc_batch(oslam_reloc_proj_t* h, int n_problems, const oslam_reloc_proj_problem_t* problems, const oslam_reloc_proj_frame_rows_t* frame,
                                                 const oslam_reloc_proj_pt_rows_t* pts, int n_pt_out, const uint8_t* skip, int n_kp_out, const oslam_camera_t* cam,
                                                 const float bounds[4], const float* scaleFactors, int nlevels, float logScaleFactor, int check_orientation, int32_t* matched,
                                                 int32_t* n_matches, int32_t* n_removed, int32_t* n_passes);
/* The same over device arrays (frame and pts are host structs of device pointers; cam, bounds and scaleFactors are host pointers), one launch,
 * asynchronous on `stream`, no host synchronisation.  Calls on one handle must not overlap on the device: the search keeps per-point state in the handle. */
int oslam_match_search_by_projection_reloc_batch_device(oslam_reloc_proj_t* h, int n_problems, const oslam_reloc_proj_problem_t* d_problems,
                                                        const oslam_reloc_proj_frame_rows_t* frame, const oslam_reloc_proj_pt_rows_t* pts, int n_pt_out, const uint8_t* d_skip,
                                                        int n_kp_out, const oslam_camera_t* cam, const float bounds[4], const float* scaleFactors, int nlevels,
                                                        float logScaleFactor, int check_orientation, int32_t* d_matched, int32_t* d_n_matches, int32_t* d_n_removed,
                                                        int32_t* d_n_passes, void* stream);

/* ------------------------------------------------------------------------------------------
 * OptimizeEssentialGraph — Optimizer::OptimizeEssentialGraph (include/Optimizer.h, src/Optimizer.cc:781-1044), called by LoopClosing::CorrectLoop
 * (src/LoopClosing.cc:568), for batches of independent pose graphs: one per sequence that closes a loop on this step.  One launch whatever the batch
 * size, one workgroup per graph.  An operator: the driver does not close loops and does not call it.
 *
 * A problem is n_kf keyframes at kf_offset of the packed per-keyframe arrays and n_edges edges at edge_offset of the packed edge array.  The caller
 * passes the keyframes that are not bad, in ascending mnId, re-indexed 0 .. n_kf - 1.  Per keyframe (float at the ABI, fp64 from there on): Scw
 * [13] = s, R[9] row-major, t[3]: CorrectedSim3[pKF] where present, otherwise (Rcw, tcw, 1) (:818-832); has_noncorrected (a byte) and Snc [13], read
 * only where the byte is set: NonCorrectedSim3[pKF]; fixed (a byte): pKF == pLoopKF.  Per problem fix_scale (bFixScale).  Per edge (i, j, kind): i is
 * setVertex(0), j is setVertex(1), and the measurement is formed on the device:
 *   kind 0, a new loop connection (:857-867):           Sji = Scw[j] * Scw[i].inverse()
 *   kind 1, spanning tree / old loop / covisibility (:889-972): Sji = (has_nc[j] ? Snc[j] : Scw[j]) * (has_nc[i] ? Snc[i] : Scw[i]).inverse()
 * The information is the identity and there is no robust kernel.  The same pair may appear more than once (the reference's rules let duplicates
 * through); every copy is an edge.  Every Sim3 is g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s): r = Quaterniond(R), not normalised.
 *
 * The g2o pieces, restated from the published ORB_SLAM2 Thirdparty/g2o sources (types_seven_dof_expmap, sim3.h, base_binary_edge.hpp,
 * optimization_algorithm_levenberg.cpp, block_solver.hpp); csrc/sim3_math.h holds the Sim3 ones, shared with OptimizeSim3:
 *  - EdgeSim3::computeError: _error = (C * v0->estimate() * v1->estimate().inverse()).log(), 7 rows; chi2 = _error . _error.
 *  - Sim3::log(): sigma = log(s), R = r.toRotationMatrix(), d = 0.5 (R00 + R11 + R22 - 1), eps = 1e-5, four branches on |sigma| < eps and d > 1 - eps:
 *    omega = 0.5 deltaR(R) for d > 1 - eps, otherwise theta / (2 sqrt(1 - d d)) deltaR(R) with theta = acos(d); deltaR(R) = (R21 - R12, R02 - R20,
 *    R10 - R01); A, B, C as in Sim3(Vector7d) (the published B of the |sigma| >= eps, small-angle branch unchanged); upsilon = W^-1 t with
 *    W = A Omega + B Omega^2 + C I; result (omega, upsilon, sigma).
 *  - EdgeSim3 overrides no linearizeOplus: BaseBinaryEdge's numeric Jacobian for both vertices, per non-fixed vertex and dimension d push,
 *    oplus(+1e-9 e_d), computeError, pop, the same with -1e-9; the column is (1 / 2e-9) * (e+ - e-).  A fixed vertex gets no Jacobian and no block; an
 *    edge between two fixed vertices adds to F only.
 *  - VertexSim3Expmap::oplusImpl with _fix_scale: update[6] = 0, so column 6 of every Jacobian block is exactly zero, row and column 6 of every
 *    vertex's diagonal block hold lambda alone, and x[6] = 0 / lambda = 0 (b[6] is a sum of exact zeros).
 *  - OptimizationAlgorithmLevenberg with setUserLambdaInit(1e-16) and one optimize(20): lambda = 1e-16 and ni = 2 at iteration 0; per trial solve
 *    (H + lambda I) x = b, oplus on every free vertex, F' = the plain chi2 of all edges (DBL_MAX after a failed factorisation, with x = 0),
 *    rho = (F - F') / (x . (lambda x + b) + 1e-3); rho > 0 and F' finite accepts: lambda *= max(1 / 3, min(1 - (2 rho - 1)^3, 2 / 3)), ni = 2; otherwise
 *    lambda *= ni, ni *= 2 and the estimates are popped; trials repeat while rho < 0, ten at most; the call stops on the tenth trial or rho == 0.
 *  - BlockSolver_7_3: H = sum A^T A, b = sum A^T (-e) over the edges, A the 7 x 7 Jacobian of the edge in a free vertex; H(a, b) = A_a^T A_b.
 *
 * The system.  H is symmetric in 7 x 7 blocks, one block row per free vertex in the caller's order, stored as a block envelope: row f holds the blocks
 * from its first column first[f] to the diagonal.  Cholesky fills nothing outside the envelope, so H + lambda I = L L^T is factored in place, again on
 * every trial, by a right-looking block Cholesky: per block column the 7 x 7 diagonal block (scalar Cholesky, square roots), the blocks below it
 * (L_IJ = A_IJ L_JJ^-T), the trailing update A_IK -= L_IJ L_KJ^T.  H, L and the working vectors live in device memory owned by the handle.
 * row_first [n_kf_total] int32 (device entry point; the host entry point computes it): per keyframe k the smallest index m <= k of a keyframe that an
 * edge joins to k (k itself without one), fixed or not; the row of a free keyframe starts at the first free keyframe at or after row_first[k].  The
 * problem record names its share of the handle's storage: env_offset and env_blocks, in 7 x 7 blocks (98 doubles of device memory each).
 *
 * Normalisations:
 *  1. Order of the sums: H and b are gathered per block row over the row's incident edges in edge order (the seven products of one edge's A^T A entry
 *     from row 0 upwards); F and x . (lambda x + b): lane l of 256 adds its terms l, l + 256, ..., then the xor butterfly 32 .. 1 inside each wavefront,
 *     then the four wavefronts' sums from 0 upwards.  The factorisation visits block columns in order and every entry has one owner lane per step.
 *     No atomics: results are bit-identical between calls, batch compositions and entry points.
 *  2. Block Cholesky without pivoting stands in for LinearSolverEigen's sparse Cholesky with its fill-reducing ordering; a pivot that is not positive
 *     and finite is a failed factorisation.  With fix_scale the pivots of dimension 6 are lambda itself (1e-16 at first): sqrt(1e-16) is an ordinary number.
 *  3. W.lu().solve(t) of Sim3::log is a 3 x 3 Gaussian elimination with row pivoting on the largest magnitude (Eigen's PartialPivLU), then back
 *     substitution.  (2 rho - 1)^3 is two products; log, exp, acos, sin, cos and sqrt are the device's.
 *  4. Invalid: a problem with a non-finite Scw (or Snc where has_noncorrected is set), s <= 0, an edge with i == j, an index outside the problem or a
 *     kind other than 0 / 1, or no fixed keyframe among n_kf > 0 (the reference always fixes the loop keyframe; without one the gauge is free at
 *     lambda = 1e-16) gets status {-1, 0, n_edges, 0}; its output rows keep the caller's bytes and the other problems are not affected.
 *  5. n_kf == 0, n_edges == 0 or no free keyframe: no optimisation, status {0, n_free, n_edges, 0}, the outputs hold the inputs.
 *  6. Scw_out of a keyframe the optimiser did not move (fixed ones included) is r.toRotationMatrix() of the quaternion built from the input R, t and s
 *     widened to double: what the reference's recovery loop computes for it.
 *
 * Outputs: Scw_out [n_kf_total][13] double = R (row-major, r.toRotationMatrix()), t, s; Tcw_out [n_kf_total][16] float = [R | t * (1. / s)] with last
 * row 0 0 0 1 (:992-1009); status [n_problems][4] int32 = 0 done / -1 invalid / -2 (device entry point) a record outside the arrays, a row_first
 * that leaves an edge outside the envelope or an envelope larger than env_blocks: nothing else of the problem is written; n_free; n_edges;
 * 256 * LM iterations + LM trials.  trace / trace_n: NULL, or [n_problems][OSLAM_ESSENTIAL_GRAPH_TRACE_ROWS][6] double and [n_problems] int32: per
 * trial F before, F of the trial, rho, lambda of the trial, accepted, first trial of the call (the fields of oslam_poseopt_trace).
 * Refusals: more problems, keyframes or edges than the handle was created for, or (host entry point) envelopes of more blocks than
 * max_envelope_blocks_total: OSLAM_E_CAPACITY before anything is launched.  A record outside the arrays: OSLAM_E_INVALID from the host entry point.
 * Problems of one call must not share keyframe rows, edge rows or envelope storage; calls on one handle must not overlap on the device.
 *
 * Point correction (:1013-1043), one elementwise kernel over the points of all problems: P' = Scw_out[r].inverse().map(Scw[r].map(P)) with
 * map(x) = s (r x) + t, float in, fp64 arithmetic, float out.  Per point point_problem and ref = r, the index inside that problem of the keyframe
 * the caller resolved from mnCorrectedByKF / mnCorrectedReference or GetReferenceKeyFrame().  A point with ref < 0 (bad), a problem index outside
 * the call, ref >= n_kf or a problem whose status[0] is not 0 is skipped: its output bytes stay.  UpdateNormalAndDepth is the mappoint operator's.
 * ---------------------------------------------------------------------------------------- */
#define OSLAM_ESSENTIAL_GRAPH_TRACE_ROWS 200   /* 20 iterations of at most 10 trials */
typedef struct oslam_essential_graph oslam_essential_graph_t;
typedef struct oslam_essential_graph_problem {
    int32_t n_kf, kf_offset;       /* keyframes kf_offset .. kf_offset + n_kf - 1 of the per-keyframe arrays */
    int32_t n_edges, edge_offset;  /* edges edge_offset .. edge_offset + n_edges - 1 */
    int32_t fix_scale;             /* bFixScale */
    int32_t env_offset, env_blocks; /* device entry point: the problem's 7 x 7 blocks of the handle's storage; the host entry point fills them in */
    int32_t reserved;
} oslam_essential_graph_problem_t;
/* max_envelope_blocks_total bounds the sum over a call's problems of the envelope's 7 x 7 blocks (< 2^31); the handle allocates about 800 bytes of device
 * memory per block (H and the factor, 392 bytes each, and a column-list entry).  OSLAM_E_HIP without a device: there is no CPU fallback. */
int oslam_essential_graph_create(oslam_essential_graph_t** out, int max_problems, int max_keyframes_total, int max_edges_total, long long max_envelope_blocks_total, int device);
void oslam_essential_graph_destroy(oslam_essential_graph_t* h);
/* Host arithmetic only: row_first [n_kf_total] and env_blocks [n_problems] (int64) of the problems as defined above. */
int oslam_essential_graph_envelope(int n_problems, const oslam_essential_graph_problem_t* problems, int n_kf_total, const uint8_t* fixed, int n_edges_total, const int32_t* edges,
                                   int32_t* row_first, int64_t* env_blocks);
/* Host pointers, staged through one pinned / device block pair: one upload, one launch, one download, synchronous.  Scw, Snc [n_kf_total][13], edges
 * [n_edges_total][3]; Scw_out, Tcw_out and status are read and written; trace and trace_n may both be NULL. */
int oslam_optimize_essential_graph_batch(oslam_essential_graph_t* h, int n_problems, const oslam_essential_graph_problem_t* problems, int n_kf_total, const float* Scw,
                                         const float* Snc, const uint8_t* has_noncorrected, const uint8_t* fixed, int n_edges_total, const int32_t* edges, double* Scw_out,
                                         float* Tcw_out, int32_t* status, double* trace, int32_t* trace_n);
/* The same over device arrays (the problem records, with env_offset / env_blocks, and row_first included), one launch, asynchronous on `stream`, no
 * host synchronisation. */
int oslam_optimize_essential_graph_batch_device(oslam_essential_graph_t* h, int n_problems, const oslam_essential_graph_problem_t* d_problems, int n_kf_total, const float* d_Scw,
                                                const float* d_Snc, const uint8_t* d_has_noncorrected, const uint8_t* d_fixed, const int32_t* d_row_first, int n_edges_total,
                                                const int32_t* d_edges, double* d_Scw_out, float* d_Tcw_out, int32_t* d_status, double* d_trace, int32_t* d_trace_n, void* stream);
/* Point correction: P, P_out [n_points][3] float, point_problem, ref [n_points] int32; Scw the optimiser's input, Scw_out and status its outputs. */
int oslam_essential_graph_correct_points(oslam_essential_graph_t* h, int n_problems, const oslam_essential_graph_problem_t* problems, int n_kf_total, const float* Scw,
                                         const double* Scw_out, const int32_t* status, int n_points, const int32_t* point_problem, const int32_t* ref, const float* P,
                                         float* P_out);
int oslam_essential_graph_correct_points_device(oslam_essential_graph_t* h, int n_problems, const oslam_essential_graph_problem_t* d_problems, int n_kf_total, const float* d_Scw,
                                                const double* d_Scw_out, const int32_t* d_status, int n_points, const int32_t* d_point_problem, const int32_t* d_ref,
                                                const float* d_P, float* d_P_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * LoopClosing: map corrections — the arithmetic of LoopClosing (include/LoopClosing.h, src/LoopClosing.cc) that the operators above do not cover, for
 * batches of independent sequences: mg2oScw (:334-336), CorrectLoop's Sim3 propagation with its point correction and corrected poses (:436-517), and the
 * map update after global BA (:677-738).  Operators: the driver does not close loops and calls none of this.  One handle, created for a maximum number
 * of problems, keyframes, (keyframe, keypoint) entries and points in all problems of a call.  Every Sim3 is g2o::Sim3 over Eigen::Quaterniond as
 * csrc/sim3_math.h and se3_math.h restate it; quaternions are not normalised; fp64 from the float inputs on.
 *
 * compose_scw (:334-336), one lane per problem.  Scm [13] double = R row-major, t, s (the S12 output of OptimizeSim3); Tmw [16] float = the matched
 *   keyframe's pose.  gScm = Sim3(Quaterniond(R), t, s); gSmw = Sim3(Quaterniond(toMatrix3d(Rmw)), toVector3d(tmw), 1.0); Scw = gScm * gSmw.
 *   Outputs Scw [13] double = r.toRotationMatrix(), t, s and mScw [16] float = Converter::toCvMat(Sim3) = [(float)(s R) | (float)t; 0 0 0 1]
 *   (src/Converter.cc:56-62), what the Sim3 SearchByProjection operator takes at :376.  No status: non-finite inputs give non-finite outputs.
 *   Normalisation: the reference keeps the quaternion of gScm that OptimizeSim3 left; here it is rebuilt from the R that operator returns.
 *
 * propagate (:436-517).  A problem is one sequence that closes a loop: n_kf keyframes = mvpCurrentConnectedKFs IN ASCENDING mnId at kf_offset of the
 *   per-keyframe arrays, cur = the index of mpCurrentKF among them, its points (a table of n_points rows at point_offset: P [3] float and a bad byte)
 *   and its entries (n_entries at entry_offset).  Per keyframe Tiw [16] float and kf_entries [2] int32 = first, count: its GetMapPointMatches() as
 *   `count` entries from `first` (relative to entry_offset), each the index of a point in the problem's table or -1 for a NULL pointer (NULL entries
 *   may also be left out).  Scw [n_problems][13] double as compose_scw writes it.
 *   Roundings:
 *    - Twc of the current keyframe as KeyFrame::SetPose computes it (src/KeyFrame.cc:74-81): Rwc = Rcw.t(), Ow = -Rwc * tcw = the three float products
 *      summed in float from left to right, negated; last row 0 0 0 1.
 *    - Tic = Tiw * Twc (:456), a CV_32F 4 x 4 product: every entry is the float sum, left to right, of its four float products (cv::gemm's small-matrix
 *      branch; the rule of the 3-term products elsewhere in this header extended to four terms, restated from memory of OpenCV 3.2 and unpinned).
 *    - g2oSic = Sim3(Quaterniond(toMatrix3d(Ric)), toVector3d(tic), 1.0); Corrected[i] = g2oSic * Scw for i != cur, Corrected[cur] = Scw (rebuilt from
 *      its 13 doubles); NonCorrected[i] = Sim3(Quaterniond(Riw), tiw, 1.0).
 *    - Points: P' = Corrected[k].inverse().map(NonCorrected[k].map(P)), map(x) = s (r x) + t; float in (toVector3d), fp64, float out (toCvMat).
 *    - Poses (:505-513): Tiw_out = [r.toRotationMatrix() | t * (1. / s)] rounded to float, last row 0 0 0 1.
 *   Normalisation: the reference walks CorrectedSim3, a std::map<KeyFrame*, ...>, in pointer order, and a point seen by several keyframes is corrected
 *   by the first that reaches it (mnCorrectedByKF, :489, :499).  Here the order is ascending keyframe index: a point that is not bad is corrected by the
 *   smallest-index keyframe that holds it (one integer atomicMin per entry into a claim word per point, then one pass over the points).
 *   UpdateNormalAndDepth (:501) is the mappoint operator's, as for the essential graph's point correction; the reference calls it in mid-loop, with
 *   half of the poses updated, and again after the graph optimisation.
 *   Outputs: Scorr_out, Snc_out [n_kf_total][13] double = R, t, s; Tiw_out [n_kf_total][16] float; P_out [n_points_total][3] float, written for
 *   corrected points only (the others keep the caller's bytes); corrected_ref [n_points_total] int32 = the in-problem index of the keyframe that
 *   corrected the point (mnCorrectedReference) or -1, written for every point of a valid problem: the `ref` of oslam_essential_graph_correct_points;
 *   status [n_problems][4] int32 = 0 / -1 / -2, n_kf, points corrected, entries read (the entries >= 0 of the problem's keyframes).
 *   Invalid: a non-finite pose or Scw, s <= 0, cur outside the problem, a keyframe's entries outside the problem's, or an entry below -1 or outside the
 *   point table: status {-1, n_kf, 0, 0}, none of the problem's rows is written, the other problems are not affected.  A record outside the arrays:
 *   OSLAM_E_INVALID from the host entry point, status {-2, 0, 0, 0} from the device one.  More than the handle was created for: OSLAM_E_CAPACITY before
 *   anything is launched.  Problems of one call must not share rows; calls on one handle must not overlap on the device.  Three launches whatever the
 *   batch: every problem is spread over 32 workgroups in each.
 *
 * update_after_gba (:677-738).  A problem is a whole map: n_kf keyframes in ascending mnId with parent [n_kf] int32 (-1: a member of
 *   mvpKeyFrameOrigins), kf_in_ba bytes (mnBAGlobalForKF == nLoopKF), Tcw [16] float (the poses now = mTcwBefGBA afterwards) and TcwGBA [16] float (read
 *   only where kf_in_ba is set); its points P, PosGBA (read where pt_in_ba is set), bad, ref = the in-problem index of GetReferenceKeyFrame().
 *   Keyframes (:680-701): a keyframe with kf_in_ba keeps its TcwGBA; any other gets TcwGBA[c] = (Tcw[c] * Twc[p]) * TcwGBA[p] with Twc[p] from the
 *   parent's pose BEFORE the update by SetPose's arithmetic above, both products the CV_32F 4 x 4 product above, rounded in this parenthesisation.
 *   The reference's queue order does not change the result: each keyframe has one parent and only old poses enter Tchildc.  The kernel sweeps by depth
 *   (round 1 the roots, round r + 1 the keyframes whose parent was settled by round r: at most n_kf rounds by construction).  A keyframe that no root
 *   reaches (the reference's walk starts at the origins) has reached = 0 and Tcw_out = Tcw; with one parent per keyframe it lies on or behind a cycle, which
 *   the host entry point refuses (below), so only the device entry point can report one.
 *   Points (:706-738): bad: skipped; pt_in_ba: P_out = PosGBA; otherwise, when ref is a keyframe of the problem that was reached: Xc = Rcw_before * P +
 *   tcw_before, P_out = Rwc_new * Xc + twc_new, both the float R x + t of one cv::gemm (the float sum of the three products, the + t in double,
 *   rounded once), Twc_new = SetPose(Tcw_out[ref]); otherwise the point keeps its bytes.
 *   Outputs: Tcw_out [16] float, reached bytes, P_out, status [n_problems][4] = 0 / -1 / -2, keyframes propagated (reached, not in the BA), points
 *   written (both kinds), depth rounds used (those that settled a keyframe, the roots' round included).
 *   Invalid (status {-1, 0, 0, 0}, no row written): a parent outside [-1, n_kf), a keyframe that is its own parent, a root without kf_in_ba (the
 *   reference would read an unset mTcwGBA), a non-finite Tcw, or TcwGBA where kf_in_ba is set.  The host entry point also walks `parent` before it
 *   launches anything (csrc/loop_parent_check.h) and refuses a problem with a cycle (problem.refuse, which the device entry point honours): the sweep
 *   is bounded with a cycle too, but it would report the cycle's keyframes as unreached.  Two launches: one workgroup per map for the sweep, which is a
 *   chain of dependent 4 x 4 products, and 32 per map for the points.
 * ---------------------------------------------------------------------------------------- */
typedef struct oslam_loop_correct oslam_loop_correct_t;
typedef struct oslam_loop_correct_problem {
    int32_t n_kf, kf_offset;          /* keyframes kf_offset .. kf_offset + n_kf - 1 of the per-keyframe arrays */
    int32_t cur;                      /* mpCurrentKF among them */
    int32_t n_points, point_offset;   /* the problem's point table */
    int32_t n_entries, entry_offset;  /* the problem's share of `entries` */
    int32_t reserved;
} oslam_loop_correct_problem_t;
typedef struct oslam_loop_gba_problem {
    int32_t n_kf, kf_offset, n_points, point_offset;
    int32_t refuse;                   /* not 0: status -1 and nothing else (the host entry point sets it for a `parent` with a cycle) */
    int32_t reserved[3];
} oslam_loop_gba_problem_t;
/* OSLAM_E_HIP without a device: there is no CPU fallback. */
int oslam_loop_correct_create(oslam_loop_correct_t** out, int max_problems, int max_keyframes_total, int max_entries_total, int max_points_total, int device);
void oslam_loop_correct_destroy(oslam_loop_correct_t* h);
/* Host pointers, staged through one pinned / device block pair and synchronous; the _device forms take device arrays, are asynchronous on `stream` and
 * do not synchronise the host.  Output arrays are read and written: what a call does not write keeps the caller's bytes. */
int oslam_loop_compose_scw(oslam_loop_correct_t* h, int n, const double* Scm, const float* Tmw, double* Scw, float* mScw);
int oslam_loop_compose_scw_device(oslam_loop_correct_t* h, int n, const double* d_Scm, const float* d_Tmw, double* d_Scw, float* d_mScw, void* stream);
int oslam_loop_propagate(oslam_loop_correct_t* h, int n_problems, const oslam_loop_correct_problem_t* problems, int n_kf_total, const float* Tiw, const double* Scw,
                         const int32_t* kf_entries, int n_entries_total, const int32_t* entries, int n_points_total, const float* P, const uint8_t* bad, double* Scorr_out,
                         double* Snc_out, float* Tiw_out, float* P_out, int32_t* corrected_ref, int32_t* status);
int oslam_loop_propagate_device(oslam_loop_correct_t* h, int n_problems, const oslam_loop_correct_problem_t* d_problems, int n_kf_total, const float* d_Tiw, const double* d_Scw,
                                const int32_t* d_kf_entries, int n_entries_total, const int32_t* d_entries, int n_points_total, const float* d_P, const uint8_t* d_bad,
                                double* d_Scorr_out, double* d_Snc_out, float* d_Tiw_out, float* d_P_out, int32_t* d_corrected_ref, int32_t* d_status, void* stream);
int oslam_loop_update_after_gba(oslam_loop_correct_t* h, int n_problems, const oslam_loop_gba_problem_t* problems, int n_kf_total, const int32_t* parent, const uint8_t* kf_in_ba,
                                const float* Tcw, const float* TcwGBA, int n_points_total, const float* P, const float* PosGBA, const uint8_t* pt_in_ba, const uint8_t* bad,
                                const int32_t* ref, float* Tcw_out, uint8_t* reached, float* P_out, int32_t* status);
int oslam_loop_update_after_gba_device(oslam_loop_correct_t* h, int n_problems, const oslam_loop_gba_problem_t* d_problems, int n_kf_total, const int32_t* d_parent,
                                       const uint8_t* d_kf_in_ba, const float* d_Tcw, const float* d_TcwGBA, int n_points_total, const float* d_P, const float* d_PosGBA,
                                       const uint8_t* d_pt_in_ba, const uint8_t* d_bad, const int32_t* d_ref, float* d_Tcw_out, uint8_t* d_reached, float* d_P_out,
                                       int32_t* d_status, void* stream);

/* ------------------------------------------------------------------------------------------
 * KeyFrameDatabase — ORB_SLAM2::KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc:33-309): the query both
 * Tracking::Relocalization (src/Tracking.cc:1616) and LoopClosing::DetectLoop (src/LoopClosing.cc:143) begin with, for many independent databases
 * (one per sequence) that live on the device.  Each query call is one launch, one workgroup per query.  An operator: the driver does not call it,
 * and DetectLoop's consistency groups (src/LoopClosing.cc:153-212) live in a detector over this handle: "LoopClosing::DetectLoop" below.
 *
 * State.  Database d has keyframe slots 0 .. max_keyframes - 1; the caller's keyframe id IS the slot.  A slot holds a present bit, the keyframe's
 * BowVector in the layout of oslam_voc_vectors (word ids uint32 strictly ascending, values double, at most max_words), its add serial (a counter of
 * the database, taken at add), its best-covisibility list (at most OSLAM_KFDB_COVIS = 10 keyframe ids in the caller's order: what
 * GetBestCovisibilityKeyFrames(10) returns) and reloc_score (float).  Words are stored in chunks of OSLAM_KFDB_CHUNK = 128 words taken from a pool
 * that all databases share; the pool's size is fixed at creation and erase / clear hand a keyframe's chunks back.
 *
 * There is no inverted file.  The reference's result is restated over the vectors themselves:
 *  - words(kf) = |ids(query) n ids(kf)|; a keyframe is reached when words > 0 (a loop query: and it is not one of the connected ids).
 *  - lKFsSharingWords (:86-104, :207-222) is filled walking the query's words in ascending order and each word's list in add order: its order is
 *    ascending (smallest common word id, add serial).  Every later list is that order, filtered.
 *  - minCommonWords = (int)(maxCommonWords * 0.8f) (:120, :235); a reached keyframe is scored when words > minCommonWords.
 *  - score = the L1 score of oslam_voc_score (-0.5 * sum over common words of |a - b| - |a| - |b|, a the query's value) in fp64, cast to float.
 *  - loop (:125-196): entries with si >= minScore; bestAccScore starts at minScore; a neighbour contributes when it was reached and scored by this
 *    query (mnLoopQuery == id && mnLoopWords > minCommonWords).  reloc (:242-308): every scored keyframe; bestAccScore starts at 0; a neighbour
 *    contributes when it was reached by this query, scored or not (:273).  The accumulation walks the covisibility list in order, in float; pBestKF
 *    changes on strictly greater only; entries with acc > 0.75f * bestAccScore are kept and their pBestKF is output, the first occurrence of each.
 * Normalisations:
 *  1. reloc_score.  A reloc neighbour that was reached but not scored contributes the mRelocScore an EARLIER query left in it, and the reference
 *     never initialises that field (src/KeyFrame.cc:35 names its neighbours, not it).  Here reloc_score is 0 at add, is rewritten whenever a reloc
 *     query scores the keyframe, and persists across calls.
 *  2. Every query counts as one with a fresh id (the reference's frame and keyframe ids never repeat): "reached by this query" never sees an
 *     earlier query's mark.  query_id is carried for the caller and takes no part in the result.
 *  3. Order of a score's sum: lane c of 16 adds the terms of the keyframe's common words at positions c, c + 16, ... of the keyframe's vector in
 *     ascending position, then the xor butterfly 8, 4, 2, 1 over the 16 lanes.  It depends on the two vectors only: identical vectors give identical
 *     scores, and results are bit-identical between calls, batch compositions and entry points.  No atomics on global memory.
 *  4. Ids of a covisibility list, and connected ids, outside 0 .. max_keyframes - 1 or of a slot that is not present are skipped.
 * Because of 1., two reloc queries on one database are sequential: a call holds at most one query per database.
 *
 * Mutations take arrays of records, are applied in record order on the handle's stream and return when they are applied.  A refused call changes
 * nothing.  Queries: records name their words (word_off, n_words into ids / vals) and, for loop queries, their connected keyframe ids (conn_off,
 * n_conn into conn) and min_score.  Outputs per query q: cand, cand_acc [q * max_keyframes ..]: candidate ids in the reference's order and their
 * accumulated scores; n_cand [q] their number; diag [q * 5 ..] int32 = lKFsSharingWords.size(), maxCommonWords, minCommonWords, nscores,
 * lScoreAndMatch.size(); loop queries also conn_score [n_conn_total] float: the score of the query against each connected id that is present,
 * -1 for the others (what DetectLoop :125-139 takes its minScore from).  Only L1_NORM vocabularies (scoring 0), as for oslam_voc_score.
 * ---------------------------------------------------------------------------------------- */
#define OSLAM_KFDB_COVIS 10
#define OSLAM_KFDB_CHUNK 128
#define OSLAM_KFDB_MAX_KEYFRAMES 2048   /* per database: the per-slot scratch of a query lives in LDS */
#define OSLAM_KFDB_MAX_WORDS 2400
typedef struct oslam_kfdb oslam_kfdb_t;
typedef struct oslam_kfdb_add {
    int32_t database, keyframe;
    int32_t word_off, n_words;     /* words word_off .. word_off + n_words - 1 of the call's ids / vals */
} oslam_kfdb_add_t;
typedef struct oslam_kfdb_key { int32_t database, keyframe; } oslam_kfdb_key_t;
typedef struct oslam_kfdb_covis {
    int32_t database, keyframe, n;
    int32_t ids[OSLAM_KFDB_COVIS];
} oslam_kfdb_covis_t;
typedef struct oslam_kfdb_query {
    int32_t database, query_id;
    int32_t word_off, n_words;
    int32_t conn_off, n_conn;      /* loop queries: spConnectedKeyFrames; ignored by reloc queries */
    float min_score;               /* loop queries */
    int32_t reserved;
} oslam_kfdb_query_t;
/* pool_words is rounded up to whole chunks; a keyframe of n words takes ceil(n / 128) chunks.  max_keyframes <= OSLAM_KFDB_MAX_KEYFRAMES, max_words <=
 * OSLAM_KFDB_MAX_WORDS.  OSLAM_E_HIP without a device: there is no CPU fallback.  (KeyFrameDatabase::KeyFrameDatabase, :33-37) */
int oslam_kfdb_create(oslam_kfdb_t** out, int n_databases, int max_keyframes, int max_words, long long pool_words, int device);
void oslam_kfdb_destroy(oslam_kfdb_t* h);
/* out[0] = free chunks of the pool, out[1] = all its chunks, out[2] = present keyframes over all databases. */
int oslam_kfdb_info(const oslam_kfdb_t* h, int64_t out[3]);
/* KeyFrameDatabase::add (:40-46).  OSLAM_E_INVALID: a slot that is present (or named twice in the call), ids not strictly ascending, a database
 * outside the handle; OSLAM_E_CAPACITY: keyframe >= max_keyframes, n_words > max_words, or fewer free chunks than the call needs.  The new keyframe
 * has an empty covisibility list and reloc_score 0. */
int oslam_kfdb_add(oslam_kfdb_t* h, int n, const oslam_kfdb_add_t* recs, int n_words_total, const uint32_t* ids, const double* vals);
/* KeyFrameDatabase::erase (:48-67); a slot that is not present is left alone. */
int oslam_kfdb_erase(oslam_kfdb_t* h, int n, const oslam_kfdb_key_t* recs);
/* KeyFrameDatabase::clear (:69-73) of each named database. */
int oslam_kfdb_clear(oslam_kfdb_t* h, int n, const int32_t* databases);
/* The list KeyFrame::GetBestCovisibilityKeyFrames(10) (src/KeyFrame.cc:193-201) returns for a present keyframe; replaces the one it had. */
int oslam_kfdb_set_covisibility(oslam_kfdb_t* h, int n, const oslam_kfdb_covis_t* recs);
/* KeyFrameDatabase::DetectLoopCandidates (:76-197) / DetectRelocalizationCandidates (:199-309).  Host pointers, staged through one pinned / device
 * block pair: one upload, one launch, one download, synchronous.  Refused before anything runs: two queries on one database, ids not strictly
 * ascending, a record outside the arrays (OSLAM_E_INVALID); n_words > max_words (OSLAM_E_CAPACITY). */
int oslam_kfdb_detect_loop_candidates(oslam_kfdb_t* h, const oslam_voc_t* voc, int n_queries, const oslam_kfdb_query_t* queries, int n_words_total, const uint32_t* ids,
                                      const double* vals, int n_conn_total, const int32_t* conn, int32_t* cand, float* cand_acc, int32_t* n_cand, int32_t* diag,
                                      float* conn_score);
int oslam_kfdb_detect_relocalization_candidates(oslam_kfdb_t* h, const oslam_voc_t* voc, int n_queries, const oslam_kfdb_query_t* queries, int n_words_total,
                                                const uint32_t* ids, const double* vals, int32_t* cand, float* cand_acc, int32_t* n_cand, int32_t* diag);
/* The same over device arrays, one launch, asynchronous on `stream`, no host synchronisation; the caller orders it after the mutations it depends on
 * (they have completed when they return) and before the next call on the handle.  What the host entry points refuse per call is answered per query
 * here: n_cand = -2 and nothing else of that query is written (both queries of a pair that names one database). */
int oslam_kfdb_detect_loop_candidates_device(oslam_kfdb_t* h, const oslam_voc_t* voc, int n_queries, const oslam_kfdb_query_t* d_queries, int n_words_total,
                                             const uint32_t* d_ids, const double* d_vals, int n_conn_total, const int32_t* d_conn, int32_t* d_cand, float* d_cand_acc,
                                             int32_t* d_n_cand, int32_t* d_diag, float* d_conn_score, void* stream);
int oslam_kfdb_detect_relocalization_candidates_device(oslam_kfdb_t* h, const oslam_voc_t* voc, int n_queries, const oslam_kfdb_query_t* d_queries, int n_words_total,
                                                       const uint32_t* d_ids, const double* d_vals, int32_t* d_cand, float* d_cand_acc, int32_t* d_n_cand,
                                                       int32_t* d_diag, void* stream);

/* ------------------------------------------------------------------------------------------
 * LoopClosing::DetectLoop — the step that decides whether a loop exists (src/LoopClosing.cc:104-230), for many independent sequences: a detector
 * handle over a BORROWED oslam_kfdb_t.  It takes n_databases, K = max_keyframes, the device and the stream from the kfdb, which must outlive it.
 * An operator: the driver does not call it.  No CPU fallback.
 *
 * State per database, resident on the device, W = ceil(K / 32):
 *  - Connected rows: K rows of W uint32 words; row k is the bitset of KeyFrame::GetConnectedKeyFrames() of keyframe k (bit i of word i / 32 = id i),
 *    zero at creation.  A row does not depend on keyframe k (or any id in it) being present in the kfdb: the reference keeps pointers to bad
 *    keyframes in these sets.  The caller keeps both sides of a connection current, as AddConnection / EraseConnection do.
 *    Memory: n_databases * K * W * 4 bytes (512 KB per database at K = 2048).
 *  - mvConsistentGroups (:159-212): up to max_groups groups, each a W-word bitset and an int32 consistency counter, in list order; two banks, a
 *    group count and the current bank per database.  An update writes the other bank and flips the bank only when it succeeds: a refused query
 *    changes nothing.
 *
 * The consistency update (:144-226, given the candidates c_0 .. c_{n-1} and the previous groups prev_0 .. prev_{m-1} with counters n_g), as sets:
 *  1. group_i = row(c_i) u {c_i} (:165-166).
 *  2. C(i, g) holds iff group_i n prev_g is not empty (:175-183).
 *  3. first(g) = the smallest i with C(i, g) (vbConsistentGroup, :189-194).
 *  4. The new list, for i ascending: for g ascending with first(g) == i push (group_i, n_g + 1); then, if no g has C(i, g), push (group_i, 0)
 *     (:204-208).
 *  5. Candidate i is "enough" iff some g has C(i, g) and n_g + 1 >= consistency_th (:195-199); each candidate once, in ascending i.
 * n_cand == 0 clears the groups (:145-151).  A candidate id that repeats in the input is two candidates, literally.
 *
 * Normalisations:
 *  1. minScore (:127-139) is min(1.0f, the scores of the query's connected ids that are PRESENT in the kfdb): "present in the database" stands in
 *     for !isBad(); a connected keyframe that is not in the database takes no part.  The minimum is exact and independent of execution order.
 *  2. Ids of a connected row outside 0 .. K - 1 are skipped (normalisation 4 of the kfdb).
 * Two things stay with the caller, because they are host bookkeeping over the kfdb's host free list: the gate mnId < mLastLoopKFid + 10 (:115) and
 * mpKeyFrameDB->add(mpCurrentKF) (:117, :147, :216).
 *
 * One workgroup per query; no atomics on global memory, nothing that depends on the order the hardware runs anything in; results are bit-identical
 * between calls, batch compositions and entry points.  Per-query refusals, all of which leave the state unchanged: n_enough = -2 (a database outside
 * the handle, two queries on one database in one call, a record outside the arrays or n_cand > K, a candidate id outside 0 .. K - 1, a query the
 * kfdb refused); n_enough = -3 (the new list would exceed max_groups).  Nothing else of such a query is written.
 * ---------------------------------------------------------------------------------------- */
#define OSLAM_LOOPDET_MAX_GROUPS 64
typedef struct oslam_loopdet oslam_loopdet_t;
typedef struct oslam_loopdet_conn {
    int32_t database, keyframe;
    int32_t off, n;                /* ids off .. off + n - 1 of the call's ids */
} oslam_loopdet_conn_t;
typedef struct oslam_loopdet_update {
    int32_t database;
    int32_t cand_off, n_cand;      /* vpCandidateKFs: ids cand_off .. cand_off + n_cand - 1 of the call's cand */
} oslam_loopdet_update_t;
/* LoopClosing::LoopClosing (:37-46): consistency_th is mnCovisibilityConsistencyTh (3 at :44), >= 1; 1 <= max_groups <= OSLAM_LOOPDET_MAX_GROUPS.
 * Rows and groups start empty. */
int oslam_loopdet_create(oslam_loopdet_t** out, oslam_kfdb_t* kfdb, int max_groups, int consistency_th);
void oslam_loopdet_destroy(oslam_loopdet_t* h);
/* KeyFrame::GetConnectedKeyFrames (src/KeyFrame.cc:159-166) of each named keyframe: replaces whole rows, in record order (a keyframe named twice
 * keeps its last row).  Synchronous.  OSLAM_E_INVALID: a database or keyframe outside the handle, a record outside ids. */
int oslam_loopdet_set_connected(oslam_loopdet_t* h, int n, const oslam_loopdet_conn_t* recs, int n_ids_total, const int32_t* ids);
/* Clears the rows and the groups of each named database: the partner of oslam_kfdb_clear (LoopClosing::ResetIfRequested, :635-645). */
int oslam_loopdet_reset(oslam_loopdet_t* h, int n, const int32_t* databases);
/* mvConsistentGroups of one database in list order: *n_out groups, consistency_out [max_groups], bits_out [max_groups * W]. */
int oslam_loopdet_get_groups(oslam_loopdet_t* h, int database, int32_t* n_out, int32_t* consistency_out, uint32_t* bits_out);
/* :144-226 given the candidates.  Outputs per query q: enough [q * K ..] (mvpEnoughConsistentCandidates, in candidate order), n_enough [q],
 * n_groups [q] (mvConsistentGroups.size() afterwards).  Host pointers: one upload, one launch, one download, synchronous; a call that holds what
 * would be answered with -2 is refused as a whole with OSLAM_E_INVALID before anything runs. */
int oslam_loopdet_update_consistency(oslam_loopdet_t* h, int n_queries, const oslam_loopdet_update_t* recs, int n_cand_total, const int32_t* cand, int32_t* enough,
                                     int32_t* n_enough, int32_t* n_groups);
/* The same over device arrays, asynchronous on `stream`, no host synchronisation. */
int oslam_loopdet_update_consistency_device(oslam_loopdet_t* h, int n_queries, const oslam_loopdet_update_t* d_recs, int n_cand_total, const int32_t* d_cand,
                                            int32_t* d_enough, int32_t* d_n_enough, int32_t* d_n_groups, void* stream);
/* :122-226 for the current keyframe of each database: the loop query of the kfdb with its bound derived from the connected scores (the record's
 * min_score is ignored), then the consistency update over that query's candidates; two launches on one stream, nothing returns to the host in
 * between.  Outputs: those of oslam_kfdb_detect_loop_candidates, min_score [q], and those of oslam_loopdet_update_consistency.  Refusals as for
 * oslam_kfdb_detect_loop_candidates; a query the kfdb refuses on the device (n_cand = -2) gives n_enough = -2 and leaves the groups unchanged. */
int oslam_loopdet_detect(oslam_loopdet_t* h, const oslam_voc_t* voc, int n_queries, const oslam_kfdb_query_t* queries, int n_words_total, const uint32_t* ids,
                         const double* vals, int n_conn_total, const int32_t* conn, int32_t* cand, float* cand_acc, int32_t* n_cand, int32_t* diag, float* conn_score,
                         float* min_score, int32_t* enough, int32_t* n_enough, int32_t* n_groups);
int oslam_loopdet_detect_device(oslam_loopdet_t* h, const oslam_voc_t* voc, int n_queries, const oslam_kfdb_query_t* d_queries, int n_words_total, const uint32_t* d_ids,
                                const double* d_vals, int n_conn_total, const int32_t* d_conn, int32_t* d_cand, float* d_cand_acc, int32_t* d_n_cand, int32_t* d_diag,
                                float* d_conn_score, float* d_min_score, int32_t* d_enough, int32_t* d_n_enough, int32_t* d_n_groups, void* stream);

/* ------------------------------------------------------------------------------------------
 * Covisibility graph — the point-side observation lists and KeyFrame's covisibility bookkeeping (src/KeyFrame.cc:123-208, :289-398, :553-567;
 * src/MapPoint.cc:201-271) for many independent sequences, one graph per sequence, resident on the device, with KeyFrame::UpdateConnections
 * (src/KeyFrame.cc:289-379), the covisibility queries and Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1496-1604) as kernels over it.  It produces
 * what oslam_kfdb_set_covisibility (GetBestCovisibilityKeyFrames(10)), oslam_loopdet_set_connected (GetConnectedKeyFrames()) and the edge list of
 * OptimizeEssentialGraph (GetCovisiblesByWeight(100), parents, LoopConnections) take.  An operator: the driver does not call it.  No CPU fallback.
 *
 * State per graph, K = max_keyframes, P = max_points, C = obs_cap, W = ceil(K / 32):
 *  - mObservations of every point slot: up to C entries (keyframe id, keypoint index) in ascending keyframe id, a count, mbBad and an overflow bit.
 *  - mConnectedKeyFrameWeights of every keyframe: a row of K int32 weights, 0 = absent.
 *  - per keyframe OSLAM_COVIS_KF_ORDERED_ALL: which part of the row is mvpOrderedConnectedKeyFrames.  Clear (after the keyframe's own
 *    UpdateConnections): the entries >= 15, or the single maximum when none is (:341-352).  Set (after an UpdateBestCovisibles, i.e. an AddConnection
 *    with a new or changed weight or an EraseConnection that erased): every entry.  The ordered list depends on this history, not on the row alone.
 *  - per keyframe OSLAM_COVIS_KF_CONNECTED (= !mbFirstConnection), OSLAM_COVIS_KF_IS_BAD (mbBad) and mpParent (-1 = none).
 * Bytes per graph: 8 P C + 4 P + 4 K K + 8 K (K = 2048, P = 200000, C = 16: 43.2 MB; K = 200, P = 20000, C = 16: 2.8 MB).
 *
 * Normalisations:
 *  1. Wherever the reference walks a std::map<KeyFrame*, ...> or std::set<KeyFrame*> in pointer order, ids ascend (csrc/slam_map.h:3).  sort(vPairs)
 *     with push_front therefore gives descending weight with ties in descending id.
 *  2. Children are the keyframes whose mpParent it is: ChangeParent moves a child (the reference leaves it in the old parent's mspChildrens, which it
 *     only does while that parent is being erased).
 *  3. An observation list holds at most C entries.  An OBS_ADD that meets a full list changes nothing but the point's overflow bit and is counted;
 *     whatever reads such a point afterwards answers -3 and changes nothing.  POINT_BAD clears the bit with the list.
 *
 * Whatever changes a graph runs in one workgroup (events: one wavefront) per graph, which takes the records of its graph in record order; graphs are
 * independent and records of different graphs may interleave in any way.  The queries run one workgroup per record.  No atomics on global memory,
 * nothing that depends on the order the hardware runs anything in: results are bit-identical between calls, batch compositions and entry points.
 * The host-pointer entry points are synchronous and refuse a call that holds an id outside the handle, a record outside its arrays or an unknown
 * event type as a whole with OSLAM_E_INVALID before anything runs.  The _device entry points take device arrays, are asynchronous on `stream` and do
 * no host synchronisation; there an event with such an id is skipped and such a record answers -2.  Calls on one handle are sequential: they share its
 * state (the host entry points hold the handle's lock; _device callers order their streams themselves).
 * ---------------------------------------------------------------------------------------- */
#define OSLAM_COVIS_MAX_KEYFRAMES 2048
#define OSLAM_COVIS_MAX_OBS 64
#define OSLAM_COVIS_PT_BAD 1u              /* point flags, as oslam_covis_get_state returns them */
#define OSLAM_COVIS_PT_OVERFLOW 2u
#define OSLAM_COVIS_KF_ORDERED_ALL 1u      /* keyframe flags */
#define OSLAM_COVIS_KF_CONNECTED 2u
#define OSLAM_COVIS_KF_IS_BAD 4u
enum {
    OSLAM_COVIS_EV_OBS_ADD = 0,      /* (point, keyframe, keypoint index): MapPoint::AddObservation (src/MapPoint.cc:201-212); nothing if the point has
                                      * an observation in the keyframe; the bad bit is not looked at */
    OSLAM_COVIS_EV_OBS_ERASE = 1,    /* (point, keyframe): MapPoint::EraseObservation (:214-240) without the nObs <= 2 -> SetBadFlag rule, which stays
                                      * with the caller (who knows nObs's stereo weights) and sends POINT_BAD */
    OSLAM_COVIS_EV_POINT_BAD = 2,    /* (point): MapPoint::SetBadFlag (:254-263): the bad bit, an empty list, no overflow bit */
    OSLAM_COVIS_EV_CONN_ADD = 3,     /* (keyframe, other, weight > 0): KeyFrame::AddConnection (src/KeyFrame.cc:123-136), the early return of an equal
                                      * weight included, which leaves OSLAM_COVIS_KF_ORDERED_ALL alone */
    OSLAM_COVIS_EV_CONN_ERASE = 4,   /* (keyframe, other): KeyFrame::EraseConnection (:553-567) */
    OSLAM_COVIS_EV_KF_BAD = 5,       /* (keyframe): mbBad = true alone; SetBadFlag's erasures and spanning-tree repair (:466-537) are the caller's events */
    OSLAM_COVIS_EV_PARENT_SET = 6    /* (keyframe, parent): KeyFrame::ChangeParent (:393-398) */
};
typedef struct oslam_covis oslam_covis_t;
typedef struct oslam_covis_event {
    int32_t graph, type;
    int32_t a, b, c;               /* the operands in the order the event lists them; unused ones are ignored */
} oslam_covis_event_t;
typedef struct oslam_covis_update {
    int32_t graph, keyframe;
    int32_t pts_off, n_pts;        /* mvpMapPoints as point ids, -1 = empty slot: points pts_off .. pts_off + n_pts - 1 of the call's points */
    int32_t excl_off, n_excl;      /* keyframe ids left out of new_links: exclude excl_off .. excl_off + n_excl - 1 */
} oslam_covis_update_t;
typedef struct oslam_covis_query {
    int32_t graph, keyframe;
    int32_t max_n, min_w;          /* at most max_n entries; min_w > 0: GetCovisiblesByWeight(min_w) */
} oslam_covis_query_t;
typedef struct oslam_covis_key {
    int32_t graph, keyframe;
} oslam_covis_key_t;
typedef struct oslam_covis_local {
    int32_t graph;
    int32_t pts_off, n_pts;        /* mCurrentFrame.mvpMapPoints as point ids, -1 = NULL */
} oslam_covis_local_t;
/* n_graphs graphs in the state of a new map: no observation, no connection, no parent, nothing bad.  1 <= max_keyframes <= OSLAM_COVIS_MAX_KEYFRAMES,
 * 1 <= obs_cap <= OSLAM_COVIS_MAX_OBS. */
int oslam_covis_create(oslam_covis_t** out, int n_graphs, int max_keyframes, int max_points, int obs_cap, int device);
void oslam_covis_destroy(oslam_covis_t* h);
/* Returns each named graph to the created state (Map::clear, src/Map.cc:260). */
int oslam_covis_reset(oslam_covis_t* h, int n, const int32_t* graphs);
/* The events of each graph in record order (the bookkeeping of src/MapPoint.cc:201-271 and src/KeyFrame.cc:123-136, :393-398, :553-567; MapPoint::Replace,
 * :280, is the caller's sequence of them).  n_overflow_out [n_graphs]: per graph the OBS_ADDs of this call that met a full list (0 for a graph
 * without events). */
int oslam_covis_apply(oslam_covis_t* h, int n_events, const oslam_covis_event_t* events, int32_t* n_overflow_out);
int oslam_covis_apply_device(oslam_covis_t* h, int n_events, const oslam_covis_event_t* d_events, int32_t* d_n_overflow_out, void* stream);
/* KeyFrame::UpdateConnections (src/KeyFrame.cc:289-379, the product's host restatement is csrc/slam_map.h:473-509) of each record's keyframe over its
 * mvpMapPoints; the records of one graph in record order, a later one seeing the AddConnections of an earlier one.  A duplicate point id counts once
 * per occurrence, as the reference's loop over vpMP does.  Outputs per record r:
 *   status [r]        0; 1: the counter was empty and nothing changed (:323); -3: a point with the overflow bit was read and nothing changed
 *                     (n_ordered = n_new_links = 0 then); -2 (_device only): a record outside the handle or the arrays
 *   ordered_ids / ordered_w [r * K ..], n_ordered [r]   mvpOrderedConnectedKeyFrames / mvOrderedWeights afterwards
 *   parent [r]        mpParent afterwards
 *   new_links [r * K ..], n_new_links [r]   the keys of the row AFTER the update, minus the ordered list BEFORE it, minus the exclude ids, ascending:
 *                     LoopConnections[pKFi] of src/LoopClosing.cc:549-565 with exclude = mvpCurrentConnectedKFs */
int oslam_covis_update_connections(oslam_covis_t* h, int n, const oslam_covis_update_t* recs, int n_points_total, const int32_t* points, int n_excl_total,
                                   const int32_t* exclude, int32_t* status, int32_t* ordered_ids, int32_t* ordered_w, int32_t* n_ordered, int32_t* parent,
                                   int32_t* new_links, int32_t* n_new_links);
int oslam_covis_update_connections_device(oslam_covis_t* h, int n, const oslam_covis_update_t* d_recs, int n_points_total, const int32_t* d_points, int n_excl_total,
                                          const int32_t* d_exclude, int32_t* d_status, int32_t* d_ordered_ids, int32_t* d_ordered_w, int32_t* d_n_ordered,
                                          int32_t* d_parent, int32_t* d_new_links, int32_t* d_n_new_links, void* stream);
/* The ordered list with its weights: ids / weights [r * K ..], n_out [r].  max_n = K, min_w = 0: GetVectorCovisibleKeyFrames (src/KeyFrame.cc:168-172);
 * max_n = N: GetBestCovisibilityKeyFrames(N) (:174-182; N = 10 gives the layout of oslam_kfdb_covis_t::ids); min_w = w: GetCovisiblesByWeight(w)
 * (:184-199), its quirk included: when EVERY weight is >= w, upper_bound returns end() and the answer is empty (:192-193). */
int oslam_covis_covisibles(oslam_covis_t* h, int n, const oslam_covis_query_t* recs, int32_t* ids, int32_t* weights, int32_t* n_out);
int oslam_covis_covisibles_device(oslam_covis_t* h, int n, const oslam_covis_query_t* d_recs, int32_t* d_ids, int32_t* d_weights, int32_t* d_n_out, void* stream);
/* GetConnectedKeyFrames() (src/KeyFrame.cc:159-166) as bitset rows: bits [r * W ..], bit i of word i / 32 = id i — the row oslam_loopdet_set_connected
 * builds from ids. */
int oslam_covis_connected_rows(oslam_covis_t* h, int n, const oslam_covis_key_t* recs, uint32_t* bits);
int oslam_covis_connected_rows_device(oslam_covis_t* h, int n, const oslam_covis_key_t* d_recs, uint32_t* d_bits, void* stream);
/* Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1496-1604; the driver's host restatement is csrc/slam_driver.hip:534), whole: the vote over the points
 * that are not bad, the voters that are not bad in ascending id, pKFmax by the strict '>', then for each of those voters in order, while the list has
 * at most 80 entries: the first keyframe of GetBestCovisibilityKeyFrames(10) that is neither bad nor included, the first such child in ascending id,
 * and the parent if it is not included — which leaves the OUTER loop (the break of :1593).  Outputs per record r: list [r * K ..], n_list [r]
 * (mvpLocalKeyFrames), ref_kf [r] (mpReferenceKF; -1: no voter that is not bad, the reference keeps the old one), null_out [pts_off + i] = 1 where the
 * reference sets mvpMapPoints[i] = NULL (:1513), else 0.  n_list = -1: the vote was empty (:1518), list and ref_kf are not written; -3: a point with
 * the overflow bit was read; -2 (_device only): a record outside the handle or the arrays. */
int oslam_covis_local_keyframes(oslam_covis_t* h, int n, const oslam_covis_local_t* recs, int n_points_total, const int32_t* points, int32_t* list, int32_t* n_list,
                                int32_t* ref_kf, uint8_t* null_out);
int oslam_covis_local_keyframes_device(oslam_covis_t* h, int n, const oslam_covis_local_t* d_recs, int n_points_total, const int32_t* d_points, int32_t* d_list,
                                       int32_t* d_n_list, int32_t* d_ref_kf, uint8_t* d_null_out, void* stream);
/* A plain readback of one graph (synchronous): weights [K * K] (GetWeight, src/KeyFrame.cc:201-208), parents [K], kf_flags [K] (OSLAM_COVIS_KF_*) —
 * each may be NULL — and for each of n_points point ids: obs [i * C * 2 ..] as (keyframe, index) pairs, obs_count [i], point_flags [i]
 * (OSLAM_COVIS_PT_*). */
int oslam_covis_get_state(oslam_covis_t* h, int graph, int32_t* weights, int32_t* parents, uint32_t* kf_flags, int n_points, const int32_t* points, int32_t* obs,
                          int32_t* obs_count, uint32_t* point_flags);

/* ------------------------------------------------------------------------------------------
 * Initializer —ORB_SLAM2::Initializer (include/Initializer.h, src/Initializer.cc: homography / fundamental RANSAC, model selection, motion recovery),
 * the numerical operator of Tracking::MonocularInitialization (src/Tracking.cc:661, :695), for batches of independent problems (one per sequence
 * that is still initialising).  One shot: Initialize has no resumable state.  The tracking driver does not call it: oslam_slam.h is RGB-D / stereo
 * only.  ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:405), which produces vMatches12, is the "Initialisation search" section below.
 *
 * A problem is the n1 undistorted keys of the reference frame (mvKeysUn[i].pt, float [.][2]) at off1 of the packed keys-1 array, the n2 keys of the
 * current frame at off2 of the keys-2 array, vMatches12 (int32, parallel to the keys-1 array: entry >= 0 is an index into the problem's keys 2,
 * entry < 0 no match), the intrinsics, sigma and a seed.  Problems of one call must not share keys-1 entries.
 * Initialize (:44-121):
 *  - mvMatches12 (:54-63) is the match list compacted in key-1 order; N is its length and every draw indexes it.
 *  - Normalize (:749-795) of ALL keys of each frame (not only the matched ones): mean, mean absolute deviation, T = [sX 0 -meanX sX; 0 sY -meanY sY; 0 0 1].
 *  - per iteration eight indices by the swap-with-back rule (:82-97); ComputeH21 (:226-266: the right singular vector of the smallest singular value
 *    of the 16 x 9 system) and ComputeF21 (:268-303: the null vector of the 8 x 9 system, then w(2) = 0 in a 3 x 3 SVD), both stored as CV_32F;
 *    H21i = T2inv Hn T1, H12i = H21i.inv() (:160-161), F21i = T2t Fn T1 (:212).
 *  - CheckHomography (:305-388, th 5.991) and CheckFundamental (:390-468, th 3.841, thScore 5.991) over all N matches in the reference's float
 *    arithmetic; comparisons are strict; the first iteration of strictly highest score wins per model (:165, :216), starting from score 0.
 *  - RH = SH / (SH + SF) in float; RH > 0.40 takes ReconstructH, anything else (a NaN included) ReconstructF (:112-118).
 *  - ReconstructF (:470-570): E21 = Kt F21 K, DecomposeE (:909-929), four motions (R1 t, R2 t, R1 -t, R2 -t), nMinGood = max((int)(0.9 N), 50), the
 *    0.7 maxGood similarity count, the == cascade.  ReconstructH (:572-732): Faugeras' eight motions, the d1/d2, d2/d3 < 1.00001 rejection, best /
 *    second best in the order 0..7, the final four-way condition.  (N there is the number of inliers of the best iteration.)
 *  - CheckRT (:798-907) per inlier match: the 4 x 4 DLT Triangulate (:734-747), the finiteness test, cosParallax, both depth tests with their 0.99998
 *    exemption, both reprojection tests against 4 sigma^2, nGood, parallax = acos(sorted cosParallax[min(50, size - 1)]) 180 / pi; vbGood only where
 *    cosParallax < 0.99998.
 *
 * Normalisations:
 *  1. The generator: the reference seeds DUtils::Random with 0 (:80) and DUtils is not in the tree.  As normalisation 1 of the PnP solver with eight
 *     draws (oslam_init_draw), or the caller's `samples` [n][max_iterations][8]: eight distinct indices of the compacted match list; anything else
 *     gives both hypotheses of that iteration score 0, no inliers and a NaN matrix in the dump.
 *  2. N < 8 (the reference indexes an empty list): status returned 0, model 0, no iteration is run and nothing else is written.
 *  3. Sums: Normalize and the scores accumulate sequentially in float in the reference.  Here every term is the reference's float term; the sums are taken
 *     in fp64 in a fixed order (which depends on the problem alone) and rounded to float once.
 *  4. cvSVD's choices.  The sign and scale of a null vector: nothing downstream depends on them; the vector has unit norm and its component of largest
 *     magnitude (the first of equals) is positive, which fixes the sign of the dumped H21i / F21i.  The order of the motions depends on the signs of
 *     the singular vectors: in DecomposeE t = u.col(2) has its component of largest magnitude positive and R1 is the rotation of larger trace (R1 and
 *     R2 differ by a half turn about t; u.col(2) and vt.row(2) are formed as cross products of the other two vectors, since E's third singular value is
 *     zero); in ReconstructH every left singular vector has its component of largest magnitude positive and its right vector follows.  status[4] is
 *     the winning motion's index under these conventions; the winner itself does not depend on them.  The 9 x 9 and 3 x 3 decompositions are fp64
 *     Jacobi and rounded where the reference stores CV_32F; products of float matrices accumulate in fp64 and round once (cv::gemm).
 *  5. Input validation: a key, intrinsic or sigma that is not finite, or a match index >= n2, gives status returned 0, model 0, N 0 and no iteration.
 *  6. A model without a best iteration (every score 0 or NaN) has no matrix: if it is the chosen one, status returned 0 with that model and motion -1.
 *  7. A returning problem gets all n1 entries of P3D and triangulated: zeros where the winning motion did not count the key (vP3D.resize, :808-809),
 *     the point wherever CheckRT counted it (:889) and triangulated only where cosParallax < 0.99998 (:892-893).
 * ---------------------------------------------------------------------------------------- */
typedef struct oslam_init oslam_init_t;
typedef struct oslam_init_params {   /* Initializer(ReferenceFrame, 1.0, 200) (src/Tracking.cc:661); ReconstructF / H are called with (1.0, 50) (:116-118) */
    int32_t max_iterations;
    float min_parallax;
    int32_t min_triangulated;
    int32_t reserved;
} oslam_init_params_t;
typedef struct oslam_init_problem {
    int32_t n1, off1;   /* keys off1 .. off1 + n1 - 1 of the keys-1 array (and of matches12, P3D, triangulated, match_inliers) */
    int32_t n2, off2;   /* keys of the current frame in the keys-2 array */
    float fx, fy, cx, cy;
    float sigma;
    uint32_t seed;
    int32_t reserved[2];
} oslam_init_problem_t;
/* The eight indices iteration `iteration` of a problem with N >= 8 matches draws from `seed` (normalisation 1).  Host only, needs no device. */
int oslam_init_draw(uint32_t seed, int iteration, int N, int32_t idx[8]);
/* max_keys_total bounds the keys-1 and the keys-2 array of a call, max_iterations its params.max_iterations.  OSLAM_E_HIP without a device. */
int oslam_init_create(oslam_init_t** out, int max_problems, int max_keys_total, int max_iterations);
void oslam_init_destroy(oslam_init_t* h);
/* Host pointers; one upload, two launches, one download, synchronous.  keys1 [n_keys1][2], matches12 [n_keys1], keys2 [n_keys2][2]; samples NULL or
 * [n_problems][params.max_iterations][8] int32.  Outputs: R21 [n_problems][9] and t21 [n_problems][3] float; P3D [n_keys1][3] float and triangulated
 * [n_keys1] bytes by key-1 index (normalisation 7); status [n_problems][8] int32 = returned (0 / 1), model used (0 none run, 1 H, 2 F), N, nGood of
 * the winning motion (bestGood / maxGood), its index (0..7 for H, 0..3 for F, -1 none), best H iteration, best F iteration (-1 none), nsimilar (F) or
 * secondBestGood (H); scores [n_problems][4] float = SH, SF, RH, parallax of that motion in degrees.  Dumps, each NULL or: iter_scores
 * [n_problems][max_iterations][2] float (H, F; NaN where not run), hypotheses [n_problems][max_iterations][2][9] float (H21i, F21i; NaN where not run),
 * iter_inliers [n_problems][max_iterations][2] int32 (-1 where not run), match_inliers [n_keys1][2] bytes (vbMatchesInliersH / F of the best
 * iterations by key-1 index).  A problem that does not return keeps the caller's R21, t21, P3D and triangulated.  More problems, keys or iterations
 * than the handle was created for: OSLAM_E_CAPACITY before anything is launched. */
int oslam_init_initialize_batch(oslam_init_t* h, int n_problems, const oslam_init_problem_t* problems, int n_keys1, const float* keys1, const int32_t* matches12, int n_keys2,
                                const float* keys2, const oslam_init_params_t* params, const int32_t* samples, float* R21, float* t21, float* P3D, uint8_t* triangulated,
                                int32_t* status, float* scores, float* iter_scores, float* hypotheses, int32_t* iter_inliers, uint8_t* match_inliers);
/* The same over device arrays (`params` is a host pointer), asynchronous on `stream`, no host synchronisation.  Dump entries of what is not run are left
 * as they were.  A problem record that does not lie inside the key arrays gets status -1, 0, 0, 0, -1, -1, -1, 0 and nothing else. */
int oslam_init_initialize_batch_device(oslam_init_t* h, int n_problems, const oslam_init_problem_t* d_problems, int n_keys1, const float* d_keys1, const int32_t* d_matches12,
                                       int n_keys2, const float* d_keys2, const oslam_init_params_t* params, const int32_t* d_samples, float* d_R21, float* d_t21, float* d_P3D,
                                       uint8_t* d_triangulated, int32_t* d_status, float* d_scores, float* d_iter_scores, float* d_hypotheses, int32_t* d_iter_inliers,
                                       uint8_t* d_match_inliers, void* stream);
/* Measurement: with timing on, every later call records events before, between and after its two launches on the call's stream;
 * oslam_init_last_kernel_ms waits for the last call's events and gives the milliseconds of the hypothesis kernel and of the reconstruction kernel. */
int oslam_init_set_timing(oslam_init_t* h, int on);
int oslam_init_last_kernel_ms(oslam_init_t* h, float ms[2]);

/* ------------------------------------------------------------------------------------------
 * Initialisation search — ORBmatcher::SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched, vector<int>& vnMatches12,
 * int windowSize) (src/ORBmatcher.cc:405-520), which Tracking::MonocularInitialization calls with ORBmatcher(0.9, true) and windowSize = 100
 * (src/Tracking.cc:680-681), for batches of independent problems: one per sequence that is still initialising.  It produces the vMatches12 that the
 * Initializer above takes, in the layout it takes (matches12 [n_rows1], parallel to the frames-1 rows), so that the two operators chain on one stream
 * with no host step.  One launch, one workgroup per problem.  An operator: the driver does not call it (oslam_slam.h is RGB-D / stereo only).
 *
 * A problem (oslam_init_match_problem_t) is F1 (n1 rows at off1 of oslam_init_match_f1_rows_t, and of prev_matched and matches12), F2 (n2 rows at off2
 * of oslam_init_match_f2_rows_t) and windowSize.  Per row: mvKeysUn (x, y, octave and angle are read) and mDescriptors.  bounds[4] = mnMinX, mnMinY,
 * mnMaxX, mnMaxY, nnratio (mfNNratio) and check_orientation (mbCheckOrientation) per call.  prev_matched [n_rows1][2] is vbPrevMatched, read and written.
 *
 * vMatchedDistance [n2] starts at INT_MAX and vnMatches21 [n2] at -1 (:415-416).  Per key i1 of F1 in index order (:418-487):
 *  1. a key with octave > 0 does not search (:421-423).
 *  2. F2.GetFeaturesInArea(vbPrevMatched[i1].x, .y, windowSize, 0, 0) (src/Frame.cc:567-620): the window is centred on the CARRIED point, not on the key;
 *     r = (float)windowSize; the cell range is the floor and ceil of the float expressions, nothing when it lies outside the 64 x 48 grid; only F2 keys
 *     of octave 0 are candidates (bCheckLevels is true: maxLevel >= 0); the strict window fabs(dx) < r && fabs(dy) < r; the visiting order is cell
 *     column, cell row, key index.
 *  3. per candidate i2: dist = DescriptorDistance; a candidate with vMatchedDistance[i2] <= dist is skipped entirely, it is neither best nor second
 *     best (:444-445); else bestDist / bestDist2 / bestIdx2 update by strict < (:447-456): the first visited among equal distances is the best.
 *  4. accepted when bestDist <= TH_LOW (50) and bestDist < (float)bestDist2 * mfNNratio (:459-461); bestDist2 stays INT_MAX without a second candidate.
 *  5. on acceptance (:463-471): if vnMatches21[bestIdx2] >= 0 that earlier key is displaced (its vnMatches12 becomes -1); then vnMatches12[i1] =
 *     bestIdx2, vnMatches21[bestIdx2] = i1, vMatchedDistance[bestIdx2] = bestDist.  A later key takes a keypoint from an earlier one only when it
 *     is strictly nearer.
 *  6. with check_orientation (:473-483): rot = F1.angle[i1] - F2.angle[bestIdx2] in float, + 360.0f when rot < 0; bin = round(rot * (1.0f / 30)), half
 *     away from zero; 30 becomes 0; i1 is pushed to its bin at acceptance: a key displaced later stays there and counts towards the bin's size.
 * After the loop, with check_orientation: ComputeThreeMaxima (:1601-1642, as in the relocalisation section) over the sizes of the 30 bins; the entries
 * of every other bin that still hold a match lose it (:489-512).  A match removed here has still blocked and displaced others during the loop.
 * Finally vbPrevMatched[i1] = F2.mvKeysUn[vnMatches12[i1]].pt for the surviving matches only (:514-517); every other entry keeps what it held.
 * Outputs: matches12 [n_rows1] (all n1 entries of a problem are written: the keypoint of F2, or -1); prev_matched; n_matches [n_problems]: the
 * reference's return value.  May be NULL: n_removed [n_problems]: the matches the histogram took away; n_displaced [n_problems]: the displacements of
 * step 5; n_overflow [n_problems]: the keys whose candidate list did not fit the kernel's per-key cache (a cost figure: the result does not depend on
 * it).
 * The kernel finds every key's candidates in parallel and then replays steps 3-5 in key order by one wavefront, literally; it uses no atomics on
 * global memory and its outputs are bit-identical from run to run.
 *
 * Roundings: r = (float)windowSize; the grid arithmetic of the relocalisation section; (float)bestDist < (float)bestDist2 * mfNNratio with the product
 * and the comparison in float; rot, rot * factor and 0.1f * (float)max in float; round() half away from zero.
 * Normalisations (declared, not pinned facts):
 *  - An F1 key with octave < 0 does not search.  (The reference would search all levels: bCheckLevels is false for minLevel = maxLevel < 0.  The
 *    extractor never produces such a key.)
 *  - A carried point that is not finite has no candidates ((int)floor(NaN) is INT_MIN on x86 and GetFeaturesInArea returns nothing).
 *  - Angles are degrees in [0, 360], as in the relocalisation section: a match whose bin falls outside 0 .. 29 (a NaN, an angle outside the
 *    contract) is counted in no bin and removed.
 *  - windowSize small enough for the cell coordinates to fit an int; beyond that the kernel's conversions saturate, the walk stays inside the grid
 *    and the strict window test decides.
 * Refusals: more problems than max_problems, an F2 above max_keypoints, more frames-1 rows than max_keys1_total, or a negative count:
 * OSLAM_E_CAPACITY, nothing is launched; rows outside the arrays, windowSize < 0, or an nnratio that is not finite or <= 0: OSLAM_E_INVALID.  The
 * device entry point cannot read the records: there such a record gets count -2 and nothing else of it is written.  Problems of one call must not
 * share frames-1 rows (they may share frames-2 rows); rows no problem owns keep what they held.
 * ---------------------------------------------------------------------------------------- */
typedef struct oslam_init_match oslam_init_match_t;
typedef struct oslam_init_match_problem {
    int32_t n1, off1;      /* F1 = frames-1 rows off1 .. off1 + n1 - 1 (and those of prev_matched and matches12) */
    int32_t n2, off2;      /* F2 = frames-2 rows off2 .. off2 + n2 - 1 */
    int32_t windowSize;
    int32_t reserved;
} oslam_init_match_problem_t;
typedef struct oslam_init_match_f1_rows {   /* n_rows entries each; the device entry points take device pointers, desc 16-byte aligned */
    int32_t n_rows;
    const oslam_keypoint_t* keysUn;   /* F1.mvKeysUn */
    const uint8_t* desc;              /* [n_rows][32] F1.mDescriptors */
} oslam_init_match_f1_rows_t;
typedef struct oslam_init_match_f2_rows {
    int32_t n_rows;
    const oslam_keypoint_t* keysUn;   /* F2.mvKeysUn */
    const uint8_t* desc;              /* [n_rows][32] F2.mDescriptors */
} oslam_init_match_f2_rows_t;
/* max_keypoints <= 2400 bounds n2: F2 is staged in LDS with the 51 bytes per keypoint of the projection handles (the two int vectors are
 * vMatchedDistance and vnMatches21).  max_keys1_total bounds the frames-1 rows of one call (the handle keeps 32 bytes of device memory per row; the
 * bins are 30 counters in LDS).  OSLAM_E_HIP without a device: there is no CPU fallback. */
int oslam_init_match_create(oslam_init_match_t** out, int max_problems, int max_keypoints, int max_keys1_total, int device);
void oslam_init_match_destroy(oslam_init_match_t* h);
/* Host pointers, staged through one pinned / device block pair: one upload, one launch, one download, synchronous.  n_removed, n_displaced and
 * n_overflow may be NULL; prev_matched and the outputs are read and written (rows no problem owns keep what they held). */
int oslam_match_search_for_initialization_batch(oslam_init_match_t* h, int n_problems, const oslam_init_match_problem_t* problems, const oslam_init_match_f1_rows_t* frames1,
                                                const oslam_init_match_f2_rows_t* frames2, const float bounds[4], float nnratio, int check_orientation, float* prev_matched,
                                                int32_t* matches12, int32_t* n_matches, int32_t* n_removed, int32_t* n_displaced, int32_t* n_overflow);
/* The same over device arrays (frames1 and frames2 are host structs of device pointers; bounds is a host pointer), one launch, asynchronous on
 * `stream`, no host synchronisation.  Calls on one handle must not overlap on the device: the search keeps per-key state in the handle. */
int oslam_match_search_for_initialization_batch_device(oslam_init_match_t* h, int n_problems, const oslam_init_match_problem_t* d_problems,
                                                       const oslam_init_match_f1_rows_t* frames1, const oslam_init_match_f2_rows_t* frames2, const float bounds[4], float nnratio,
                                                       int check_orientation, float* d_prev_matched, int32_t* d_matches12, int32_t* d_n_matches, int32_t* d_n_removed,
                                                       int32_t* d_n_displaced, int32_t* d_n_overflow, void* stream);
/* Measurement: the shader-clock ticks workgroup 0 of the handle's last call spent in staging F2, in the candidate search, in the sequential replay and
 * in the histogram and the outputs.  Waits for the device. */
int oslam_init_match_last_phase_ticks(oslam_init_match_t* h, int64_t ticks[4]);

/* ------------------------------------------------------------------------------------------
 * Object association — what Tracking::TrackObject (src/Tracking.cc:1058-1076) runs on every frame: Frame::ExtractHSVHistogramsFromMask
 * (src/Frame.cc:388-414) per detection, ObjectMatcher::MatchTwoFrame(mLastFrame, mCurrentFrame) (src/ObjectMatcher.cc:47-440) and
 * ObjectMatcher::MatchMapToFrame(GetAllObject3Ds(), mCurrentFrame) (:442-801), for batches of independent frames.  Operators: the driver does not call
 * them, oslam_slam.h still takes the caller's track_id per detection.  Only the live code is built: the commented-out 3D-2D and ORB checks of
 * MatchTwoFrame, and the 3D-2D counts, 3-D boxes and view vectors that MatchMapToFrame computes and never uses, are not.
 *
 * 1. Appearance (src/Frame.cc:388-414, constants include/Frame.h:123-127).  Per frame an 8-bit 3-channel interleaved image [H][stride], read as B, G, R
 *    whatever the camera's order is (the reference always applies CV_BGR2HSV), and n masks [H][mask_stride] of bytes; a pixel counts for a mask when
 *    its byte is non-zero (cv::calcHist's mask rule).  Frames of one call share W, H and the strides.  Per mask: counts [94] int32 and hist [94] float,
 *    columns in the order the hconcat calls (:403-410) leave: V (32 bins), S (32), H (30).  OpenCV is not in the tree; its arithmetic is restated:
 *     - RGB2HSV_b, hue range 180, hsv_shift = 12: sdiv[i] = saturate_cast<int>((255 << 12) / (1.0 * i)), hdiv[i] = saturate_cast<int>((180 << 12) /
 *       (6.0 * i)), sdiv[0] = hdiv[0] = 0 (saturate_cast<int>(double) rounds to nearest even); v = max(b, g, r), vmin = min(b, g, r), diff = v - vmin;
 *       s = (diff * sdiv[v] + (1 << 11)) >> 12; h = g - b when v == r, else b - r + 2 diff when v == g, else r - g + 4 diff;
 *       h = (h * hdiv[diff] + (1 << 11)) >> 12 (arithmetic shift), + 180 when h < 0; the outputs are (uchar)h, (uchar)s, (uchar)v.
 *     - calcHist, 8-bit, uniform: per channel a 256-entry table idx = cvFloor(j * a + b) in double, a = size / (high - low), b = -a * low; a value
 *       whose idx lies outside [0, size) is not counted.  Built on the host once per handle.
 *     - cv::normalize(NORM_L1): norm = the sum of the 94 counts as a double (three times the mask's pixel count), scale = norm > DBL_EPSILON ?
 *       1.0 / norm : 0.0, hist[k] = (float)count[k] * (float)scale.  An empty mask gives zeros.
 *    The image is read once per frame; each pixel is converted once and tested against every mask of its frame.  A workgroup owns a band of 32 rows and
 *    counts with integer LDS atomics; a second pass sums the bands' counts in band order, in integers: counts and hist are bit-identical from run to run.
 *
 * 2. MatchTwoFrame.  A problem (oslam_objmatch_pair_problem_t) is the previous frame's objects in order (rows of `pre`: obj3d = the Object3D's id,
 *    negative for NULL; label = the Object3D's mLabel; hist; box x, y, w, h) and the current frame's detections (rows of `cur`: label, hist, box and
 *    obj3d = mvpObject3Ds, negative for NULL, read and written).  Per previous object in order (:59), NULL ones skipped (:62): every detection that is
 *    not claimed (:98) and has the object's label (:101) gets
 *     - CalCosineSimilarity(Pre, Cur) (:877-889) over bins 0..93 in order: xy += a * b in float; xx = (float)((double)xx + (double)a * (double)a)
 *       (pow(float, 2) promotes to double), yy likewise; xy / (sqrtf(xx) * sqrtf(yy)) in float;
 *     - the box IoU (:131-147) in float: corners x + w, y + h, areas w * h, std::max / std::min with the current box as first argument, 0 when
 *       x1 >= x2 || y1 >= y2 (what :138 leaves unset reads as 0 through map::operator[]), else inter / (PreArea + CurArea - inter).
 *    The winner is the detection of largest similarity (:271-283); it is claimed when MaxSimilarity > min_similarity && idx >= 0 && IoU[idx] > min_iou
 *    (:430-435), the floats compared against the double thresholds.  A detection claimed for one object is hidden from the next.
 *    similarity and iou [n_pre][n_cur] at off_score hold NaN where the reference computes nothing (a NULL object, a claimed detection, another label).
 *    Normalisations (declared, not pinned facts):
 *     - `for(int idx_pre; ...)` (:59) has no initialiser: 0.
 *     - std::sort followed by back() leaves ties unspecified: what a stable sort gives, the largest index among equals.
 *     - A NaN similarity (a histogram of zeros) makes the comparator of std::sort inconsistent: such a detection is never the winner.  Whichever the
 *       reference picked, a NaN MaxSimilarity would claim nothing.
 *
 * 3. MatchMapToFrame.  A problem (oslam_objmatch_map_problem_t) is the frame's Rwc, Ow, fx, fy, cx, cy, its detections (rows of `cur`: label, hist,
 *    obj3d read and written, and kp_n keypoints (u, v, z), z > 0, at kp_off of the flat array kps) and the map's objects in the caller's order (rows of
 *    oslam_objmatch_obj_rows_t: id, label, obs_n observations at obs_off of obs_center [.][3] and obs_hist [.][94]).  Objects whose id is among the
 *    frame's obj3d when the call begins are skipped (the snapshot of :451-459, not updated inside the loop), NULL objects too (:468).  Per object in
 *    order, per detection that is not claimed (:507) and has the object's label (:512):
 *     - similarity = the maximum over the observations of CalCosineSimilarity(observed, detection), starting from 0 with a strict > (:519-542);
 *     - the centre of the unprojected keypoints (:567-573, Frame::UnprojectStereo src/Frame.cc:906-920): x = (u - cx) * z * invfx with invfx = 1.0f / fx,
 *       y likewise; Rwc * x3Dc + Ow, every row accumulated in float in column order, then + Ow; the float sum over the keypoints in order, times
 *       (float)(1.0 / n);
 *     - Dist = (float)sqrt((double)dx * dx + (double)dy * dy + (double)dz * dz) on the float differences observed centre - centre; meanDist = the float
 *       sum in observation order divided by (float)nObs (equal to the reference's division by a double: both operands are floats and a double
 *       quotient rounds to the same float); minDist starts at FLT_MAX with a strict < (:577-594).
 *    Two independent decisions (:783-794), both may fire for one object: MaxSimilarity > min_similarity && idx >= 0 && meanDist[idx] < max_mean_dist
 *    claims the detection of largest similarity (largest index among equals), MinMinPosDist < max_min_dist && idx2 >= 0 claims the detection of
 *    smallest minDist (smallest index among equals, as a stable sort followed by front()).  Claims hide detections from later objects.
 *    similarity, mean_dist, min_dist [n_obj][n_cur] at off_score hold NaN where nothing is computed.
 *    Normalisations: Map::GetAllObject3Ds iterates a std::set of pointers, so the reference's object order is the allocator's: here it is the
 *    caller's order (the adapter passes ascending mTrackID).  Where OpenCV's own rounding is not known (Mat expressions, cv::norm) the lines above are
 *    the specification.  A NaN score is never a winner.
 *    Preconditions, each refused per problem: an object without observations and a detection without keypoints (both would divide 0 by 0), a range
 *    outside its flat array.
 *
 * Refusals: more frames or problems than max_frames, a size above max_width x max_height, more detection rows than max_frames * max_detections, more
 * object rows than max_frames * max_objects, more observations or keypoints than the handle was created for, or a negative count: OSLAM_E_CAPACITY
 * before anything is launched.  A matcher problem that does not fit (counts above max_detections / max_objects, rows or scores outside the arrays, a
 * broken precondition) gets a negative status[b] and nothing else of it is written; the other problems of the call are unaffected.  A frame record of
 * the histogram call that does not fit: OSLAM_E_CAPACITY / OSLAM_E_INVALID from the host entry point; the device entry point cannot read the
 * records and writes nothing for such a frame.  Problems of one call must not share `cur` rows or score entries; rows no problem owns keep what they
 * held.  The kernels use no atomics on global memory.
 * ---------------------------------------------------------------------------------------- */
#define OSLAM_OBJMATCH_BINS 94             /* 32 V + 32 S + 30 H (include/Frame.h:127) */
#define OSLAM_OBJMATCH_MAX_DETECTIONS 32   /* per frame */
#define OSLAM_OBJMATCH_DONE 0
#define OSLAM_OBJMATCH_REFUSED_RECORD (-1)           /* a count above the handle's, or a range outside the arrays */
#define OSLAM_OBJMATCH_REFUSED_NO_OBSERVATION (-2)   /* an object without observations */
#define OSLAM_OBJMATCH_REFUSED_NO_KEYPOINT (-3)      /* a detection without keypoints */
typedef struct oslam_objmatch oslam_objmatch_t;
typedef struct oslam_objmatch_params {   /* the literals of src/ObjectMatcher.cc:430, :783 and :789, as doubles: the reference compares floats against them */
    double min_similarity;   /* 0.8 */
    double min_iou;          /* 0.5 */
    double max_mean_dist;    /* 0.3; "5.0 for outdoor" by the reference's own comment */
    double max_min_dist;     /* 0.1 */
} oslam_objmatch_params_t;
typedef struct oslam_objmatch_frame {
    int32_t n_masks, mask_off;   /* masks mask_off .. mask_off + n_masks - 1 of the masks array (and of counts and hist) */
} oslam_objmatch_frame_t;
typedef struct oslam_objmatch_det_rows {   /* n_rows entries each; the device entry points take device pointers */
    int32_t n_rows;
    const int32_t* label;    /* Object2D::label (for `pre`: the Object3D's mLabel) */
    const float* hist;       /* [n_rows][94] mHSVHistogram */
    const float* box;        /* [n_rows][4] x, y, w, h; MatchTwoFrame only */
    int32_t* obj3d;          /* mvpObject3Ds as ids, negative = NULL; written for `cur` */
    const int32_t* kp_off;   /* MatchMapToFrame only: the detection's keypoints kp_off .. kp_off + kp_n - 1 of kps */
    const int32_t* kp_n;
    int32_t n_kps;
    const float* kps;        /* [n_kps][3] u, v (mvKeysUn) and z (mvDepth) */
} oslam_objmatch_det_rows_t;
typedef struct oslam_objmatch_obj_rows {
    int32_t n_rows;
    const int32_t* obj3d_id;   /* negative = NULL */
    const int32_t* label;      /* Object3D::mLabel */
    const int32_t* obs_off;    /* mvObservations = observations obs_off .. obs_off + obs_n - 1 */
    const int32_t* obs_n;
    int32_t n_obs;
    const float* obs_center;   /* [n_obs][3] ObjectObservation::ObjectCenterW */
    const float* obs_hist;     /* [n_obs][94] ObjectObservation::AppearanceVec */
} oslam_objmatch_obj_rows_t;
typedef struct oslam_objmatch_pair_problem {
    int32_t n_pre, off_pre;   /* the previous frame's objects: rows of `pre` */
    int32_t n_cur, off_cur;   /* the current frame's detections: rows of `cur` */
    int32_t off_score;        /* similarity and iou [n_pre][n_cur] start here */
    int32_t reserved[3];
} oslam_objmatch_pair_problem_t;
typedef struct oslam_objmatch_map_problem {
    int32_t n_cur, off_cur;   /* the frame's detections: rows of `cur` */
    int32_t n_obj, off_obj;   /* the map's objects: rows of the object rows */
    int32_t off_score;        /* similarity, mean_dist and min_dist [n_obj][n_cur] start here */
    int32_t reserved;
    float Rwc[9], Ow[3];      /* Frame::mRwc row-major, Frame::mOw */
    float fx, fy, cx, cy;
} oslam_objmatch_map_problem_t;
/* max_detections is per frame, 8 .. 32; max_width * max_height <= 2^29.  The handle keeps max_frames * ceil(max_height / 32) * max_detections * 94
 * int32 of partial counts.  Uses the current device.  OSLAM_E_HIP without a device: there is no CPU fallback. */
int oslam_objmatch_create(oslam_objmatch_t** out, int max_frames, int max_width, int max_height, int max_detections, int max_objects, int max_observations_total,
                          int max_keypoints_total);
void oslam_objmatch_destroy(oslam_objmatch_t* h);
/* Frame::ExtractHSVHistogramsFromMask (src/Frame.cc:388-414) of every mask of every frame.  Host pointers; one upload, two launches, one download,
 * synchronous.  images [n_frames][height][stride], masks [n_masks_total][height][mask_stride], counts and hist [n_masks_total][94]. */
int oslam_objmatch_hsv_histograms(oslam_objmatch_t* h, int n_frames, int width, int height, int stride, int mask_stride, const uint8_t* images, const oslam_objmatch_frame_t* frames,
                                  int n_masks_total, const uint8_t* masks, int32_t* counts, float* hist);
/* The same over device arrays (d_images 4-byte aligned), asynchronous on `stream`, no host synchronisation.  Calls on one handle must not overlap on
 * the device: the partial counts live in the handle. */
int oslam_objmatch_hsv_histograms_device(oslam_objmatch_t* h, int n_frames, int width, int height, int stride, int mask_stride, const uint8_t* d_images,
                                         const oslam_objmatch_frame_t* d_frames, int n_masks_total, const uint8_t* d_masks, int32_t* d_counts, float* d_hist, void* stream);
/* ObjectMatcher::MatchTwoFrame (src/ObjectMatcher.cc:47-440).  Host pointers; one upload, one launch, one download, synchronous.  cur->obj3d is read
 * and written; similarity and iou [n_scores]; n_assigned [n_problems]: the claims made; status [n_problems]: OSLAM_OBJMATCH_*. */
int oslam_objmatch_match_two_frame(oslam_objmatch_t* h, int n_problems, const oslam_objmatch_pair_problem_t* problems, const oslam_objmatch_det_rows_t* pre,
                                   const oslam_objmatch_det_rows_t* cur, const oslam_objmatch_params_t* params, int n_scores, float* similarity, float* iou, int32_t* n_assigned,
                                   int32_t* status);
/* The same over device arrays (pre, cur and params are host structs; the row pointers are device pointers), asynchronous on `stream`. */
int oslam_objmatch_match_two_frame_device(oslam_objmatch_t* h, int n_problems, const oslam_objmatch_pair_problem_t* d_problems, const oslam_objmatch_det_rows_t* pre,
                                          const oslam_objmatch_det_rows_t* cur, const oslam_objmatch_params_t* params, int n_scores, float* d_similarity, float* d_iou,
                                          int32_t* d_n_assigned, int32_t* d_status, void* stream);
/* ObjectMatcher::MatchMapToFrame (src/ObjectMatcher.cc:442-801).  n_by_similarity and n_by_distance [n_problems]: the claims of the rule of :783 and
 * of the rule of :789. */
int oslam_objmatch_match_map_to_frame(oslam_objmatch_t* h, int n_problems, const oslam_objmatch_map_problem_t* problems, const oslam_objmatch_det_rows_t* cur,
                                      const oslam_objmatch_obj_rows_t* objects, const oslam_objmatch_params_t* params, int n_scores, float* similarity, float* mean_dist,
                                      float* min_dist, int32_t* n_by_similarity, int32_t* n_by_distance, int32_t* status);
int oslam_objmatch_match_map_to_frame_device(oslam_objmatch_t* h, int n_problems, const oslam_objmatch_map_problem_t* d_problems, const oslam_objmatch_det_rows_t* cur,
                                             const oslam_objmatch_obj_rows_t* objects, const oslam_objmatch_params_t* params, int n_scores, float* d_similarity, float* d_mean_dist,
                                             float* d_min_dist, int32_t* d_n_by_similarity, int32_t* d_n_by_distance, int32_t* d_status, void* stream);
/* Measurement: with timing on, every later call records events before, between and after its launches on the call's stream;
 * oslam_objmatch_last_kernel_ms waits for the last call's events and gives the milliseconds of the counting kernel and of the combine pass of a
 * histogram call, or of the one kernel of a matcher call and 0. */
int oslam_objmatch_set_timing(oslam_objmatch_t* h, int on);
int oslam_objmatch_last_kernel_ms(oslam_objmatch_t* h, float ms[2]);

/* ------------------------------------------------------------------------------------------
 * Object map maintenance — what the reference does with an association once it has one: Object3D::RejectOutliers (src/ObjectTypes.cc:152-162) at the
 * end of Object3D::Update (:117-124) and inside Map::MergeObject (src/Map.cc:138-139), the new-object path of Tracking::UpdateCurrentObject
 * (src/Tracking.cc:1113-1199), Object3D::CalculateCenterAndSize (src/ObjectTypes.cc:805-833) and the merge sets of Map::ObjectMapRegularization
 * (src/Map.cc:47-112), for batches of independent objects and maps.  Operators: the driver does not call them; oslam_slam.h still takes the caller's
 * track_id and keeps Object3D::Update's list logic without the rejection.  PCL is not in the tree; what its Euclidean clustering computes is restated.
 *
 * Rows are map points: pos [.][3] float world position, label_cnt and label_sum int32 (the count of the object's label in the point's mLabelCnt and
 * the sum over all labels).  A problem (oslam_objmap_problem_t) is one point list: rows off .. off + n - 1 in list order, and a mode.
 *
 * 1. oslam_objmap_reject_outliers.  One sequential scan in list order (RejectOutliersTEST5 :590-628, RejectOutliersTEST7 :661-764, Tracking.cc:1120-1137):
 *     - mode UPDATE: a row is bad when GetLabelProb(mLabel) < 0.5 (:143-148, src/MapPoint.cc:109-137): (float)((double)label_cnt / (double)label_sum)
 *       compared against the double 0.5, probability 0 when label_sum == 0.  Bad rows are dropped.  Mode NEW_OBJECT has no bad test.
 *     - the other rows are the candidates: Center += PosW in float per component; square = (float)sqrt(x*x + y*y + z*z) with the squares and the sum
 *       in double (cv::norm); SquareSum = SquareSum + square * square in float.
 *     - Center = Center * (float)(1.0 / N) (Mat / double); CandidatesStdDev = (float)sqrt((double)SquareSum / (double)N - norm * norm) with norm the
 *       double cv::norm of Center.  This simplified variance cancels far from the origin and can be negative: the root is NaN and every
 *       `dist > 3 * StdDev` is false.
 *    Path TEST5 (mode UPDATE and n > 3000): a candidate is dropped when dist > 3.0f * StdDev, dist = (float)sqrt of the double sum of the squared float
 *    differences to Center.  Rows are streamed from global memory; n is unbounded.
 *    Path TEST7 (mode UPDATE and n <= 3000; mode NEW_OBJECT always): the candidates with finite coordinates are clustered as
 *    pcl::EuclideanClusterExtraction does with tolerance 0.1, minimum size 1, maximum 9999: the connected components of "d2 < (float)(0.1 * 0.1)",
 *    d2 = dx*dx + dy*dy + dz*dz in float in that order (FLANN L2_Simple<float>), strict.  A cluster with (double)(float)((double)size / (double)N) < 0.1
 *    and N > 15 is dropped whole; in every other cluster the 3-sigma rule above applies per point.  A candidate with a non-finite coordinate is in no
 *    cluster: no rule drops it.  Path SHORTCUT (mode NEW_OBJECT, one cluster, N > 5: Tracking.cc:1158): everything is kept.
 *    Per row: keep (uint8) and cluster (int32: the smallest row index, relative to the problem, of the row's component; -1 for a row in no cluster and
 *    on path TEST5).  Per problem an oslam_objmap_result_t; center and bbox are those of the kept rows (item 2) and stay untouched when nothing is kept.
 *    The clustering stages positions and one component label per point in LDS: n <= the handle's max_cluster_points.  Components are found by rounds of
 *    (every point takes the smallest label among its neighbours; every component root hooks onto the smallest label seen by its members; pointer
 *    jumping until every point names its root).  Roots that are no local minimum disappear each round, so a chain of any length needs O(log n) rounds;
 *    `rounds` reports them.  The outcome does not depend on the order of anything: results are bit-identical from run to run.
 *
 * 2. oslam_objmap_center_and_size (CalculateCenterAndSize :805-833) of every row of a problem: the float sum in list order divided by (float)n
 *    (Eigen::Vector3f / double), and per axis the minimum and maximum.  Writes n_kept = n, center and bbox of the result; nothing when n == 0.
 *    bbox is in the order of ObjectMatcher's BBox3D (src/ObjectMatcher.cc:838): max x, max y, max z, min x, min y, min z.
 *
 * 3. oslam_objmap_merge_sets (Map::ObjectMapRegularization src/Map.cc:67-100, CheckIfMerge :47-65, Compute3DOverlapRatio
 *    src/ObjectMatcher.cc:844-873).  A problem (oslam_objmap_merge_problem_t) is one map's objects in the caller's order (the adapter passes ascending
 *    mTrackID): rows label, track_id and bbox (bbox_stride floats from one row to the next, so that the array may be the bbox members of result
 *    records).  ratio [n][n] at off_pair, entries i < j written: the overlap ratio in float, std::max(a, b) = a < b ? b : a, std::min(a, b) = b < a ?
 *    b : a, 0 when an axis has min >= max.  Pair (i, j) merges when the labels are equal, the track ids differ and (double)ratio > 0.4.  The merging
 *    pairs are replayed in lexicographic order: a pair enters every existing set that holds either index, and opens a new set when there is none.
 *    Sets are not merged transitively; an index can sit in several.  member [.][n] uint8 at off_pair: rows 0 .. n_sets - 1 written; target [.] at
 *    off_obj: entries 0 .. n_sets - 1 written, the member of largest track_id, the first among equals (Map.cc:121-129).  n <= 128.
 *
 * Normalisations (readings of published sources that are not pinned here): the cv::norm, Mat / double, Eigen / double, L2_Simple and
 * non-finite rules above; std::sort of a list holding NaN is undefined: minimum and maximum start at +inf / -inf and move on a strict < / >, so NaN
 * is skipped and the first of equal values stays; every NaN written is the quiet NaN 0x7fc00000; MergeObject's MaxTrackID starts at -1, so a set of
 * negative track ids has no defined target: the first member.
 *
 * Refusals: more problems than max_problems or a negative count: OSLAM_E_CAPACITY; NULL pointers: OSLAM_E_INVALID.  The host entry points read the
 * records: a negative n, an unknown mode or rows outside the arrays are OSLAM_E_INVALID, a clustering problem above max_cluster_points or a map above
 * max_objects OSLAM_E_CAPACITY, before anything is launched.  The device entry points cannot: such a problem gets a negative status and nothing else
 * of it is written.  Problems of one call must not share rows; rows no problem owns are never written.  No atomics on global memory.
 * ---------------------------------------------------------------------------------------- */
#define OSLAM_OBJMAP_MODE_UPDATE 0        /* Object3D::RejectOutliers */
#define OSLAM_OBJMAP_MODE_NEW_OBJECT 1    /* Tracking::UpdateCurrentObject's new-object path */
#define OSLAM_OBJMAP_PATH_TEST5 0
#define OSLAM_OBJMAP_PATH_TEST7 1
#define OSLAM_OBJMAP_PATH_SHORTCUT 2
#define OSLAM_OBJMAP_TEST5_ABOVE 3000     /* src/ObjectTypes.cc:154 */
#define OSLAM_OBJMAP_MIN_CLUSTER_POINTS 3000
#define OSLAM_OBJMAP_MAX_CLUSTER_POINTS 4000   /* 16 bytes of LDS per point */
#define OSLAM_OBJMAP_MAX_OBJECTS 128      /* per map: a set is a lane of one wavefront, its members two 64-bit words */
#define OSLAM_OBJMAP_DONE 0
#define OSLAM_OBJMAP_REFUSED_RECORD (-1)     /* a negative n, an unknown mode, rows outside the arrays */
#define OSLAM_OBJMAP_REFUSED_CAPACITY (-2)   /* a clustering problem above max_cluster_points, a map above max_objects */
typedef struct oslam_objmap oslam_objmap_t;
typedef struct oslam_objmap_problem {
    int32_t off, n;   /* rows off .. off + n - 1, in list order */
    int32_t mode;     /* OSLAM_OBJMAP_MODE_* (center_and_size ignores it) */
    int32_t reserved;
} oslam_objmap_problem_t;
typedef struct oslam_objmap_result {
    int32_t status;        /* OSLAM_OBJMAP_* */
    int32_t n_candidates, n_clusters, n_kept;
    int32_t path;          /* OSLAM_OBJMAP_PATH_* */
    int32_t rounds;        /* of the component search */
    float std_dev, candidates_center[3];
    float center[3], bbox[6];   /* of the kept rows; max x, y, z, min x, y, z */
    int32_t reserved;
} oslam_objmap_result_t;
typedef struct oslam_objmap_merge_problem {
    int32_t n, off_obj;   /* the map's objects: rows off_obj .. off_obj + n - 1; target entries from off_obj */
    int32_t off_pair;     /* ratio [n][n] floats and member [.][n] bytes start here */
    int32_t reserved;
} oslam_objmap_merge_problem_t;
/* max_cluster_points 3000 .. 4000, max_objects 1 .. 128.  Uses the current device.  OSLAM_E_HIP without a device: there is no CPU fallback. */
int oslam_objmap_create(oslam_objmap_t** out, int max_problems, int max_cluster_points, int max_objects);
void oslam_objmap_destroy(oslam_objmap_t* h);
/* Item 1.  Host pointers; one upload, one launch, one download, synchronous.  pos [n_rows][3], label_cnt, label_sum, keep, cluster [n_rows] (the label
 * arrays may be NULL when every problem is of mode NEW_OBJECT), results [n_problems]. */
int oslam_objmap_reject_outliers(oslam_objmap_t* h, int n_problems, const oslam_objmap_problem_t* problems, int n_rows, const float* pos, const int32_t* label_cnt,
                                 const int32_t* label_sum, uint8_t* keep, int32_t* cluster, oslam_objmap_result_t* results);
/* The same over device arrays, asynchronous on `stream`, no host synchronisation.  The records cannot be read here, so the label arrays are required. */
int oslam_objmap_reject_outliers_device(oslam_objmap_t* h, int n_problems, const oslam_objmap_problem_t* d_problems, int n_rows, const float* d_pos, const int32_t* d_label_cnt,
                                        const int32_t* d_label_sum, uint8_t* d_keep, int32_t* d_cluster, oslam_objmap_result_t* d_results, void* stream);
/* Item 2. */
int oslam_objmap_center_and_size(oslam_objmap_t* h, int n_problems, const oslam_objmap_problem_t* problems, int n_rows, const float* pos, oslam_objmap_result_t* results);
int oslam_objmap_center_and_size_device(oslam_objmap_t* h, int n_problems, const oslam_objmap_problem_t* d_problems, int n_rows, const float* d_pos,
                                        oslam_objmap_result_t* d_results, void* stream);
/* Item 3.  label, track_id, target [n_rows]; bbox: row r at bbox + r * bbox_stride floats, bbox_stride >= 6; ratio [n_pairs] float and member [n_pairs]
 * uint8; n_sets and status [n_problems]. */
int oslam_objmap_merge_sets(oslam_objmap_t* h, int n_problems, const oslam_objmap_merge_problem_t* problems, int n_rows, const int32_t* label, const int32_t* track_id,
                            const float* bbox, int bbox_stride, int n_pairs, float* ratio, uint8_t* member, int32_t* target, int32_t* n_sets, int32_t* status);
int oslam_objmap_merge_sets_device(oslam_objmap_t* h, int n_problems, const oslam_objmap_merge_problem_t* d_problems, int n_rows, const int32_t* d_label,
                                   const int32_t* d_track_id, const float* d_bbox, int bbox_stride, int n_pairs, float* d_ratio, uint8_t* d_member, int32_t* d_target,
                                   int32_t* d_n_sets, int32_t* d_status, void* stream);
/* Measurement, as oslam_objmatch_set_timing: the milliseconds of the last call's one kernel, and 0. */
int oslam_objmap_set_timing(oslam_objmap_t* h, int on);
int oslam_objmap_last_kernel_ms(oslam_objmap_t* h, float ms[2]);

#ifdef __cplusplus
}
#endif
#endif /* OSLAM_HIP_H */
