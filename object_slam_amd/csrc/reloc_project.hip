// reloc_project.hip — ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist) (reference
// src/ORBmatcher.cc:1472-1599), the projection search of Tracking::Relocalization (src/Tracking.cc:1717, :1731), for batches of independent problems on gfx950
// (include/oslam_hip.h, "Relocalisation projection").  One launch, one workgroup per problem: the workgroup stages the FRAME in LDS (the same grid and
// visiting order as a keyframe's) and its threads stride over the keyframe's map-point slots, which stay in global memory.  The sequential claims of :1541 /
// :1557 are reproduced with claim_fixpoint; the rotation histogram (:1577-1596) runs once on the final claims, so a match it removes has still blocked the
// slots after it.  The staging, the level, the window walk, the claims and the handle are window_search.h's (shared with sim3_match.hip and
// sim3_project.hip); the gates of a slot, ORBdist and the histogram's use are here.
// No inter-workgroup synchronisation and no atomics on global memory: the result does not depend on the order the hardware runs anything in (the LDS
// atomics are minima and counts).  The roundings are those the header lists.  Product code; never includes oracle/.
#include <climits>
#include <cmath>
#include <mutex>

#include "common.h"
#include "stage_layout.h"
#include "window_search.h"

using oslam::set_error;
using namespace oslam::kf_stage;   // the staged frame, the window search, the claims and gemm_row

struct oslam_reloc_proj : ProjHandle {};

namespace {

struct RelocArgs {
    const oslam_reloc_proj_problem_t* problems;
    int n_problems, n_pt_out, n_kp_out, ncap;
    oslam_reloc_proj_frame_rows_t fr;
    oslam_reloc_proj_pt_rows_t pts;
    const uint8_t* skip;
    uint32_t* cache;
    int32_t* matched;   // [n_kp_out]
    int32_t* count;     // n_matches
    int32_t* removed;   // may be NULL
    int32_t* passes;    // may be NULL
    WindowCam cam;
    int check_ori;
};

struct Pose { float Rcw[9], tcw[3], Ow[3], th; int orbdist; };

// One slot through the gates of :1496-1526 and the window (:1528-1553).  Returns bestIdx2 of an accepted slot (bestDist <= ORBdist), else -1.
// Under the claims `claim`, with the cache line `cache` or NULL (nearest_unclaimed).
__device__ int evaluate(const RelocArgs& a, const Staged& s, const float* s_scale, const Pose& T, size_t o, int i, const int* claim, uint32_t* cache) {
    const WindowCam& c = a.cam;
    const float X[3] = {a.pts.Xw[3 * o], a.pts.Xw[3 * o + 1], a.pts.Xw[3 * o + 2]};
    const float xc = gemm_row(T.Rcw, X, T.tcw[0]), yc = gemm_row(T.Rcw + 3, X, T.tcw[1]), zc = gemm_row(T.Rcw + 6, X, T.tcw[2]);
    const float invzc = (float)(1.0 / (double)zc);   // (no test of the sign of z, :1502)
    const float u = c.fx * xc * invzc + c.cx, v = c.fy * yc * invzc + c.cy;
    if (u < c.minX || u > c.maxX) return -1;   // inclusive on both sides (:1507-1510)
    if (v < c.minY || v > c.maxY) return -1;
    if (!(isfinite(u) && isfinite(v))) return -1;   // a NaN passes the comparisons above and finds nothing in GetFeaturesInArea
    const float mfMax = a.pts.maxDistance[o];
    const float maxDistance = 1.2f * mfMax, minDistance = 0.8f * a.pts.minDistance[o];
    const float PO[3] = {X[0] - T.Ow[0], X[1] - T.Ow[1], X[2] - T.Ow[2]};
    const float dist = (float)sqrt(((double)PO[0] * (double)PO[0] + (double)PO[1] * (double)PO[1]) + (double)PO[2] * (double)PO[2]);   // cv::norm
    if (dist < minDistance || dist > maxDistance) return -1;
    // Frame::GetFeaturesInArea (src/Frame.cc:567-620) with minLevel = level - 1, maxLevel = level + 1
    const int level = predict_level(mfMax, dist, c);
    return nearest_unclaimed<-1, 1>(s, c, u, v, T.th * s_scale[level], level, a.pts.desc + o * 32, T.orbdist, i, claim, cache);
}

__global__ __launch_bounds__(kThreads) void k_reloc_project(RelocArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const oslam_reloc_proj_problem_t& P = a.problems[b];
    const int n_kp = P.n_kp, kp_off = P.kp_off, n_pts = P.n_pts, pt_off = P.pt_off, kp_out = P.kp_out_off, pt_out = P.pt_out_off;
    // a record that does not fit the handle or the arrays: -2, nothing else is written (the host-pointer entry point refuses the call instead)
    const ProjExtent ext = {a.ncap, a.fr.n_rows, a.pts.n_rows, a.n_kp_out, a.n_pt_out, true};
    const bool fits = record_counts_fit(P, ext) && record_lies_inside(P, ext) && P.ORBdist >= 0 && P.ORBdist <= 255;
    if (!fits) {
        if (tid == 0) a.count[b] = -2;
        return;
    }
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 12; i++) finite = finite && isfinite(P.Tcw[i]);
    if (!finite) {
        for (int i = tid; i < n_kp; i += kThreads) a.matched[kp_out + i] = -1;
        if (tid == 0) {
            a.count[b] = -1;
            if (a.removed) a.removed[b] = 0;
            if (a.passes) a.passes[b] = 0;
        }
        return;
    }
    Pose T;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int k = 0; k < 3; k++) T.Rcw[3 * r + k] = P.Tcw[4 * r + k];
        T.tcw[r] = P.Tcw[4 * r + 3];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) T.Ow[i] = -(T.Rcw[i] * T.tcw[0] + T.Rcw[3 + i] * T.tcw[1] + T.Rcw[6 + i] * T.tcw[2]);   // :1478
    T.th = P.th;
    T.orbdist = P.ORBdist;

    extern __shared__ __align__(16) uint8_t smem[];
    const Lds s = carve(smem, a.ncap);
    int* c_prev = s.v0;   // [ncap] the lowest slot that claimed the keypoint in the pass before
    int* c_cur = s.v1;    // [ncap] the same of the running pass
    __shared__ int s_wtot[kThreads / 64];
    __shared__ float s_scale[OSLAM_MAX_LEVELS];
    __shared__ int s_hist[kHistoLen], s_ind[3];
    __shared__ int s_count, s_removed, s_changed;

    const uint8_t* has_mp = a.fr.has_mp + kp_off;
    const uint8_t* skip = a.skip ? a.skip + pt_out : nullptr;
    if (tid < OSLAM_MAX_LEVELS) s_scale[tid] = a.cam.scale[tid];
    if (tid < kHistoLen) s_hist[tid] = 0;
    if (tid == 0) { s_count = 0; s_removed = 0; }
    const auto occupied = [&](int k) { return has_mp[k] != 0; };   // mvpMapPoints[k] on entry (:1541)
    reset_claims(c_prev, n_kp, occupied);
    // (stage_target begins and ends with a barrier)
    stage_target(s, a.fr.keysUn + kp_off, a.fr.desc + (size_t)kp_off * 32, n_kp, a.cam, s_wtot);

    // ---- the search: fixpoint over the sequential claim order (:1541, :1557) ----
    const int passes = claim_fixpoint(n_kp, n_pts, c_prev, c_cur, a.cache + (size_t)pt_out * kCacheWords, &s_changed, occupied, [&](int i, const int* claim, uint32_t* cl) {
        return (skip && skip[i]) ? -1 : evaluate(a, s, s_scale, T, (size_t)pt_off + i, i, claim, cl);
    });

    // ---- mvpMapPoints after the loop: every accepted slot claimed a keypoint of its own; rotation consistency (:1577-1596) ----
    const oslam_keypoint_t* keys = a.fr.keysUn + kp_off;
    const float* kf_angle = a.pts.kf_angle + pt_off;
    if (a.check_ori) {
        for (int k = tid; k < n_kp; k += kThreads) {
            const int o = c_cur[k];
            if (is_claimed(o)) {
                const int bin = rot_bin(kf_angle[o], keys[k].angle);
                if (bin >= 0) atomicAdd(&s_hist[bin], 1);
            }
        }
        __syncthreads();
        if (tid == 0) three_maxima(s_hist, s_ind);
        __syncthreads();
    }
    int removed = 0;
    const int found = write_claims(c_cur, n_kp, a.matched + kp_out, [&](int k, int o) {
        if (!a.check_ori) return true;
        const int bin = rot_bin(kf_angle[o], keys[k].angle);
        if (bin >= 0 && (bin == s_ind[0] || bin == s_ind[1] || bin == s_ind[2])) return true;
        removed++;
        return false;
    });
    if (found) atomicAdd(&s_count, found);
    if (removed) atomicAdd(&s_removed, removed);
    __syncthreads();
    if (tid == 0) {
        a.count[b] = s_count;
        if (a.removed) a.removed[b] = s_removed;
        if (a.passes) a.passes[b] = passes;
    }
}

int check_call(const char* fn, const oslam_reloc_proj* h, int n_problems, const oslam_reloc_proj_frame_rows_t* fr, const oslam_reloc_proj_pt_rows_t* pts, int n_pt_out, int n_kp_out,
               const oslam_camera_t* cam, const float* bounds, const float* scaleFactors, int nlevels, float logScaleFactor) {
    OSLAM_CHECK(check_proj_call(fn, h, n_problems, fr, "frame", pts, n_pt_out, "skip", n_kp_out, cam, bounds, scaleFactors, nlevels, logScaleFactor));
    if (fr->n_rows > 0 && (!fr->keysUn || !fr->desc || !fr->has_mp)) { set_error("%s: a per-keypoint array is NULL", fn); return OSLAM_E_INVALID; }
    if (pts->n_rows > 0 && (!pts->Xw || !pts->desc || !pts->maxDistance || !pts->minDistance || !pts->kf_angle)) { set_error("%s: a per-point array is NULL", fn); return OSLAM_E_INVALID; }
    return OSLAM_OK;
}

// The device entry point: checks, the argument block, one launch
int launch(const char* fn, oslam_reloc_proj* h, int n_problems, const oslam_reloc_proj_problem_t* d_problems, const oslam_reloc_proj_frame_rows_t* fr,
           const oslam_reloc_proj_pt_rows_t* pts, int n_pt_out, const uint8_t* d_skip, int n_kp_out, const oslam_camera_t* cam, const float* bounds, const float* scaleFactors,
           int nlevels, float logScaleFactor, int check_orientation, int32_t* d_matched, int32_t* d_count, int32_t* d_removed, int32_t* d_passes, void* stream) {
    OSLAM_CHECK(check_call(fn, h, n_problems, fr, pts, n_pt_out, n_kp_out, cam, bounds, scaleFactors, nlevels, logScaleFactor));
    if (n_problems == 0) return OSLAM_OK;
    if (!d_problems || !d_count || (n_kp_out > 0 && !d_matched)) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    RelocArgs a;
    a.problems = d_problems; a.n_problems = n_problems; a.n_pt_out = n_pt_out; a.n_kp_out = n_kp_out; a.ncap = h->max_kps;
    a.fr = *fr; a.pts = *pts; a.skip = d_skip; a.cache = h->cache.as<uint32_t>();
    a.matched = d_matched; a.count = d_count; a.removed = d_removed; a.passes = d_passes;
    fill_window_cam(a.cam, cam, bounds, scaleFactors, nlevels, logScaleFactor);
    a.check_ori = check_orientation ? 1 : 0;
    hipLaunchKernelGGL(k_reloc_project, dim3(n_problems), dim3(kThreads), h->lds, (hipStream_t)stream, a);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

}  // namespace

extern "C" {

void oslam_reloc_proj_destroy(oslam_reloc_proj_t* h) {
    if (!h) return;
    delete h;
}

int oslam_reloc_proj_create(oslam_reloc_proj_t** out, int max_problems, int max_keypoints, int max_points_total, int device) {
    return create_proj("oslam_reloc_proj_create", "the frame's", out, max_problems, max_keypoints, max_points_total, device, {(const void*)k_reloc_project});
}

int oslam_match_search_by_projection_reloc_batch_device(oslam_reloc_proj_t* h, int n_problems, const oslam_reloc_proj_problem_t* d_problems,
                                                        const oslam_reloc_proj_frame_rows_t* frame, const oslam_reloc_proj_pt_rows_t* pts, int n_pt_out, const uint8_t* d_skip,
                                                        int n_kp_out, const oslam_camera_t* cam, const float bounds[4], const float* scaleFactors, int nlevels,
                                                        float logScaleFactor, int check_orientation, int32_t* d_matched, int32_t* d_n_matches, int32_t* d_n_removed,
                                                        int32_t* d_n_passes, void* stream) {
    return launch("oslam_match_search_by_projection_reloc_batch_device", h, n_problems, d_problems, frame, pts, n_pt_out, d_skip, n_kp_out, cam, bounds, scaleFactors, nlevels,
                  logScaleFactor, check_orientation, d_matched, d_n_matches, d_n_removed, d_n_passes, stream);
}

// The host-pointer entry point: the records checked, one block up, launch(), the outputs down
int oslam_match_search_by_projection_reloc_batch(oslam_reloc_proj_t* h, int n_problems, const oslam_reloc_proj_problem_t* problems, const oslam_reloc_proj_frame_rows_t* fr,
                                                 const oslam_reloc_proj_pt_rows_t* pts, int n_pt_out, const uint8_t* skip, int n_kp_out, const oslam_camera_t* cam,
                                                 const float bounds[4], const float* scaleFactors, int nlevels, float logScaleFactor, int check_orientation, int32_t* matched,
                                                 int32_t* n_matches, int32_t* n_removed, int32_t* n_passes) {
    const char* fn = "oslam_match_search_by_projection_reloc_batch";
    OSLAM_CHECK(check_call(fn, h, n_problems, fr, pts, n_pt_out, n_kp_out, cam, bounds, scaleFactors, nlevels, logScaleFactor));
    if (n_problems == 0) return OSLAM_OK;
    if (!problems || !n_matches || (n_kp_out > 0 && !matched)) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_CHECK(check_proj_records(fn, problems, n_problems, ProjExtent{h->max_kps, fr->n_rows, pts->n_rows, n_kp_out, n_pt_out, true}, "frame",
                                   [&](int b, const oslam_reloc_proj_problem_t& P) {
        if (P.ORBdist >= 0 && P.ORBdist <= 255) return OSLAM_OK;
        set_error("%s: problem %d has ORBdist %d outside 0 .. 255 (with every candidate claimed the reference would write mvpMapPoints[-1])", fn, b, P.ORBdist);
        return OSLAM_E_INVALID;
    }));
    std::lock_guard<std::mutex> lock(h->mu);
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t np = (size_t)n_problems, K = (size_t)fr->n_rows, M = (size_t)pts->n_rows, NO = (size_t)n_pt_out, NK = (size_t)n_kp_out;
    oslam::StageLayout lay;   // one block, inputs then outputs: one upload, one download
    const auto fProb = lay.add<oslam_reloc_proj_problem_t>(np);
    const auto fKeys = lay.add<oslam_keypoint_t>(K);
    const auto fDesc = lay.add<uint8_t>(K * 32), fHas = lay.add<uint8_t>(K);
    const auto fXw = lay.add<float>(M * 3);
    const auto fPd = lay.add<uint8_t>(M * 32);
    const auto fMax = lay.add<float>(M), fMin = lay.add<float>(M), fAng = lay.add<float>(M);
    const auto fSkip = lay.add<uint8_t>(NO, skip != nullptr);
    const auto fOut = lay.add<int32_t>(NK), fCount = lay.add<int32_t>(np), fRem = lay.add<int32_t>(np, n_removed != nullptr), fPass = lay.add<int32_t>(np, n_passes != nullptr);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fProb, ph, problems); put(fKeys, ph, fr->keysUn); put(fDesc, ph, fr->desc); put(fHas, ph, fr->has_mp); put(fXw, ph, pts->Xw); put(fPd, ph, pts->desc);
    put(fMax, ph, pts->maxDistance); put(fMin, ph, pts->minDistance); put(fAng, ph, pts->kf_angle); put(fSkip, ph, skip);
    // the caller's output rows travel too: rows no problem owns, and those of a problem the kernel leaves alone, come back as they were
    put(fOut, ph, (const int32_t*)matched); put(fCount, ph, (const int32_t*)n_matches); put(fRem, ph, (const int32_t*)n_removed); put(fPass, ph, (const int32_t*)n_passes);
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, nullptr));
    const oslam_reloc_proj_frame_rows_t df = {fr->n_rows, at(fKeys, pd), at(fDesc, pd), at(fHas, pd)};
    const oslam_reloc_proj_pt_rows_t dp = {pts->n_rows, at(fXw, pd), at(fPd, pd), at(fMax, pd), at(fMin, pd), at(fAng, pd)};
    OSLAM_CHECK(launch(fn, h, n_problems, at(fProb, pd), &df, &dp, n_pt_out, at(fSkip, pd), n_kp_out, cam, bounds, scaleFactors, nlevels, logScaleFactor, check_orientation,
                       at(fOut, pd), at(fCount, pd), at(fRem, pd), at(fPass, pd), nullptr));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fOut.off, pd + fOut.off, lay.total() - fOut.off, hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(fOut, ph, matched); get(fCount, ph, n_matches); get(fRem, ph, n_removed); get(fPass, ph, n_passes);
    return OSLAM_OK;
}

}  // extern "C"
