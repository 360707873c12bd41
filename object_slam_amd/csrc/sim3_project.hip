// sim3_project.hip — ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (reference src/ORBmatcher.cc:290-403) and ORBmatcher::Fuse(pKF, Scw,
// vpPoints, th, vpReplacePoint) (:977-1100) for batches of independent problems on gfx950 (include/oslam_hip.h, "Sim3 projection").  One launch, one
// workgroup per problem: the workgroup stages the keyframe in LDS and its threads stride over the problem's candidate points, which stay in global memory.
// The search reproduces the sequential claims of :375 / :396 with claim_fixpoint; Fuse has no claims, takes one pass and reports the surgery of :1084-1094
// instead of performing it.  The staging, the level, the window walk, the claims and the handle are window_search.h's (shared with sim3_match.hip and
// reloc_project.hip); the gates of a point, the pose and Fuse's bookkeeping are here.
// No inter-workgroup synchronisation and no atomics on global memory: the result does not depend on the order the hardware runs anything in.
// The roundings are those the header lists.  Product code; never includes oracle/.
#include <climits>
#include <cmath>
#include <mutex>

#include "common.h"
#include "stage_layout.h"
#include "window_search.h"

using oslam::set_error;
using namespace oslam::kf_stage;   // the staged keyframe, the window search, the claims and gemm_row

struct oslam_sim3_proj : ProjHandle {};

namespace {

constexpr int kThLow = 50;      // ORBmatcher::TH_LOW, src/ORBmatcher.cc:37

struct ProjArgs {
    const oslam_sim3_proj_problem_t* problems;
    int n_problems, n_pt_out, n_kp_out, ncap;
    oslam_sim3_proj_kf_rows_t kf;
    oslam_sim3_proj_pt_rows_t pts;
    const uint8_t* skip;
    uint32_t* cache;
    int32_t* out0;     // search: matched [n_kp_out]; Fuse: fused_kp [n_pt_out]
    int32_t* out1;     // Fuse: replace [n_pt_out]
    int32_t* count;    // n_matches / n_fused
    int32_t* passes;   // search, may be NULL
    WindowCam cam;
};

struct Pose { float Rcw[9], tcw[3], Ow[3], th; };

// One point through the gates of :312-365 / :1000-1054 and the window (:367-392 / :1056-1079).  Returns bestIdx of an accepted point (bestDist <= TH_LOW), else -1.
// Search: under the claims `claim`, with the cache line `cache` or NULL (nearest_unclaimed).
template <bool kFuse>
__device__ int evaluate(const ProjArgs& a, const Staged& s, const float* s_scale, const Pose& T, size_t o, int i, const int* claim, uint32_t* cache) {
    const WindowCam& c = a.cam;
    const float X[3] = {a.pts.Xw[3 * o], a.pts.Xw[3 * o + 1], a.pts.Xw[3 * o + 2]};
    const float Pc[3] = {gemm_row(T.Rcw, X, T.tcw[0]), gemm_row(T.Rcw + 3, X, T.tcw[1]), gemm_row(T.Rcw + 6, X, T.tcw[2])};
    if (Pc[2] < 0.0f) return -1;
    const float invz = (float)(1.0 / (double)Pc[2]);
    const float x = Pc[0] * invz, y = Pc[1] * invz;
    const float u = c.fx * x + c.cx, v = c.fy * y + c.cy;
    if (!(u >= c.minX && u < c.maxX && v >= c.minY && v < c.maxY)) return -1;   // KeyFrame::IsInImage (src/KeyFrame.cc:610)
    const float mfMax = a.pts.maxDistance[o];
    const float maxDistance = 1.2f * mfMax, minDistance = 0.8f * a.pts.minDistance[o];
    const float PO[3] = {X[0] - T.Ow[0], X[1] - T.Ow[1], X[2] - T.Ow[2]};
    const float dist = (float)sqrt(((double)PO[0] * (double)PO[0] + (double)PO[1] * (double)PO[1]) + (double)PO[2] * (double)PO[2]);   // cv::norm
    if (dist < minDistance || dist > maxDistance) return -1;
    const float Pn[3] = {a.pts.normal[3 * o], a.pts.normal[3 * o + 1], a.pts.normal[3 * o + 2]};
    const double dot = ((double)PO[0] * (double)Pn[0] + (double)PO[1] * (double)Pn[1]) + (double)PO[2] * (double)Pn[2];
    if (dot < 0.5 * (double)dist) return -1;
    const int level = predict_level(mfMax, dist, c);
    const float r = T.th * s_scale[level];
    const uint8_t* desc = a.pts.desc + o * 32;
    if (!kFuse) return nearest_unclaimed<-1, 0>(s, c, u, v, r, level, desc, kThLow, i, claim, cache);
    const Nearest best = nearest_in_window<-1, 0>(s, c, u, v, r, level, desc);
    return best.dist <= kThLow ? best.idx : -1;
}

template <bool kFuse>
__global__ __launch_bounds__(kThreads) void k_sim3_project(ProjArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const oslam_sim3_proj_problem_t& P = a.problems[b];
    const int n_kp = P.n_kp, kp_off = P.kp_off, n_pts = P.n_pts, pt_off = P.pt_off, kp_out = P.kp_out_off, pt_out = P.pt_out_off;
    // a record that does not fit the handle or the arrays: -2, nothing else is written (the host-pointer entry points refuse the call instead)
    const ProjExtent ext = {a.ncap, a.kf.n_rows, a.pts.n_rows, a.n_kp_out, a.n_pt_out, !kFuse};
    if (!(record_counts_fit(P, ext) && record_lies_inside(P, ext))) {
        if (tid == 0) a.count[b] = -2;
        return;
    }
    // Scw = [s R | s t] (:299-303)
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 12; i++) finite = finite && isfinite(P.Scw[i]);
    const float scw = (float)sqrt(((double)P.Scw[0] * (double)P.Scw[0] + (double)P.Scw[1] * (double)P.Scw[1]) + (double)P.Scw[2] * (double)P.Scw[2]);
    if (!(finite && isfinite(scw) && scw > 0.0f)) {
        if (kFuse) {
            for (int i = tid; i < n_pts; i += kThreads) { a.out0[pt_out + i] = -1; a.out1[pt_out + i] = -1; }
        } else {
            for (int i = tid; i < n_kp; i += kThreads) a.out0[kp_out + i] = -1;
            if (tid == 0 && a.passes) a.passes[b] = 0;
        }
        if (tid == 0) a.count[b] = -1;
        return;
    }
    Pose T;
    const double inv = 1.0 / (double)scw;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int k = 0; k < 3; k++) T.Rcw[3 * r + k] = (float)((double)P.Scw[4 * r + k] * inv);
        T.tcw[r] = (float)((double)P.Scw[4 * r + 3] * inv);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) T.Ow[i] = -(T.Rcw[i] * T.tcw[0] + T.Rcw[3 + i] * T.tcw[1] + T.Rcw[6 + i] * T.tcw[2]);
    T.th = P.th;

    extern __shared__ __align__(16) uint8_t smem[];
    const Lds s = carve(smem, a.ncap);
    int* c_prev = s.v0;   // [ncap] search: the lowest point that claimed the keypoint in the pass before; Fuse: the first point added there
    int* c_cur = s.v1;    // [ncap] search: the same of the running pass
    __shared__ int s_wtot[kThreads / 64];
    __shared__ float s_scale[OSLAM_MAX_LEVELS];
    __shared__ int s_count, s_changed;

    const uint8_t* state = a.kf.state + kp_off;
    const uint8_t* skip = a.skip ? a.skip + pt_out : nullptr;
    if (tid < OSLAM_MAX_LEVELS) s_scale[tid] = a.cam.scale[tid];
    if (tid == 0) s_count = 0;
    const auto occupied = [&](int k) { return !kFuse && state[k]; };   // vpMatched[k] on entry (:375)
    reset_claims(c_prev, n_kp, occupied);
    // (stage_target begins and ends with a barrier)
    stage_target(s, a.kf.keysUn + kp_off, a.kf.desc + (size_t)kp_off * 32, n_kp, a.cam, s_wtot);

    if (kFuse) {
        int32_t* fused_kp = a.out0 + pt_out;
        int32_t* replace = a.out1 + pt_out;
        int fused = 0;
        for (int i = tid; i < n_pts; i += kThreads) {
            const int k = (skip && skip[i]) ? -1 : evaluate<true>(a, s, s_scale, T, (size_t)pt_off + i, i, nullptr, nullptr);
            fused_kp[i] = k;
            if (k >= 0) {
                fused++;
                if (state[k] == 0) atomicMin(&c_prev[k], i);   // AddMapPoint (:1093): the first accepted point of the list stays there
            }
        }
        if (fused) atomicAdd(&s_count, fused);
        __syncthreads();
        for (int i = tid; i < n_pts; i += kThreads) {
            const int k = fused_kp[i];   // (this thread wrote it)
            int rep = -1;
            if (k >= 0) {
                const int st = state[k];
                if (st == 0) rep = c_prev[k] == i ? OSLAM_FUSE_ADDED : c_prev[k];
                else if (st == 1) rep = OSLAM_FUSE_OCCUPANT;   // (a bad occupant, :1087: nothing is written, the point still counts)
            }
            replace[i] = rep;
        }
        if (tid == 0) a.count[b] = s_count;
        return;
    }

    // ---- the search: fixpoint over the sequential claim order (:375, :396) ----
    const int passes = claim_fixpoint(n_kp, n_pts, c_prev, c_cur, a.cache + (size_t)pt_out * kCacheWords, &s_changed, occupied, [&](int i, const int* claim, uint32_t* cl) {
        return (skip && skip[i]) ? -1 : evaluate<false>(a, s, s_scale, T, (size_t)pt_off + i, i, claim, cl);
    });
    // vpMatched after the loop: every accepted point claimed a keypoint of its own
    const int found = write_claims(c_cur, n_kp, a.out0 + kp_out, [](int, int) { return true; });
    if (found) atomicAdd(&s_count, found);
    __syncthreads();
    if (tid == 0) {
        a.count[b] = s_count;
        if (a.passes) a.passes[b] = passes;
    }
}

int check_call(const char* fn, const oslam_sim3_proj* h, int n_problems, const oslam_sim3_proj_kf_rows_t* kf, const oslam_sim3_proj_pt_rows_t* pts, int n_pt_out, int n_kp_out,
               const oslam_camera_t* cam, const float* bounds, const float* scaleFactors, int nlevels, float logScaleFactor) {
    OSLAM_CHECK(check_proj_call(fn, h, n_problems, kf, "keyframe", pts, n_pt_out, "point output", n_kp_out, cam, bounds, scaleFactors, nlevels, logScaleFactor));
    if (kf->n_rows > 0 && (!kf->keysUn || !kf->desc || !kf->state)) { set_error("%s: a per-keypoint array is NULL", fn); return OSLAM_E_INVALID; }
    if (pts->n_rows > 0 && (!pts->Xw || !pts->normal || !pts->desc || !pts->maxDistance || !pts->minDistance)) { set_error("%s: a per-point array is NULL", fn); return OSLAM_E_INVALID; }
    return OSLAM_OK;
}

// Both device entry points: checks, the argument block, one launch
int launch(const char* fn, bool fuse, oslam_sim3_proj* h, int n_problems, const oslam_sim3_proj_problem_t* d_problems, const oslam_sim3_proj_kf_rows_t* kf,
           const oslam_sim3_proj_pt_rows_t* pts, int n_pt_out, const uint8_t* d_skip, int n_kp_out, const oslam_camera_t* cam, const float* bounds, const float* scaleFactors,
           int nlevels, float logScaleFactor, int32_t* d_out0, int32_t* d_out1, int32_t* d_count, int32_t* d_passes, void* stream) {
    OSLAM_CHECK(check_call(fn, h, n_problems, kf, pts, n_pt_out, n_kp_out, cam, bounds, scaleFactors, nlevels, logScaleFactor));
    if (n_problems == 0) return OSLAM_OK;
    const int n_out0 = fuse ? n_pt_out : n_kp_out;
    if (!d_problems || !d_count || (n_out0 > 0 && !d_out0) || (fuse && n_pt_out > 0 && !d_out1)) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    ProjArgs a;
    a.problems = d_problems; a.n_problems = n_problems; a.n_pt_out = n_pt_out; a.n_kp_out = n_kp_out; a.ncap = h->max_kps;
    a.kf = *kf; a.pts = *pts; a.skip = d_skip; a.cache = h->cache.as<uint32_t>();
    a.out0 = d_out0; a.out1 = d_out1; a.count = d_count; a.passes = d_passes;
    fill_window_cam(a.cam, cam, bounds, scaleFactors, nlevels, logScaleFactor);
    if (fuse) hipLaunchKernelGGL(k_sim3_project<true>, dim3(n_problems), dim3(kThreads), h->lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_sim3_project<false>, dim3(n_problems), dim3(kThreads), h->lds, (hipStream_t)stream, a);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

// Both host-pointer entry points: the records checked, one block up, launch(), the outputs down
int run_host(const char* fn, bool fuse, oslam_sim3_proj* h, int n_problems, const oslam_sim3_proj_problem_t* problems, const oslam_sim3_proj_kf_rows_t* kf,
             const oslam_sim3_proj_pt_rows_t* pts, int n_pt_out, const uint8_t* skip, int n_kp_out, const oslam_camera_t* cam, const float* bounds, const float* scaleFactors,
             int nlevels, float logScaleFactor, int32_t* out0, int32_t* out1, int32_t* count, int32_t* passes) {
    OSLAM_CHECK(check_call(fn, h, n_problems, kf, pts, n_pt_out, n_kp_out, cam, bounds, scaleFactors, nlevels, logScaleFactor));
    if (n_problems == 0) return OSLAM_OK;
    const int n_out0 = fuse ? n_pt_out : n_kp_out;
    if (!problems || !count || (n_out0 > 0 && !out0) || (fuse && n_pt_out > 0 && !out1)) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_CHECK(check_proj_records(fn, problems, n_problems, ProjExtent{h->max_kps, kf->n_rows, pts->n_rows, n_kp_out, n_pt_out, !fuse}, "keyframe",
                                   [](int, const oslam_sim3_proj_problem_t&) { return OSLAM_OK; }));
    std::lock_guard<std::mutex> lock(h->mu);
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t np = (size_t)n_problems, K = (size_t)kf->n_rows, M = (size_t)pts->n_rows, NO = (size_t)n_pt_out, N0 = (size_t)n_out0;
    oslam::StageLayout lay;   // one block, inputs then outputs: one upload, one download
    const auto fProb = lay.add<oslam_sim3_proj_problem_t>(np);
    const auto fKeys = lay.add<oslam_keypoint_t>(K);
    const auto fDesc = lay.add<uint8_t>(K * 32), fState = lay.add<uint8_t>(K);
    const auto fXw = lay.add<float>(M * 3), fNormal = lay.add<float>(M * 3);
    const auto fPd = lay.add<uint8_t>(M * 32);
    const auto fMax = lay.add<float>(M), fMin = lay.add<float>(M);
    const auto fSkip = lay.add<uint8_t>(NO, skip != nullptr);
    const auto fOut0 = lay.add<int32_t>(N0), fOut1 = lay.add<int32_t>(NO, fuse), fCount = lay.add<int32_t>(np), fPass = lay.add<int32_t>(np, passes != nullptr);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fProb, ph, problems); put(fKeys, ph, kf->keysUn); put(fDesc, ph, kf->desc); put(fState, ph, kf->state); put(fXw, ph, pts->Xw); put(fNormal, ph, pts->normal);
    put(fPd, ph, pts->desc); put(fMax, ph, pts->maxDistance); put(fMin, ph, pts->minDistance); put(fSkip, ph, skip);
    // the caller's output rows travel too: rows no problem owns, and those of a problem the kernel leaves alone, come back as they were
    put(fOut0, ph, (const int32_t*)out0); put(fOut1, ph, (const int32_t*)out1); put(fCount, ph, (const int32_t*)count); put(fPass, ph, (const int32_t*)passes);
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, nullptr));
    const oslam_sim3_proj_kf_rows_t dk = {kf->n_rows, at(fKeys, pd), at(fDesc, pd), at(fState, pd)};
    const oslam_sim3_proj_pt_rows_t dp = {pts->n_rows, at(fXw, pd), at(fNormal, pd), at(fPd, pd), at(fMax, pd), at(fMin, pd)};
    OSLAM_CHECK(launch(fn, fuse, h, n_problems, at(fProb, pd), &dk, &dp, n_pt_out, at(fSkip, pd), n_kp_out, cam, bounds, scaleFactors, nlevels, logScaleFactor, at(fOut0, pd),
                       at(fOut1, pd), at(fCount, pd), at(fPass, pd), nullptr));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fOut0.off, pd + fOut0.off, lay.total() - fOut0.off, hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(fOut0, ph, out0); get(fOut1, ph, out1); get(fCount, ph, count); get(fPass, ph, passes);
    return OSLAM_OK;
}

}  // namespace

extern "C" {

void oslam_sim3_proj_destroy(oslam_sim3_proj_t* h) {
    if (!h) return;
    delete h;
}

int oslam_sim3_proj_create(oslam_sim3_proj_t** out, int max_problems, int max_keypoints, int max_points_total, int device) {
    return create_proj("oslam_sim3_proj_create", "the keyframe's", out, max_problems, max_keypoints, max_points_total, device,
                       {(const void*)k_sim3_project<false>, (const void*)k_sim3_project<true>});
}

int oslam_match_search_by_projection_sim3_batch_device(oslam_sim3_proj_t* h, int n_problems, const oslam_sim3_proj_problem_t* d_problems, const oslam_sim3_proj_kf_rows_t* kf,
                                                       const oslam_sim3_proj_pt_rows_t* pts, int n_pt_out, const uint8_t* d_skip, int n_kp_out, const oslam_camera_t* cam,
                                                       const float bounds[4], const float* scaleFactors, int nlevels, float logScaleFactor, int32_t* d_matched,
                                                       int32_t* d_n_matches, int32_t* d_n_passes, void* stream) {
    return launch("oslam_match_search_by_projection_sim3_batch_device", false, h, n_problems, d_problems, kf, pts, n_pt_out, d_skip, n_kp_out, cam, bounds, scaleFactors, nlevels,
                  logScaleFactor, d_matched, nullptr, d_n_matches, d_n_passes, stream);
}

int oslam_match_fuse_sim3_batch_device(oslam_sim3_proj_t* h, int n_problems, const oslam_sim3_proj_problem_t* d_problems, const oslam_sim3_proj_kf_rows_t* kf,
                                       const oslam_sim3_proj_pt_rows_t* pts, int n_pt_out, const uint8_t* d_skip, const oslam_camera_t* cam, const float bounds[4],
                                       const float* scaleFactors, int nlevels, float logScaleFactor, int32_t* d_fused_kp, int32_t* d_replace, int32_t* d_n_fused,
                                       void* stream) {
    return launch("oslam_match_fuse_sim3_batch_device", true, h, n_problems, d_problems, kf, pts, n_pt_out, d_skip, 0, cam, bounds, scaleFactors, nlevels, logScaleFactor, d_fused_kp,
                  d_replace, d_n_fused, nullptr, stream);
}

int oslam_match_search_by_projection_sim3_batch(oslam_sim3_proj_t* h, int n_problems, const oslam_sim3_proj_problem_t* problems, const oslam_sim3_proj_kf_rows_t* kf,
                                                const oslam_sim3_proj_pt_rows_t* pts, int n_pt_out, const uint8_t* skip, int n_kp_out, const oslam_camera_t* cam,
                                                const float bounds[4], const float* scaleFactors, int nlevels, float logScaleFactor, int32_t* matched, int32_t* n_matches,
                                                int32_t* n_passes) {
    return run_host("oslam_match_search_by_projection_sim3_batch", false, h, n_problems, problems, kf, pts, n_pt_out, skip, n_kp_out, cam, bounds, scaleFactors, nlevels,
                    logScaleFactor, matched, nullptr, n_matches, n_passes);
}

int oslam_match_fuse_sim3_batch(oslam_sim3_proj_t* h, int n_problems, const oslam_sim3_proj_problem_t* problems, const oslam_sim3_proj_kf_rows_t* kf,
                                const oslam_sim3_proj_pt_rows_t* pts, int n_pt_out, const uint8_t* skip, const oslam_camera_t* cam, const float bounds[4],
                                const float* scaleFactors, int nlevels, float logScaleFactor, int32_t* fused_kp, int32_t* replace, int32_t* n_fused) {
    return run_host("oslam_match_fuse_sim3_batch", true, h, n_problems, problems, kf, pts, n_pt_out, skip, 0, cam, bounds, scaleFactors, nlevels, logScaleFactor, fused_kp, replace,
                    n_fused, nullptr);
}

}  // extern "C"
