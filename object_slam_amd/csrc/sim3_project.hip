// sim3_project.hip — ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (reference src/ORBmatcher.cc:290-403) and ORBmatcher::Fuse(pKF, Scw,
// vpPoints, th, vpReplacePoint) (:977-1100) for batches of independent problems on gfx950 (include/oslam_hip.h, "Sim3 projection").  One launch, one
// workgroup per problem: the workgroup stages the keyframe in LDS (keyframe_stage.h, shared with sim3_match.hip) and its threads stride over the
// problem's candidate points, which stay in global memory.  The search reproduces the sequential claims of :375 / :396 with the fixpoint k_search_window of
// matcher.hip uses; Fuse has no claims, takes one pass and reports the surgery of :1084-1094 instead of performing it.
// No inter-workgroup synchronisation and no atomics on global memory: the result does not depend on the order the hardware runs anything in.
// The roundings are those the header lists.  Product code; never includes oracle/.
#include <climits>
#include <cmath>
#include <mutex>

#include "common.h"
#include "keyframe_stage.h"
#include "stage_layout.h"

using oslam::set_error;
using namespace oslam::kf_stage;   // the staged keyframe, its grid constants and gemm_row

namespace {
constexpr int kThLow = 50;      // ORBmatcher::TH_LOW, src/ORBmatcher.cc:37
constexpr int kCacheCap = 7;    // candidates kept per point for the later passes of the search; a point with more walks its cells again
constexpr int kCacheWords = 8;  // count | kCacheCap entries (dist << 16 | keypoint)
constexpr uint32_t kOverflow = 0xFFFFFFFFu;
constexpr int kFree = INT_MAX;  // no point claims the keypoint
}  // namespace

struct oslam_sim3_proj {
    int device = 0, max_problems = 0, max_kps = 0, max_pts = 0;
    size_t lds = 0;
    oslam::DeviceBuffer cache;   // [max_pts][kCacheWords] uint32: the search's candidates of every problem-point, written in pass 0
    oslam::StagePair io;         // staging of the host-pointer entry points: inputs | outputs
    std::mutex mu;
};

namespace {

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
    float fx, fy, cx, cy;
    float minX, minY, maxX, maxY, invW, invH;
    float scale[OSLAM_MAX_LEVELS];
    int nlevels; float logScale;
};

size_t lds_bytes(int ncap) {
    // desc 32 + xy 8 + claims of this pass 4 + claims of the pass before 4 + items 2 + octave 1 per keypoint, the cell table
    return (size_t)ncap * 51 + (kGridCells + 1) * 4 + 16;
}

struct Pose { float Rcw[9], tcw[3], Ow[3], th; };

// One point through the gates of :312-365 / :1000-1054 and the window (:367-392 / :1056-1079).  Returns bestIdx of an accepted point (bestDist <= TH_LOW), else -1.
// Search: a keypoint k with claim[k] < i is no candidate (claim[k] = -1: matched on entry); with `cache`, the candidates that can ever be accepted (distance
// <= TH_LOW, not matched on entry) are written there in visiting order.
template <bool kFuse>
__device__ int evaluate(const ProjArgs& a, const Staged& s, const float* s_scale, const Pose& T, size_t o, int i, const int* claim, uint32_t* cache) {
    if (cache) cache[0] = 0;
    const float X[3] = {a.pts.Xw[3 * o], a.pts.Xw[3 * o + 1], a.pts.Xw[3 * o + 2]};
    const float Pc[3] = {gemm_row(T.Rcw, X, T.tcw[0]), gemm_row(T.Rcw + 3, X, T.tcw[1]), gemm_row(T.Rcw + 6, X, T.tcw[2])};
    if (Pc[2] < 0.0f) return -1;
    const float invz = (float)(1.0 / (double)Pc[2]);
    const float x = Pc[0] * invz, y = Pc[1] * invz;
    const float u = a.fx * x + a.cx, v = a.fy * y + a.cy;
    if (!(u >= a.minX && u < a.maxX && v >= a.minY && v < a.maxY)) return -1;   // KeyFrame::IsInImage (src/KeyFrame.cc:610)
    const float mfMax = a.pts.maxDistance[o];
    const float maxDistance = 1.2f * mfMax, minDistance = 0.8f * a.pts.minDistance[o];
    const float PO[3] = {X[0] - T.Ow[0], X[1] - T.Ow[1], X[2] - T.Ow[2]};
    const float dist = (float)sqrt(((double)PO[0] * (double)PO[0] + (double)PO[1] * (double)PO[1]) + (double)PO[2] * (double)PO[2]);   // cv::norm
    if (dist < minDistance || dist > maxDistance) return -1;
    const float Pn[3] = {a.pts.normal[3 * o], a.pts.normal[3 * o + 1], a.pts.normal[3 * o + 2]};
    const double dot = ((double)PO[0] * (double)Pn[0] + (double)PO[1] * (double)Pn[1]) + (double)PO[2] * (double)Pn[2];
    if (dot < 0.5 * (double)dist) return -1;
    // MapPoint::PredictScale (src/MapPoint.cc:488-503) with the log convention of mappoint.hip
    const float ratio = __fdiv_rn(mfMax, dist);
    const float cl = ceilf(__fdiv_rn((float)log((double)ratio), a.logScale));
    const int level = (cl >= 0.0f && cl < 2147483648.0f) ? min((int)cl, a.nlevels - 1) : 0;   // (what does not fit an int converts to INT_MIN on x86: level 0)
    const float r = T.th * s_scale[level];
    // KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:569-608)
    const int nMinCellX = max(0, (int)floorf((u - a.minX - r) * a.invW));
    const int nMaxCellX = min(kGridCols - 1, (int)ceilf((u - a.minX + r) * a.invW));
    const int nMinCellY = max(0, (int)floorf((v - a.minY - r) * a.invH));
    const int nMaxCellY = min(kGridRows - 1, (int)ceilf((v - a.minY + r) * a.invH));
    if (nMinCellX >= kGridCols || nMaxCellX < 0 || nMinCellY >= kGridRows || nMaxCellY < 0) return -1;
    const uint4 q0 = ((const uint4*)(a.pts.desc + o * 32))[0], q1 = ((const uint4*)(a.pts.desc + o * 32))[1];
    int bestDist = kFuse ? INT_MAX : 256, bestIdx = -1;
    uint32_t nc = 0;
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
        const int c0 = ix * kGridRows + nMinCellY;
        const int st = c0 > 0 ? s.cell[c0 - 1] : 0, en = s.cell[ix * kGridRows + nMaxCellY];
        for (int q = st; q < en; q++) {   // cells iy = min .. max of a column are contiguous
            const int k = s.items[q];
            const float2 p = s.xy[k];
            if (!(fabsf(p.x - u) < r && fabsf(p.y - v) < r)) continue;
            int owner = kFree;
            if (!kFuse) {
                owner = claim[k];
                if (owner < 0) continue;   // vpMatched[idx] on entry (:375)
            }
            const int oct = s.oct[k];
            if (oct < level - 1 || oct > level) continue;
            const uint4 d0 = ((const uint4*)(s.desc + k * 8))[0], d1 = ((const uint4*)(s.desc + k * 8))[1];
            const int d = __popc(q0.x ^ d0.x) + __popc(q0.y ^ d0.y) + __popc(q0.z ^ d0.z) + __popc(q0.w ^ d0.w) + __popc(q1.x ^ d1.x) + __popc(q1.y ^ d1.y) +
                          __popc(q1.z ^ d1.z) + __popc(q1.w ^ d1.w);
            if (!kFuse) {
                if (cache && d <= kThLow) {
                    if (nc < (uint32_t)kCacheCap) cache[1 + nc] = ((uint32_t)d << 16) | (uint32_t)k;
                    nc++;
                }
                if (owner < i) continue;   // claimed by a point before this one (:375 after :396)
            }
            if (d < bestDist) { bestDist = d; bestIdx = k; }
        }
    }
    if (cache) cache[0] = nc <= (uint32_t)kCacheCap ? nc : kOverflow;
    return bestDist <= kThLow ? bestIdx : -1;
}

template <bool kFuse>
__global__ __launch_bounds__(kThreads) void k_sim3_project(ProjArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const oslam_sim3_proj_problem_t& P = a.problems[b];
    const int n_kp = P.n_kp, kp_off = P.kp_off, n_pts = P.n_pts, pt_off = P.pt_off, kp_out = P.kp_out_off, pt_out = P.pt_out_off;
    // a record that does not fit the handle or the arrays: -2, nothing else is written (the host-pointer entry points refuse the call instead)
    bool fits = n_kp >= 0 && n_pts >= 0 && n_kp <= a.ncap && kp_off >= 0 && pt_off >= 0 && pt_out >= 0 && kp_off <= a.kf.n_rows - n_kp && pt_off <= a.pts.n_rows - n_pts &&
                pt_out <= a.n_pt_out - n_pts;
    if (!kFuse) fits = fits && kp_out >= 0 && kp_out <= a.n_kp_out - n_kp;
    if (!fits) {
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
    Staged s;
    s.desc = (uint32_t*)smem;
    s.xy = (float2*)(s.desc + (size_t)a.ncap * 8);
    int* c_prev = (int*)(s.xy + a.ncap);   // [ncap] search: the lowest point that claimed the keypoint in the pass before; Fuse: the first point added there
    int* c_cur = c_prev + a.ncap;          // [ncap] search: the same of the running pass
    s.cell = c_cur + a.ncap;
    s.items = (uint16_t*)(s.cell + kGridCells + 1);
    s.oct = (int8_t*)(s.items + a.ncap);
    __shared__ int s_wtot[kThreads / 64];
    __shared__ float s_scale[OSLAM_MAX_LEVELS];
    __shared__ int s_count, s_changed;

    const uint8_t* state = a.kf.state + kp_off;
    const uint8_t* skip = a.skip ? a.skip + pt_out : nullptr;
    if (tid < OSLAM_MAX_LEVELS) s_scale[tid] = a.scale[tid];
    if (tid == 0) s_count = 0;
    for (int k = tid; k < n_kp; k += kThreads) c_prev[k] = (!kFuse && state[k]) ? -1 : kFree;
    // (stage_target begins and ends with a barrier)
    stage_target(s, a.kf.keysUn + kp_off, a.kf.desc + (size_t)kp_off * 32, n_kp, Grid{a.minX, a.minY, a.invW, a.invH}, s_wtot);

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
    uint32_t* cache = a.cache + (size_t)pt_out * kCacheWords;
    int it = 0;
    for (;; it++) {
        for (int k = tid; k < n_kp; k += kThreads) c_cur[k] = state[k] ? -1 : kFree;
        if (tid == 0) s_changed = 0;
        __syncthreads();
        for (int i = tid; i < n_pts; i += kThreads) {
            uint32_t* cl = cache + (size_t)i * kCacheWords;
            int k = -1;
            if (it == 0) {
                if (skip && skip[i]) cl[0] = 0;
                else k = evaluate<false>(a, s, s_scale, T, (size_t)pt_off + i, i, c_prev, cl);
            } else {
                const uint4 c0 = ((const uint4*)cl)[0];
                if (c0.x == kOverflow) {
                    k = evaluate<false>(a, s, s_scale, T, (size_t)pt_off + i, i, c_prev, nullptr);
                } else if (c0.x) {
                    // the candidates and their distances do not change, only the claims do: replay the list (visiting order) against the claims
                    const uint4 c1 = ((const uint4*)cl)[1];
                    const uint32_t e[kCacheCap] = {c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
                    int bestDist = 256;
#pragma unroll
                    for (int t = 0; t < kCacheCap; t++) {
                        if ((uint32_t)t < c0.x) {
                            const int kk = e[t] & 0xFFFF, d = e[t] >> 16;
                            if (c_prev[kk] >= i && d < bestDist) { bestDist = d; k = kk; }
                        }
                    }
                }
            }
            if (k >= 0) atomicMin(&c_cur[k], i);
        }
        __syncthreads();
        int diff = 0;
        for (int k = tid; k < n_kp; k += kThreads) diff |= (c_cur[k] != c_prev[k]);
        if (diff) s_changed = 1;
        __syncthreads();
        const int changed = s_changed;
        __syncthreads();
        if (!changed || it > n_pts) break;   // (point i is final after pass i + 1: the bound is never reached)
        { int* t = c_cur; c_cur = c_prev; c_prev = t; }
    }
    // vpMatched after the loop: every accepted point claimed a keypoint of its own
    int32_t* matched = a.out0 + kp_out;
    int found = 0;
    for (int k = tid; k < n_kp; k += kThreads) {
        const int o = c_cur[k];
        const bool ok = o >= 0 && o != kFree;
        matched[k] = ok ? o : -1;
        found += ok ? 1 : 0;
    }
    if (found) atomicAdd(&s_count, found);
    __syncthreads();
    if (tid == 0) {
        a.count[b] = s_count;
        if (a.passes) a.passes[b] = it + 1;
    }
}

int check_call(const char* fn, const oslam_sim3_proj* h, int n_problems, const oslam_sim3_proj_kf_rows_t* kf, const oslam_sim3_proj_pt_rows_t* pts, int n_pt_out, int n_kp_out,
               const oslam_camera_t* cam, const float* bounds, const float* scaleFactors, int nlevels, float logScaleFactor) {
    if (!h || !kf || !pts || !cam || !bounds || !scaleFactors) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    if (n_problems < 0 || kf->n_rows < 0 || pts->n_rows < 0 || n_pt_out < 0 || n_kp_out < 0) {
        set_error("%s: %d problems, %d keyframe rows, %d point rows, %d / %d output rows: none may be negative", fn, n_problems, kf->n_rows, pts->n_rows, n_pt_out, n_kp_out);
        return OSLAM_E_CAPACITY;
    }
    if (n_problems > h->max_problems) { set_error("%s: %d problems exceed the handle's %d", fn, n_problems, h->max_problems); return OSLAM_E_CAPACITY; }
    if (pts->n_rows > h->max_pts || n_pt_out > h->max_pts) {
        set_error("%s: %d point rows / %d point output rows exceed the handle's max_points_total %d", fn, pts->n_rows, n_pt_out, h->max_pts);
        return OSLAM_E_CAPACITY;
    }
    if (nlevels < 1 || nlevels > OSLAM_MAX_LEVELS) { set_error("%s: nlevels = %d outside [1, %d]", fn, nlevels, OSLAM_MAX_LEVELS); return OSLAM_E_INVALID; }
    if (!(bounds[2] > bounds[0]) || !(bounds[3] > bounds[1])) { set_error("%s: empty image bounds", fn); return OSLAM_E_INVALID; }
    if (!(logScaleFactor > 0.0f)) { set_error("%s: logScaleFactor must be positive", fn); return OSLAM_E_INVALID; }
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
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy;
    a.minX = bounds[0]; a.minY = bounds[1]; a.maxX = bounds[2]; a.maxY = bounds[3];
    a.invW = (float)kGridCols / (float)(a.maxX - a.minX);   // src/Frame.cc:160-161
    a.invH = (float)kGridRows / (float)(a.maxY - a.minY);
    for (int i = 0; i < OSLAM_MAX_LEVELS; i++) a.scale[i] = i < nlevels ? scaleFactors[i] : 0.f;
    a.nlevels = nlevels; a.logScale = logScaleFactor;
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
    for (int b = 0; b < n_problems; b++) {
        const oslam_sim3_proj_problem_t& P = problems[b];
        if (P.n_kp < 0 || P.n_pts < 0 || P.n_kp > h->max_kps) {
            set_error("%s: problem %d has %d keypoints (at most %d) and %d points: none may be negative", fn, b, P.n_kp, h->max_kps, P.n_pts);
            return OSLAM_E_CAPACITY;
        }
        bool inside = P.kp_off >= 0 && P.pt_off >= 0 && P.pt_out_off >= 0 && P.kp_off <= kf->n_rows - P.n_kp && P.pt_off <= pts->n_rows - P.n_pts && P.pt_out_off <= n_pt_out - P.n_pts;
        if (!fuse) inside = inside && P.kp_out_off >= 0 && P.kp_out_off <= n_kp_out - P.n_kp;
        if (!inside) {
            set_error("%s: problem %d (kp_off %d, pt_off %d, kp_out_off %d, pt_out_off %d) lies outside the %d keyframe rows / %d point rows / %d and %d output rows", fn, b, P.kp_off,
                      P.pt_off, P.kp_out_off, P.pt_out_off, kf->n_rows, pts->n_rows, n_kp_out, n_pt_out);
            return OSLAM_E_INVALID;
        }
    }
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
    if (!out) { set_error("oslam_sim3_proj_create: out is NULL"); return OSLAM_E_INVALID; }
    *out = nullptr;
    if (max_problems < 1 || max_keypoints < 1 || max_points_total < 1) { set_error("oslam_sim3_proj_create: bad argument"); return OSLAM_E_INVALID; }
    if (max_keypoints > kMaxKps) {
        set_error("oslam_sim3_proj_create: max_keypoints %d > %d (the keyframe's keypoints, descriptors and grid, and two claim vectors, must fit 160 KiB of LDS)", max_keypoints, kMaxKps);
        return OSLAM_E_INVALID;
    }
    const int ndev = oslam_device_count();
    if (ndev <= 0) return oslam::no_device("oslam_sim3_proj_create");
    if (device < 0 || device >= ndev) { set_error("oslam_sim3_proj_create: device out of range"); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(device));
    oslam_sim3_proj* h = new oslam_sim3_proj;
    h->device = device; h->max_problems = max_problems; h->max_kps = max_keypoints; h->max_pts = max_points_total; h->lds = lds_bytes(max_keypoints);
    int rc = h->cache.alloc((size_t)max_points_total * kCacheWords * sizeof(uint32_t));
    for (int f = 0; f < 2 && rc == OSLAM_OK; f++) {   // (the attribute belongs to the kernel, not to the handle)
        const hipError_t e = hipFuncSetAttribute(f ? (const void*)k_sim3_project<true> : (const void*)k_sim3_project<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lds_bytes(kMaxKps));
        if (e != hipSuccess) { set_error("oslam_sim3_proj_create: hipFuncSetAttribute failed: %s", hipGetErrorString(e)); rc = OSLAM_E_HIP; }
    }
    if (rc != OSLAM_OK) { delete h; return rc; }
    *out = h;
    return OSLAM_OK;
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
