// reloc_project.hip — ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist) (reference
// src/ORBmatcher.cc:1472-1599), the projection search of Tracking::Relocalization (src/Tracking.cc:1717, :1731), for batches of independent problems on gfx950
// (include/oslam_hip.h, "Relocalisation projection").  One launch, one workgroup per problem: the workgroup stages the FRAME in LDS (keyframe_stage.h: the
// same grid and visiting order as a keyframe's) and its threads stride over the keyframe's map-point slots, which stay in global memory.  The sequential
// claims of :1541 / :1557 are reproduced with the fixpoint sim3_project.hip uses; the rotation histogram (:1577-1596) runs once on the final claims, so a
// match it removes has still blocked the slots after it.
// No inter-workgroup synchronisation and no atomics on global memory: the result does not depend on the order the hardware runs anything in (the LDS
// atomics are minima and counts).  The roundings are those the header lists.  Product code; never includes oracle/.
#include <climits>
#include <cmath>
#include <mutex>

#include "common.h"
#include "keyframe_stage.h"
#include "stage_layout.h"

using oslam::set_error;
using namespace oslam::kf_stage;   // the staged frame, its grid constants and gemm_row

namespace {
constexpr int kHistoLen = 30;   // HISTO_LENGTH, src/ORBmatcher.cc:38
constexpr int kCacheCap = 7;    // candidates kept per slot for the later passes; a slot with more walks its cells again
constexpr int kCacheWords = 8;  // count | kCacheCap entries (dist << 16 | keypoint)
constexpr uint32_t kOverflow = 0xFFFFFFFFu;
constexpr int kFree = INT_MAX;  // no slot claims the keypoint
}  // namespace

struct oslam_reloc_proj {
    int device = 0, max_problems = 0, max_kps = 0, max_pts = 0;
    size_t lds = 0;
    oslam::DeviceBuffer cache;   // [max_pts][kCacheWords] uint32: the candidates of every problem-slot, written in pass 0
    oslam::StagePair io;         // staging of the host-pointer entry point: inputs | outputs
    std::mutex mu;
};

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
    float fx, fy, cx, cy;
    float minX, minY, maxX, maxY, invW, invH;
    float scale[OSLAM_MAX_LEVELS];
    int nlevels; float logScale;
    int check_ori;
};

size_t lds_bytes(int ncap) {
    // desc 32 + xy 8 + claims of this pass 4 + claims of the pass before 4 + items 2 + octave 1 per keypoint, the cell table
    return (size_t)ncap * 51 + (kGridCells + 1) * 4 + 16;
}

struct Pose { float Rcw[9], tcw[3], Ow[3], th; int orbdist; };

// One slot through the gates of :1496-1526 and the window (:1528-1553).  Returns bestIdx2 of an accepted slot (bestDist <= ORBdist), else -1.
// A keypoint k with claim[k] < i is no candidate (claim[k] = -1: a point on entry); with `cache`, the candidates that can ever be accepted (distance <=
// ORBdist, no point on entry) are written there in visiting order.
__device__ int evaluate(const RelocArgs& a, const Staged& s, const float* s_scale, const Pose& T, size_t o, int i, const int* claim, uint32_t* cache) {
    if (cache) cache[0] = 0;
    const float X[3] = {a.pts.Xw[3 * o], a.pts.Xw[3 * o + 1], a.pts.Xw[3 * o + 2]};
    const float xc = gemm_row(T.Rcw, X, T.tcw[0]), yc = gemm_row(T.Rcw + 3, X, T.tcw[1]), zc = gemm_row(T.Rcw + 6, X, T.tcw[2]);
    const float invzc = (float)(1.0 / (double)zc);   // (no test of the sign of z, :1502)
    const float u = a.fx * xc * invzc + a.cx, v = a.fy * yc * invzc + a.cy;
    if (u < a.minX || u > a.maxX) return -1;   // inclusive on both sides (:1507-1510)
    if (v < a.minY || v > a.maxY) return -1;
    if (!(isfinite(u) && isfinite(v))) return -1;   // a NaN passes the comparisons above and finds nothing in GetFeaturesInArea
    const float mfMax = a.pts.maxDistance[o];
    const float maxDistance = 1.2f * mfMax, minDistance = 0.8f * a.pts.minDistance[o];
    const float PO[3] = {X[0] - T.Ow[0], X[1] - T.Ow[1], X[2] - T.Ow[2]};
    const float dist = (float)sqrt(((double)PO[0] * (double)PO[0] + (double)PO[1] * (double)PO[1]) + (double)PO[2] * (double)PO[2]);   // cv::norm
    if (dist < minDistance || dist > maxDistance) return -1;
    // MapPoint::PredictScale (src/MapPoint.cc:505-520) with the log convention of mappoint.hip
    const float ratio = __fdiv_rn(mfMax, dist);
    const float cl = ceilf(__fdiv_rn((float)log((double)ratio), a.logScale));
    const int level = (cl >= 0.0f && cl < 2147483648.0f) ? min((int)cl, a.nlevels - 1) : 0;   // (what does not fit an int converts to INT_MIN on x86: level 0)
    const float r = T.th * s_scale[level];
    // Frame::GetFeaturesInArea (src/Frame.cc:567-620) with minLevel = level - 1, maxLevel = level + 1
    const int nMinCellX = max(0, (int)floorf((u - a.minX - r) * a.invW));
    const int nMaxCellX = min(kGridCols - 1, (int)ceilf((u - a.minX + r) * a.invW));
    const int nMinCellY = max(0, (int)floorf((v - a.minY - r) * a.invH));
    const int nMaxCellY = min(kGridRows - 1, (int)ceilf((v - a.minY + r) * a.invH));
    if (nMinCellX >= kGridCols || nMaxCellX < 0 || nMinCellY >= kGridRows || nMaxCellY < 0) return -1;
    const uint4 q0 = ((const uint4*)(a.pts.desc + o * 32))[0], q1 = ((const uint4*)(a.pts.desc + o * 32))[1];
    int bestDist = 256, bestIdx = -1;
    uint32_t nc = 0;
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
        const int c0 = ix * kGridRows + nMinCellY;
        const int st = c0 > 0 ? s.cell[c0 - 1] : 0, en = s.cell[ix * kGridRows + nMaxCellY];
        for (int q = st; q < en; q++) {   // cells iy = min .. max of a column are contiguous
            const int k = s.items[q];
            const int oct = s.oct[k];
            if (oct < level - 1 || oct > level + 1) continue;
            const float2 p = s.xy[k];
            if (!(fabsf(p.x - u) < r && fabsf(p.y - v) < r)) continue;
            const int owner = claim[k];
            if (owner < 0) continue;   // mvpMapPoints[i2] on entry (:1541)
            const uint4 d0 = ((const uint4*)(s.desc + k * 8))[0], d1 = ((const uint4*)(s.desc + k * 8))[1];
            const int d = __popc(q0.x ^ d0.x) + __popc(q0.y ^ d0.y) + __popc(q0.z ^ d0.z) + __popc(q0.w ^ d0.w) + __popc(q1.x ^ d1.x) + __popc(q1.y ^ d1.y) +
                          __popc(q1.z ^ d1.z) + __popc(q1.w ^ d1.w);
            if (cache && d <= T.orbdist) {
                if (nc < (uint32_t)kCacheCap) cache[1 + nc] = ((uint32_t)d << 16) | (uint32_t)k;
                nc++;
            }
            if (owner < i) continue;   // claimed by a slot before this one (:1541 after :1557)
            if (d < bestDist) { bestDist = d; bestIdx = k; }
        }
    }
    if (cache) cache[0] = nc <= (uint32_t)kCacheCap ? nc : kOverflow;
    return bestDist <= T.orbdist ? bestIdx : -1;
}

// bin of :1562-1567; -1 for what the reference's assert excludes
__device__ __forceinline__ int rot_bin(float kf_angle, float fr_angle) {
    float rot = kf_angle - fr_angle;
    if (rot < 0.0f) rot += 360.0f;
    const float b = roundf(rot * (1.0f / kHistoLen));
    if (!(b >= 0.0f && b <= (float)kHistoLen)) return -1;
    const int bin = (int)b;
    return bin == kHistoLen ? 0 : bin;
}

__global__ __launch_bounds__(kThreads) void k_reloc_project(RelocArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const oslam_reloc_proj_problem_t& P = a.problems[b];
    const int n_kp = P.n_kp, kp_off = P.kp_off, n_pts = P.n_pts, pt_off = P.pt_off, kp_out = P.kp_out_off, pt_out = P.pt_out_off;
    // a record that does not fit the handle or the arrays: -2, nothing else is written (the host-pointer entry point refuses the call instead)
    const bool fits = n_kp >= 0 && n_pts >= 0 && n_kp <= a.ncap && kp_off >= 0 && pt_off >= 0 && pt_out >= 0 && kp_out >= 0 && kp_off <= a.fr.n_rows - n_kp &&
                      pt_off <= a.pts.n_rows - n_pts && pt_out <= a.n_pt_out - n_pts && kp_out <= a.n_kp_out - n_kp && P.ORBdist >= 0 && P.ORBdist <= 255;
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
    Staged s;
    s.desc = (uint32_t*)smem;
    s.xy = (float2*)(s.desc + (size_t)a.ncap * 8);
    int* c_prev = (int*)(s.xy + a.ncap);   // [ncap] the lowest slot that claimed the keypoint in the pass before
    int* c_cur = c_prev + a.ncap;          // [ncap] the same of the running pass
    s.cell = c_cur + a.ncap;
    s.items = (uint16_t*)(s.cell + kGridCells + 1);
    s.oct = (int8_t*)(s.items + a.ncap);
    __shared__ int s_wtot[kThreads / 64];
    __shared__ float s_scale[OSLAM_MAX_LEVELS];
    __shared__ int s_hist[kHistoLen], s_ind[3];
    __shared__ int s_count, s_removed, s_changed;

    const uint8_t* has_mp = a.fr.has_mp + kp_off;
    const uint8_t* skip = a.skip ? a.skip + pt_out : nullptr;
    if (tid < OSLAM_MAX_LEVELS) s_scale[tid] = a.scale[tid];
    if (tid < kHistoLen) s_hist[tid] = 0;
    if (tid == 0) { s_count = 0; s_removed = 0; }
    for (int k = tid; k < n_kp; k += kThreads) c_prev[k] = has_mp[k] ? -1 : kFree;
    // (stage_target begins and ends with a barrier)
    stage_target(s, a.fr.keysUn + kp_off, a.fr.desc + (size_t)kp_off * 32, n_kp, Grid{a.minX, a.minY, a.invW, a.invH}, s_wtot);

    // ---- the search: fixpoint over the sequential claim order (:1541, :1557) ----
    uint32_t* cache = a.cache + (size_t)pt_out * kCacheWords;
    int it = 0;
    for (;; it++) {
        for (int k = tid; k < n_kp; k += kThreads) c_cur[k] = has_mp[k] ? -1 : kFree;
        if (tid == 0) s_changed = 0;
        __syncthreads();
        for (int i = tid; i < n_pts; i += kThreads) {
            uint32_t* cl = cache + (size_t)i * kCacheWords;
            int k = -1;
            if (it == 0) {
                if (skip && skip[i]) cl[0] = 0;
                else k = evaluate(a, s, s_scale, T, (size_t)pt_off + i, i, c_prev, cl);
            } else {
                const uint4 c0 = ((const uint4*)cl)[0];
                if (c0.x == kOverflow) {
                    k = evaluate(a, s, s_scale, T, (size_t)pt_off + i, i, c_prev, nullptr);
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
        if (!changed || it > n_pts) break;   // (slot i is final after pass i + 1: the bound is never reached)
        { int* t = c_cur; c_cur = c_prev; c_prev = t; }
    }

    // ---- mvpMapPoints after the loop: every accepted slot claimed a keypoint of its own; rotation consistency (:1577-1596) ----
    const oslam_keypoint_t* keys = a.fr.keysUn + kp_off;
    const float* kf_angle = a.pts.kf_angle + pt_off;
    if (a.check_ori) {
        for (int k = tid; k < n_kp; k += kThreads) {
            const int o = c_cur[k];
            if (o >= 0 && o != kFree) {
                const int bin = rot_bin(kf_angle[o], keys[k].angle);
                if (bin >= 0) atomicAdd(&s_hist[bin], 1);
            }
        }
        __syncthreads();
        if (tid == 0) {   // ComputeThreeMaxima (:1601-1642)
            int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
            for (int i = 0; i < kHistoLen; i++) {
                const int sz = s_hist[i];
                if (sz > max1) { max3 = max2; max2 = max1; max1 = sz; ind3 = ind2; ind2 = ind1; ind1 = i; }
                else if (sz > max2) { max3 = max2; max2 = sz; ind3 = ind2; ind2 = i; }
                else if (sz > max3) { max3 = sz; ind3 = i; }
            }
            if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
            else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
            s_ind[0] = ind1; s_ind[1] = ind2; s_ind[2] = ind3;
        }
        __syncthreads();
    }
    int32_t* matched = a.matched + kp_out;
    int found = 0, removed = 0;
    for (int k = tid; k < n_kp; k += kThreads) {
        const int o = c_cur[k];
        bool ok = o >= 0 && o != kFree;
        if (ok && a.check_ori) {
            const int bin = rot_bin(kf_angle[o], keys[k].angle);
            if (bin < 0 || (bin != s_ind[0] && bin != s_ind[1] && bin != s_ind[2])) { ok = false; removed++; }
        }
        matched[k] = ok ? o : -1;
        found += ok ? 1 : 0;
    }
    if (found) atomicAdd(&s_count, found);
    if (removed) atomicAdd(&s_removed, removed);
    __syncthreads();
    if (tid == 0) {
        a.count[b] = s_count;
        if (a.removed) a.removed[b] = s_removed;
        if (a.passes) a.passes[b] = it + 1;
    }
}

int check_call(const char* fn, const oslam_reloc_proj* h, int n_problems, const oslam_reloc_proj_frame_rows_t* fr, const oslam_reloc_proj_pt_rows_t* pts, int n_pt_out, int n_kp_out,
               const oslam_camera_t* cam, const float* bounds, const float* scaleFactors, int nlevels, float logScaleFactor) {
    if (!h || !fr || !pts || !cam || !bounds || !scaleFactors) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    if (n_problems < 0 || fr->n_rows < 0 || pts->n_rows < 0 || n_pt_out < 0 || n_kp_out < 0) {
        set_error("%s: %d problems, %d frame rows, %d point rows, %d / %d output rows: none may be negative", fn, n_problems, fr->n_rows, pts->n_rows, n_pt_out, n_kp_out);
        return OSLAM_E_CAPACITY;
    }
    if (n_problems > h->max_problems) { set_error("%s: %d problems exceed the handle's %d", fn, n_problems, h->max_problems); return OSLAM_E_CAPACITY; }
    if (pts->n_rows > h->max_pts || n_pt_out > h->max_pts) {
        set_error("%s: %d point rows / %d skip rows exceed the handle's max_points_total %d", fn, pts->n_rows, n_pt_out, h->max_pts);
        return OSLAM_E_CAPACITY;
    }
    if (nlevels < 1 || nlevels > OSLAM_MAX_LEVELS) { set_error("%s: nlevels = %d outside [1, %d]", fn, nlevels, OSLAM_MAX_LEVELS); return OSLAM_E_INVALID; }
    if (!(bounds[2] > bounds[0]) || !(bounds[3] > bounds[1])) { set_error("%s: empty image bounds", fn); return OSLAM_E_INVALID; }
    if (!(logScaleFactor > 0.0f)) { set_error("%s: logScaleFactor must be positive", fn); return OSLAM_E_INVALID; }
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
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy;
    a.minX = bounds[0]; a.minY = bounds[1]; a.maxX = bounds[2]; a.maxY = bounds[3];
    a.invW = (float)kGridCols / (float)(a.maxX - a.minX);   // src/Frame.cc:160-161
    a.invH = (float)kGridRows / (float)(a.maxY - a.minY);
    for (int i = 0; i < OSLAM_MAX_LEVELS; i++) a.scale[i] = i < nlevels ? scaleFactors[i] : 0.f;
    a.nlevels = nlevels; a.logScale = logScaleFactor; a.check_ori = check_orientation ? 1 : 0;
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
    if (!out) { set_error("oslam_reloc_proj_create: out is NULL"); return OSLAM_E_INVALID; }
    *out = nullptr;
    if (max_problems < 1 || max_keypoints < 1 || max_points_total < 1) { set_error("oslam_reloc_proj_create: bad argument"); return OSLAM_E_INVALID; }
    if (max_keypoints > kMaxKps) {
        set_error("oslam_reloc_proj_create: max_keypoints %d > %d (the frame's keypoints, descriptors and grid, and two claim vectors, must fit 160 KiB of LDS)", max_keypoints, kMaxKps);
        return OSLAM_E_INVALID;
    }
    const int ndev = oslam_device_count();
    if (ndev <= 0) return oslam::no_device("oslam_reloc_proj_create");
    if (device < 0 || device >= ndev) { set_error("oslam_reloc_proj_create: device out of range"); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(device));
    oslam_reloc_proj* h = new oslam_reloc_proj;
    h->device = device; h->max_problems = max_problems; h->max_kps = max_keypoints; h->max_pts = max_points_total; h->lds = lds_bytes(max_keypoints);
    int rc = h->cache.alloc((size_t)max_points_total * kCacheWords * sizeof(uint32_t));
    if (rc == OSLAM_OK) {   // (the attribute belongs to the kernel, not to the handle)
        const hipError_t e = hipFuncSetAttribute((const void*)k_reloc_project, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(kMaxKps));
        if (e != hipSuccess) { set_error("oslam_reloc_proj_create: hipFuncSetAttribute failed: %s", hipGetErrorString(e)); rc = OSLAM_E_HIP; }
    }
    if (rc != OSLAM_OK) { delete h; return rc; }
    *out = h;
    return OSLAM_OK;
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
    for (int b = 0; b < n_problems; b++) {
        const oslam_reloc_proj_problem_t& P = problems[b];
        if (P.n_kp < 0 || P.n_pts < 0 || P.n_kp > h->max_kps) {
            set_error("%s: problem %d has %d keypoints (at most %d) and %d points: none may be negative", fn, b, P.n_kp, h->max_kps, P.n_pts);
            return OSLAM_E_CAPACITY;
        }
        const bool inside = P.kp_off >= 0 && P.pt_off >= 0 && P.pt_out_off >= 0 && P.kp_out_off >= 0 && P.kp_off <= fr->n_rows - P.n_kp && P.pt_off <= pts->n_rows - P.n_pts &&
                            P.pt_out_off <= n_pt_out - P.n_pts && P.kp_out_off <= n_kp_out - P.n_kp;
        if (!inside) {
            set_error("%s: problem %d (kp_off %d, pt_off %d, kp_out_off %d, pt_out_off %d) lies outside the %d frame rows / %d point rows / %d and %d output rows", fn, b, P.kp_off,
                      P.pt_off, P.kp_out_off, P.pt_out_off, fr->n_rows, pts->n_rows, n_kp_out, n_pt_out);
            return OSLAM_E_INVALID;
        }
        if (P.ORBdist < 0 || P.ORBdist > 255) {
            set_error("%s: problem %d has ORBdist %d outside 0 .. 255 (with every candidate claimed the reference would write mvpMapPoints[-1])", fn, b, P.ORBdist);
            return OSLAM_E_INVALID;
        }
    }
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
