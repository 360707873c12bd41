// The windowed projection search of the operators that run one workgroup of 1024 threads per problem (sim3_match.hip, sim3_project.hip, reloc_project.hip, search_init.hip):
//  - one keyframe or frame in LDS: keypoint xy, octave, the 32-byte descriptors and the 64 x 48 cell table in GetFeaturesInArea's visiting order (cell
//    column, then cell row, then keypoint index), with the layout of the dynamic LDS block stated once;
//  - the level a point is predicted at, the walk over its window and the Hamming distance;
//  - the replay of the reference's sequential claims (a later point does not get a keypoint an earlier one took) as a fixpoint over two claim vectors, with
//    a per-point candidate cache, and the handle and create function of the two operators that use it;
//  - gemm_row and three_maxima, which matcher.hip takes from here too, and rot_bin.
// What differs between the operators stays with them: the gates before the window (sign of z, bounds, distance, viewing angle), the thresholds and what
// becomes of the matches.  The host arithmetic that needs no HIP is in window_search_host.h.
#pragma once
#include <climits>
#include <initializer_list>
#include <mutex>

#include "common.h"
#include "window_search_host.h"

namespace oslam {
namespace kf_stage {

constexpr int kGridCells = kGridCols * kGridRows;
constexpr int kThreads = 1024;                  // threads of the workgroup
constexpr int kMaxKps = 2400;                   // keypoints of one keyframe (what lds_bytes allows is asserted below)
constexpr int kHistoLen = 30;                   // HISTO_LENGTH, src/ORBmatcher.cc:38

struct Staged {
    uint32_t* desc;    // [ncap][8]
    float2* xy;        // [ncap]
    int* cell;         // [kGridCells + 1] end of every cell in items
    uint16_t* items;   // [ncap] keypoints sorted by cell (ix major, iy minor), index order inside a cell
    int8_t* oct;       // [ncap]
};

// ---- the dynamic LDS block: desc | xy | int[ncap] | int[ncap] | cell | items | oct ----

// The staged keyframe and the two int vectors of the including kernel (vnMatch1 / vnMatch2, or the claims of the pass before and of the running pass)
struct Lds : Staged { int* v0; int* v1; };

constexpr size_t lds_bytes(int ncap) { return (size_t)ncap * 51 + (kGridCells + 1) * 4 + 16; }
static_assert(8 * sizeof(uint32_t) + sizeof(float2) + 2 * sizeof(int) + sizeof(uint16_t) + sizeof(int8_t) == 51, "lds_bytes counts what carve lays out per keypoint");
static_assert(lds_bytes(kMaxKps) + 1024 <= 160 * 1024, "a keyframe of kMaxKps keypoints and 1 KiB of static LDS fit the 160 KiB of a workgroup");

__device__ __forceinline__ Lds carve(uint8_t* smem, int ncap) {   // smem: 16-byte aligned, lds_bytes(ncap) long
    Lds s;
    s.desc = (uint32_t*)smem;
    s.xy = (float2*)(s.desc + (size_t)ncap * 8);
    s.v0 = (int*)(s.xy + ncap);
    s.v1 = s.v0 + ncap;
    s.cell = s.v1 + ncap;
    s.items = (uint16_t*)(s.cell + kGridCells + 1);
    s.oct = (int8_t*)(s.items + ncap);
    return s;
}

// cv::Mat 3x3 * 3x1 + 3x1 = one cv::gemm, flags == 0, len == 3: the three products summed in float from left to right (OpenCV's small-matrix branch), the
// `+ c` in double, rounded once
__device__ __forceinline__ float gemm_row(const float* a, const float* x, float cc) {
    const float t0 = a[0] * x[0] + a[1] * x[1] + a[2] * x[2];
    return (float)((double)t0 + (double)cc);
}

// The keyframe (N keypoints at kps, descriptors at desc8) into LDS: xy, octave, descriptors, and mGrid (src/Frame.cc:455-470: cell = round((x - mnMinX) * inv),
// push_back in index order).  s_wtot: kThreads / 64 ints of LDS.  Begins and ends with a barrier.
__device__ inline void stage_target(const Staged& s, const oslam_keypoint_t* kps, const uint8_t* desc8, int N, const WindowCam& g, int* s_wtot) {
    const int tid = threadIdx.x;
    const uint32_t* gdesc = (const uint32_t*)desc8;
    __syncthreads();   // the readers of the keyframe staged before are done
    for (int i = tid; i <= kGridCells; i += kThreads) s.cell[i] = 0;
    __syncthreads();
    for (int i = tid; i < N; i += kThreads) {
        const oslam_keypoint_t kp = kps[i];
        s.xy[i] = make_float2(kp.x, kp.y);
        s.oct[i] = (int8_t)min(max(kp.octave, -2), 127);   // (the level gate compares with levels 0 .. 15: -2 and 127 stand for everything beyond)
        const int px = (int)roundf((kp.x - g.minX) * g.invW);
        const int py = (int)roundf((kp.y - g.minY) * g.invH);
        if (px >= 0 && px < kGridCols && py >= 0 && py < kGridRows) atomicAdd(&s.cell[px * kGridRows + py], 1);
    }
    for (int i = tid; i < N * 8; i += kThreads) s.desc[i] = gdesc[i];
    __syncthreads();
    {   // exclusive scan of the cell counts, kCellsPer per thread
        constexpr int kCellsPer = kGridCells / kThreads;
        static_assert(kCellsPer * kThreads == kGridCells, "the cell scan gives every thread the same number of cells");
        const int lane = tid & 63, wv = tid >> 6;
        const int base = tid * kCellsPer;
        int cc[kCellsPer];
        int incl = 0;
#pragma unroll
        for (int k = 0; k < kCellsPer; k++) { cc[k] = s.cell[base + k]; incl += cc[k]; }
        const int local = incl;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (lane == 63) s_wtot[wv] = incl;
        __syncthreads();
        int start = incl - local;
        for (int i = 0; i < wv; i++) start += s_wtot[i];
#pragma unroll
        for (int k = 0; k < kCellsPer; k++) { s.cell[base + k] = start; start += cc[k]; }
    }
    __syncthreads();
    // scatter with the cell starts as cursors (afterwards cell[c] = end of cell c = start of c + 1), then restore index order inside every cell
    for (int i = tid; i < N; i += kThreads) {
        const float2 p = s.xy[i];
        const int px = (int)roundf((p.x - g.minX) * g.invW);
        const int py = (int)roundf((p.y - g.minY) * g.invH);
        if (px >= 0 && px < kGridCols && py >= 0 && py < kGridRows) {
            const int pos = atomicAdd(&s.cell[px * kGridRows + py], 1);
            s.items[pos] = (uint16_t)i;
        }
    }
    __syncthreads();
    for (int cell = tid; cell < kGridCells; cell += kThreads) {
        const int st = cell > 0 ? s.cell[cell - 1] : 0, en = s.cell[cell];
        for (int q = st + 1; q < en; q++) {   // insertion sort, cells hold a handful of points
            const uint16_t v = s.items[q];
            int p = q - 1;
            while (p >= st && s.items[p] > v) { s.items[p + 1] = s.items[p]; p--; }
            s.items[p + 1] = v;
        }
    }
    __syncthreads();
}

// ---- one point against the staged keyframe ----

// MapPoint::PredictScale (src/MapPoint.cc:488-503, :505-520) with the log convention of mappoint.hip
__device__ __forceinline__ int predict_level(float mfMax, float dist, const WindowCam& cam) {
    const float ratio = __fdiv_rn(mfMax, dist);
    const float cl = ceilf(__fdiv_rn((float)log((double)ratio), cam.logScale));
    return (cl >= 0.0f && cl < 2147483648.0f) ? min((int)cl, cam.nlevels - 1) : 0;   // (what does not fit an int converts to INT_MIN on x86: level 0)
}

// DescriptorDistance of the descriptor in (q0, q1) and the staged one at d8
__device__ __forceinline__ int hamming256(const uint4& q0, const uint4& q1, const uint32_t* d8) {
    const uint4 d0 = ((const uint4*)d8)[0], d1 = ((const uint4*)d8)[1];
    return __popc(q0.x ^ d0.x) + __popc(q0.y ^ d0.y) + __popc(q0.z ^ d0.z) + __popc(q0.w ^ d0.w) + __popc(q1.x ^ d1.x) + __popc(q1.y ^ d1.y) + __popc(q1.z ^ d1.z) +
           __popc(q1.w ^ d1.w);
}

// GetFeaturesInArea(u, v, r, level + kOctLo, level + kOctHi) (src/KeyFrame.cc:569-608, src/Frame.cc:567-620): visit(k) for every staged keypoint k of the
// window, in the reference's order.  The window and the octave are tested here, so that visit sees only what GetFeaturesInArea returns.
template <int kOctLo, int kOctHi, class Visit>
__device__ __forceinline__ void walk_window(const Staged& s, const WindowCam& cam, float u, float v, float r, int level, Visit visit) {
    const int nMinCellX = max(0, (int)floorf((u - cam.minX - r) * cam.invW));
    const int nMaxCellX = min(kGridCols - 1, (int)ceilf((u - cam.minX + r) * cam.invW));
    const int nMinCellY = max(0, (int)floorf((v - cam.minY - r) * cam.invH));
    const int nMaxCellY = min(kGridRows - 1, (int)ceilf((v - cam.minY + r) * cam.invH));
    if (nMinCellX >= kGridCols || nMaxCellX < 0 || nMinCellY >= kGridRows || nMaxCellY < 0) return;
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
        const int c0 = ix * kGridRows + nMinCellY;
        const int st = c0 > 0 ? s.cell[c0 - 1] : 0, en = s.cell[ix * kGridRows + nMaxCellY];
        for (int q = st; q < en; q++) {   // cells iy = min .. max of a column are contiguous
            const int k = s.items[q];
            const float2 p = s.xy[k];
            if (!(fabsf(p.x - u) < r && fabsf(p.y - v) < r)) continue;
            const int oct = s.oct[k];
            if (oct < level + kOctLo || oct > level + kOctHi) continue;
            visit(k);
        }
    }
}

// The nearest descriptor of the window and its keypoint, the first one visited among equals; (INT_MAX, -1) for an empty window
struct Nearest { int dist, idx; };
template <int kOctLo, int kOctHi>
__device__ __forceinline__ Nearest nearest_in_window(const Staged& s, const WindowCam& cam, float u, float v, float r, int level, const uint8_t* desc32) {
    const uint4 q0 = ((const uint4*)desc32)[0], q1 = ((const uint4*)desc32)[1];
    Nearest best = {INT_MAX, -1};
    walk_window<kOctLo, kOctHi>(s, cam, u, v, r, level, [&](int k) {
        const int d = hamming256(q0, q1, s.desc + k * 8);
        if (d < best.dist) best = {d, k};
    });
    return best;
}

// ---- the sequential claims ----
// The reference walks its points in order, and a point does not take a keypoint that holds a match: one that had it on entry, or one an earlier point of the
// same call took.  claim[k] is -1 for a keypoint occupied on entry, else the lowest point that took k in the pass before (kFree: none).  A pass evaluates every
// point against the claims of the pass before; when two passes agree the claims are the sequential ones (point i is final after pass i + 1).

constexpr int kCacheCap = 7;    // candidates kept per point for the later passes; a point with more walks its cells again
constexpr int kCacheWords = 8;  // count | kCacheCap entries (dist << 16 | keypoint), in global memory
static_assert(kCacheWords == kCacheCap + 1 && kCacheWords * sizeof(uint32_t) == 2 * sizeof(uint4), "replay_cached reads a cache line as two uint4");
constexpr uint32_t kOverflow = 0xFFFFFFFFu;
constexpr int kFree = INT_MAX;  // no point claims the keypoint

__device__ __forceinline__ bool is_claimed(int owner) { return owner >= 0 && owner != kFree; }

// Point i's keypoint under `claim`: the nearest of its window that no earlier point claimed, if it is within th, else -1.  With `cache` (pass 0) the candidates
// that can ever be accepted (within th, not occupied on entry) go there in visiting order.
template <int kOctLo, int kOctHi>
__device__ __forceinline__ int nearest_unclaimed(const Staged& s, const WindowCam& cam, float u, float v, float r, int level, const uint8_t* desc32, int th, int i, const int* claim,
                                                 uint32_t* cache) {
    const uint4 q0 = ((const uint4*)desc32)[0], q1 = ((const uint4*)desc32)[1];
    int bestDist = 256, bestIdx = -1;
    uint32_t nc = 0;
    walk_window<kOctLo, kOctHi>(s, cam, u, v, r, level, [&](int k) {
        const int owner = claim[k];
        if (owner < 0) return;   // occupied on entry
        const int d = hamming256(q0, q1, s.desc + k * 8);
        if (cache && d <= th) {
            if (nc < (uint32_t)kCacheCap) cache[1 + nc] = ((uint32_t)d << 16) | (uint32_t)k;
            nc++;
        }
        if (owner < i) return;   // claimed by a point before this one
        if (d < bestDist) { bestDist = d; bestIdx = k; }
    });
    if (cache) cache[0] = nc <= (uint32_t)kCacheCap ? nc : kOverflow;
    return bestDist <= th ? bestIdx : -1;
}

// The same from the cached list (c0 = its first four words, c0.x = the count, not 0 and not kOverflow): the candidates and their distances do not change
// from pass to pass, only the claims do
__device__ __forceinline__ int replay_cached(const uint32_t* cl, const uint4& c0, int i, const int* claim) {
    const uint4 c1 = ((const uint4*)cl)[1];
    const uint32_t e[kCacheCap] = {c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    int bestDist = 256, k = -1;
#pragma unroll
    for (int t = 0; t < kCacheCap; t++) {
        if ((uint32_t)t < c0.x) {
            const int kk = e[t] & 0xFFFF, d = e[t] >> 16;
            if (claim[kk] >= i && d < bestDist) { bestDist = d; k = kk; }
        }
    }
    return k;
}

template <class Occupied>
__device__ __forceinline__ void reset_claims(int* claim, int n_kp, Occupied occupied) {
    for (int k = threadIdx.x; k < n_kp; k += kThreads) claim[k] = occupied(k) ? -1 : kFree;
}

// The passes.  On entry c_prev holds reset_claims and a barrier has passed since.  occupied(k): keypoint k holds a match on entry.  evaluate(i, claim, cache):
// point i's keypoint under `claim` or -1, by nearest_unclaimed for a point that reaches its window; in pass 0 it gets the point's cache line, afterwards NULL,
// and then it is called only for the points whose count is kOverflow.  Returns the number of passes; c_cur holds the final claims, visible to all threads.
template <class Occupied, class Evaluate>
__device__ __forceinline__ int claim_fixpoint(int n_kp, int n_pts, int*& c_prev, int*& c_cur, uint32_t* cache, int* s_changed, Occupied occupied, Evaluate evaluate) {
    const int tid = threadIdx.x;
    int it = 0;
    for (;; it++) {
        reset_claims(c_cur, n_kp, occupied);
        if (tid == 0) *s_changed = 0;
        __syncthreads();
        for (int i = tid; i < n_pts; i += kThreads) {
            uint32_t* cl = cache + (size_t)i * kCacheWords;
            int k = -1;
            if (it == 0) {
                cl[0] = 0;   // (what a point that is skipped, or stopped by a gate before its window, leaves)
                k = evaluate(i, c_prev, cl);
            } else {
                const uint4 c0 = ((const uint4*)cl)[0];
                if (c0.x == kOverflow) k = evaluate(i, c_prev, nullptr);
                else if (c0.x) k = replay_cached(cl, c0, i, c_prev);
            }
            if (k >= 0) atomicMin(&c_cur[k], i);
        }
        __syncthreads();
        int diff = 0;
        for (int k = tid; k < n_kp; k += kThreads) diff |= (c_cur[k] != c_prev[k]);
        if (diff) *s_changed = 1;
        __syncthreads();
        const int changed = *s_changed;
        __syncthreads();
        if (!changed || it > n_pts) break;   // (point i is final after pass i + 1: the bound is never reached)
        { int* t = c_cur; c_cur = c_prev; c_prev = t; }
    }
    return it + 1;
}

// matched[k] = the point that claimed keypoint k and that keep(k, point) lets stand, else -1.  Returns how many this thread wrote.
template <class Keep>
__device__ __forceinline__ int write_claims(const int* claim, int n_kp, int32_t* matched, Keep keep) {
    int found = 0;
    for (int k = threadIdx.x; k < n_kp; k += kThreads) {
        const int o = claim[k];
        const bool ok = is_claimed(o) && keep(k, o);
        matched[k] = ok ? o : -1;
        found += ok ? 1 : 0;
    }
    return found;
}

// The rotation bin of a match (src/ORBmatcher.cc:475-480, :1562-1567): rot = angle1 - angle2 in float, + 360.0f when negative, round(rot * (1.0f / 30)) half away
// from zero, 30 becomes 0; -1 for what the reference's assert excludes
__device__ __forceinline__ int rot_bin(float angle1, float angle2) {
    float rot = angle1 - angle2;
    if (rot < 0.0f) rot += 360.0f;
    const float b = roundf(rot * (1.0f / kHistoLen));
    if (!(b >= 0.0f && b <= (float)kHistoLen)) return -1;
    const int bin = (int)b;
    return bin == kHistoLen ? 0 : bin;
}

// ORBmatcher::ComputeThreeMaxima (src/ORBmatcher.cc:1601-1642) over the sizes of the kHistoLen bins; one thread
__device__ __forceinline__ void three_maxima(const int* hist, int* ind) {
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < kHistoLen; i++) {
        const int sz = hist[i];
        if (sz > max1) { max3 = max2; max2 = max1; max1 = sz; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (sz > max2) { max3 = max2; max2 = sz; ind3 = ind2; ind2 = i; }
        else if (sz > max3) { max3 = sz; ind3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
    ind[0] = ind1; ind[1] = ind2; ind[2] = ind3;
}

// ---- host: the handle of the two projection operators ----

struct ProjHandle {
    int device = 0, max_problems = 0, max_kps = 0, max_pts = 0;
    size_t lds = 0;
    oslam::DeviceBuffer cache;   // [max_pts][kCacheWords] uint32: the candidates of every problem-point, written in pass 0
    oslam::StagePair io;         // staging of the host-pointer entry points: inputs | outputs
    std::mutex mu;
};

// max_keypoints of a create function against kMaxKps.  whose: "one keyframe's", "the frame's"; vectors: what the two int vectors hold
static inline int check_max_keypoints(const char* fn, int max_keypoints, const char* whose, const char* vectors) {
    if (max_keypoints <= kMaxKps) return OSLAM_OK;
    set_error("%s: max_keypoints %d > %d (%s keypoints, descriptors and grid, and %s, must fit 160 KiB of LDS)", fn, max_keypoints, kMaxKps, whose, vectors);
    return OSLAM_E_INVALID;
}

// (the attribute belongs to the kernel, not to the handle)
static inline int allow_full_lds(const char* fn, std::initializer_list<const void*> kernels) {
    for (const void* k : kernels) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(kMaxKps));
        if (e != hipSuccess) { set_error("%s: hipFuncSetAttribute failed: %s", fn, hipGetErrorString(e)); return OSLAM_E_HIP; }
    }
    return OSLAM_OK;
}

// <fn>(out, max_problems, max_keypoints, max_points_total, device) of a handle type H derived from ProjHandle
template <class H>
static int create_proj(const char* fn, const char* whose, H** out, int max_problems, int max_keypoints, int max_points_total, int device, std::initializer_list<const void*> kernels) {
    if (!out) { set_error("%s: out is NULL", fn); return OSLAM_E_INVALID; }
    *out = nullptr;
    if (max_problems < 1 || max_keypoints < 1 || max_points_total < 1) { set_error("%s: bad argument", fn); return OSLAM_E_INVALID; }
    OSLAM_CHECK(check_max_keypoints(fn, max_keypoints, whose, "two claim vectors"));
    const int ndev = oslam_device_count();
    if (ndev <= 0) return oslam::no_device(fn);
    if (device < 0 || device >= ndev) { set_error("%s: device out of range", fn); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(device));
    H* h = new H;
    h->device = device; h->max_problems = max_problems; h->max_kps = max_keypoints; h->max_pts = max_points_total; h->lds = lds_bytes(max_keypoints);
    int rc = h->cache.alloc((size_t)max_points_total * kCacheWords * sizeof(uint32_t));
    if (rc == OSLAM_OK) rc = allow_full_lds(fn, kernels);
    if (rc != OSLAM_OK) { delete h; return rc; }
    *out = h;
    return OSLAM_OK;
}

}  // namespace kf_stage
}  // namespace oslam
