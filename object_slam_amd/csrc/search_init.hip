// search_init.hip — ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (reference src/ORBmatcher.cc:405-520), the search of
// Tracking::MonocularInitialization (src/Tracking.cc:680-681), for batches of independent problems on gfx950 (include/oslam_hip.h, "Initialisation search").
// One launch, one workgroup per problem: the workgroup stages F2 in LDS (window_search.h: the grid and visiting order of GetFeaturesInArea) with
// vMatchedDistance and vnMatches21 in the two int vectors; the keys of F1 stay in global memory.
//  Phase A, all threads: every octave-0 key of F1 walks its window around its CARRIED point and caches, in visiting order, the candidates that can matter.
//  Phase B, one wavefront: the rule of :436-471 (skip what an earlier key holds at least as near, best and second best, displacement) is not "the lowest
//  index wins", so it is replayed literally in key order over the cached lines, lanes across a line's entries.
//  Then, all threads: the rotation histogram over every acceptance (a displaced key still counts), ComputeThreeMaxima, matches12, the carried points, counts.
// No inter-workgroup synchronisation and no atomics on global memory; the LDS atomics are counts: the outputs do not depend on the order the hardware runs
// anything in.  Product code; never includes oracle/.
#include <climits>
#include <cmath>
#include <mutex>

#include "common.h"
#include "stage_layout.h"
#include "window_search.h"

using oslam::set_error;
using namespace oslam::kf_stage;

struct oslam_init_match : ProjHandle {   // (max_pts: max_keys1_total; cache: one line per frames-1 row)
    oslam::DeviceBuffer ticks;           // [4] int64 of workgroup 0
};

namespace {

constexpr int kThLow = 50;                   // TH_LOW, src/ORBmatcher.cc:37
constexpr int kChunk = 64;                   // cache lines the replaying wavefront fetches at once
constexpr uint32_t kAccepted = 0x80000000u;  // word 0 of a replayed key's line: kAccepted | bestIdx2, or 0

struct InitArgs {
    const oslam_init_match_problem_t* problems;
    int n_problems, ncap;
    oslam_init_match_f1_rows_t f1;
    oslam_init_match_f2_rows_t f2;
    uint32_t* cache;
    float* prev;          // [f1.n_rows][2] vbPrevMatched
    int32_t* m12;         // [f1.n_rows]
    int32_t* count;       // n_matches
    int32_t* removed;     // may be NULL
    int32_t* displaced;   // may be NULL
    int32_t* overflow;    // may be NULL
    long long* ticks;     // [4]
    WindowCam cam;
    float nnratio;
    int check_ori;
};

// One record against the handle and the arrays.  `off <= rows - n` with 0 <= n and 0 <= rows cannot overflow, whatever off is.
struct InitExtent { int max_kps, rows1, rows2; };
__host__ __device__ inline bool record_counts_fit(const oslam_init_match_problem_t& p, const InitExtent& e) { return p.n1 >= 0 && p.n2 >= 0 && p.n2 <= e.max_kps; }
__host__ __device__ inline bool record_lies_inside(const oslam_init_match_problem_t& p, const InitExtent& e) {   // (after record_counts_fit)
    return p.off1 >= 0 && p.off2 >= 0 && p.off1 <= e.rows1 - p.n1 && p.off2 <= e.rows2 - p.n2;
}

// A candidate at distance d that does NOT pass this can never be best (d > TH_LOW), can never fail the ratio test as second best (bestDist <= TH_LOW <
// (float)d * nnratio) and is farther than every candidate that passes (the float product is monotonic in d): whether it is skipped changes nothing.
__device__ __forceinline__ bool can_matter(int d, float nnratio) { return !(d > kThLow && (float)kThLow < (float)d * nnratio); }

// LDS written by one lane of a wavefront and read by the others of the same wavefront
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the minimum over each group of eight lanes, in all eight (all lanes of the wavefront active)
__device__ __forceinline__ int min8(int v) {
    v = min(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, true));   // lane ^ 1
    v = min(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, true));   // lane ^ 2
    v = min(v, __builtin_amdgcn_ds_swizzle(v, 0x101F));              // lane ^ 4
    return v;
}

__global__ __launch_bounds__(kThreads) void k_search_init(InitArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const oslam_init_match_problem_t P = a.problems[b];
    // a record that does not fit the handle or the arrays: -2, nothing else is written (the host-pointer entry point refuses the call instead)
    const InitExtent ext = {a.ncap, a.f1.n_rows, a.f2.n_rows};
    if (!(record_counts_fit(P, ext) && record_lies_inside(P, ext) && P.windowSize >= 0)) {
        if (tid == 0) a.count[b] = -2;
        return;
    }
    const int n1 = P.n1, n2 = P.n2;
    const float r = (float)P.windowSize, nnratio = a.nnratio;
    const long long t0 = clock64();

    extern __shared__ __align__(16) uint8_t smem[];
    const Lds s = carve(smem, a.ncap);
    int* matchedDist = s.v0;   // [ncap] vMatchedDistance
    int* matches21 = s.v1;     // [ncap] vnMatches21
    __shared__ int s_wtot[kThreads / 64];
    __shared__ int s_hist[kHistoLen], s_ind[3];
    __shared__ int s_count, s_removed, s_displaced, s_overflow;
    __shared__ __align__(16) uint32_t s_lines[kChunk * kCacheWords];

    const oslam_keypoint_t* keys1 = a.f1.keysUn + P.off1;
    const oslam_keypoint_t* keys2 = a.f2.keysUn + P.off2;
    const uint8_t* desc1 = a.f1.desc + (size_t)P.off1 * 32;
    float* prev = a.prev + (size_t)P.off1 * 2;
    int32_t* m12 = a.m12 + P.off1;
    uint32_t* cache = a.cache + (size_t)P.off1 * kCacheWords;

    if (tid < kHistoLen) s_hist[tid] = 0;
    if (tid == 0) { s_count = 0; s_removed = 0; s_displaced = 0; s_overflow = 0; }
    for (int k = tid; k < n2; k += kThreads) { matchedDist[k] = INT_MAX; matches21[k] = -1; }   // :415-416
    // (stage_target begins and ends with a barrier)
    stage_target(s, keys2, a.f2.desc + (size_t)P.off2 * 32, n2, a.cam, s_wtot);
    const long long t1 = clock64();

    // ---- phase A: the candidates of every key (:420-442), none of which depends on another key ----
    int over = 0;
    for (int i = tid; i < n1; i += kThreads) {
        uint32_t* cl = cache + (size_t)i * kCacheWords;
        uint32_t nc = 0;
        if (keys1[i].octave == 0) {   // :421-423; a negative octave: the declared normalisation
            const float u = prev[2 * i], v = prev[2 * i + 1];
            if (isfinite(u) && isfinite(v)) {
                const uint4 q0 = ((const uint4*)(desc1 + (size_t)i * 32))[0], q1 = ((const uint4*)(desc1 + (size_t)i * 32))[1];
                walk_window<0, 0>(s, a.cam, u, v, r, 0, [&](int k) {
                    const int d = hamming256(q0, q1, s.desc + k * 8);
                    if (!can_matter(d, nnratio)) return;
                    if (nc < (uint32_t)kCacheCap) cl[1 + nc] = ((uint32_t)d << 16) | (uint32_t)k;
                    nc++;
                });
            }
        }
        cl[0] = nc <= (uint32_t)kCacheCap ? nc : kOverflow;
        over += nc > (uint32_t)kCacheCap ? 1 : 0;
    }
    if (over) atomicAdd(&s_overflow, over);
    __syncthreads();
    const long long t2 = clock64();

    // ---- phase B: :436-471 in key order, by one wavefront.  Every lane holds the same bestDist, bestDist2 and bestIdx2 of the key at hand. ----
    if (tid < 64) {
        const int lane = tid;
        int ndisp = 0;
        for (int base = 0; base < n1; base += kChunk) {
            const int nwords = min(kChunk, n1 - base) * kCacheWords;
            const uint32_t* g = cache + (size_t)base * kCacheWords;
            wave_lds_sync();   // the lines of the chunk before have been read
#pragma unroll
            for (int j = 0; j < kCacheWords; j++) {
                const int w = j * 64 + lane;
                s_lines[w] = w < nwords ? g[w] : 0u;
            }
            wave_lds_sync();
            unsigned long long todo = __ballot(s_lines[lane * kCacheWords] != 0u);   // a key without candidates changes nothing
            while (todo) {
                const int j = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int i1 = base + j;
                const uint32_t* line = s_lines + j * kCacheWords;
                const uint32_t cnt = line[0];
                int bestDist = INT_MAX, bestDist2 = INT_MAX, bestIdx2 = -1;
                if (cnt == kOverflow) {   // more candidates than a line holds: the window again, every lane the same walk
                    const uint4 q0 = ((const uint4*)(desc1 + (size_t)i1 * 32))[0], q1 = ((const uint4*)(desc1 + (size_t)i1 * 32))[1];
                    walk_window<0, 0>(s, a.cam, prev[2 * i1], prev[2 * i1 + 1], r, 0, [&](int k) {
                        const int d = hamming256(q0, q1, s.desc + k * 8);
                        if (!can_matter(d, nnratio)) return;
                        if (matchedDist[k] <= d) return;   // :444-445
                        if (d < bestDist) { bestDist2 = bestDist; bestDist = d; bestIdx2 = k; }
                        else if (d < bestDist2) bestDist2 = d;
                    });
                } else {   // lane t holds entry t; the key (dist, t) orders the entries as the strict `<` of :447 does: the first visited among equals
                    int key = INT_MAX;
                    if ((uint32_t)lane < cnt) {
                        const uint32_t e = line[1 + lane];
                        const int d = (int)(e >> 16);
                        if (!(matchedDist[e & 0xFFFFu] <= d)) key = (d << 3) | lane;
                    }
                    const int best = __builtin_amdgcn_readfirstlane(min8(key));
                    if (best != INT_MAX) {
                        // bestDist2 is the smallest distance among the other entries that are not skipped (:449, :453-456)
                        const int second = __builtin_amdgcn_readfirstlane(min8((key != INT_MAX && key != best) ? (key >> 3) : INT_MAX));
                        bestDist = best >> 3;
                        bestDist2 = second;
                        bestIdx2 = (int)(line[1 + (best & 7)] & 0xFFFFu);
                    }
                }
                const bool accept = bestDist <= kThLow && (float)bestDist < (float)bestDist2 * nnratio;   // :459-461
                if (accept && lane == 0) {
                    if (matches21[bestIdx2] >= 0) ndisp++;   // :463-467: that key's vnMatches12 is -1 from here on (matches12 is written from vnMatches21 below)
                    matches21[bestIdx2] = i1;
                    matchedDist[bestIdx2] = bestDist;
                }
                if (lane == 0) cache[(size_t)i1 * kCacheWords] = accept ? (kAccepted | (uint32_t)bestIdx2) : 0u;   // for the histogram
                wave_lds_sync();
            }
        }
        if (lane == 0) s_displaced = ndisp;
    }
    __syncthreads();
    const long long t3 = clock64();

    // ---- the histogram over every acceptance (:473-483: a key displaced later stays in its bin), and matches12 = -1 (:408) ----
    for (int i = tid; i < n1; i += kThreads) {
        const uint32_t w = cache[(size_t)i * kCacheWords];
        if (a.check_ori && (w & kAccepted)) {
            const int bin = rot_bin(keys1[i].angle, keys2[w & 0xFFFFu].angle);
            if (bin >= 0) atomicAdd(&s_hist[bin], 1);
        }
        m12[i] = -1;
    }
    __syncthreads();
    if (a.check_ori && tid == 0) three_maxima(s_hist, s_ind);
    __syncthreads();
    // ---- vnMatches12 is vnMatches21 read the other way; removal (:489-512); the carried points of the survivors (:514-517) ----
    int found = 0, removed = 0;
    for (int k = tid; k < n2; k += kThreads) {
        const int i1 = matches21[k];
        if (i1 < 0) continue;
        if (a.check_ori) {
            const int bin = rot_bin(keys1[i1].angle, keys2[k].angle);
            if (!(bin >= 0 && (bin == s_ind[0] || bin == s_ind[1] || bin == s_ind[2]))) { removed++; continue; }
        }
        m12[i1] = k;
        const float2 p = s.xy[k];
        prev[2 * i1] = p.x; prev[2 * i1 + 1] = p.y;
        found++;
    }
    if (found) atomicAdd(&s_count, found);
    if (removed) atomicAdd(&s_removed, removed);
    __syncthreads();
    if (tid == 0) {
        a.count[b] = s_count;
        if (a.removed) a.removed[b] = s_removed;
        if (a.displaced) a.displaced[b] = s_displaced;
        if (a.overflow) a.overflow[b] = s_overflow;
        if (b == 0) { a.ticks[0] = t1 - t0; a.ticks[1] = t2 - t1; a.ticks[2] = t3 - t2; a.ticks[3] = clock64() - t3; }
    }
}

int check_call(const char* fn, const oslam_init_match* h, int n_problems, const oslam_init_match_f1_rows_t* f1, const oslam_init_match_f2_rows_t* f2, const float* bounds,
               float nnratio) {
    if (!h || !f1 || !f2 || !bounds) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    if (n_problems < 0 || f1->n_rows < 0 || f2->n_rows < 0) {
        set_error("%s: %d problems, %d frames-1 rows, %d frames-2 rows: none may be negative", fn, n_problems, f1->n_rows, f2->n_rows);
        return OSLAM_E_CAPACITY;
    }
    if (n_problems > h->max_problems) { set_error("%s: %d problems exceed the handle's %d", fn, n_problems, h->max_problems); return OSLAM_E_CAPACITY; }
    if (f1->n_rows > h->max_pts) { set_error("%s: %d frames-1 rows exceed the handle's max_keys1_total %d", fn, f1->n_rows, h->max_pts); return OSLAM_E_CAPACITY; }
    if (!(bounds[2] > bounds[0]) || !(bounds[3] > bounds[1])) { set_error("%s: empty image bounds", fn); return OSLAM_E_INVALID; }
    if (!(std::isfinite(nnratio) && nnratio > 0.0f)) { set_error("%s: nnratio must be finite and positive", fn); return OSLAM_E_INVALID; }
    if ((f1->n_rows > 0 && (!f1->keysUn || !f1->desc)) || (f2->n_rows > 0 && (!f2->keysUn || !f2->desc))) { set_error("%s: a per-key array is NULL", fn); return OSLAM_E_INVALID; }
    return OSLAM_OK;
}

// The device entry point: checks, the argument block, one launch
int launch(const char* fn, oslam_init_match* h, int n_problems, const oslam_init_match_problem_t* d_problems, const oslam_init_match_f1_rows_t* f1,
           const oslam_init_match_f2_rows_t* f2, const float* bounds, float nnratio, int check_orientation, float* d_prev, int32_t* d_m12, int32_t* d_count, int32_t* d_removed,
           int32_t* d_displaced, int32_t* d_overflow, void* stream) {
    OSLAM_CHECK(check_call(fn, h, n_problems, f1, f2, bounds, nnratio));
    if (n_problems == 0) return OSLAM_OK;
    if (!d_problems || !d_count || (f1->n_rows > 0 && (!d_prev || !d_m12))) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    InitArgs a;
    a.problems = d_problems; a.n_problems = n_problems; a.ncap = h->max_kps;
    a.f1 = *f1; a.f2 = *f2; a.cache = h->cache.as<uint32_t>();
    a.prev = d_prev; a.m12 = d_m12; a.count = d_count; a.removed = d_removed; a.displaced = d_displaced; a.overflow = d_overflow; a.ticks = h->ticks.as<long long>();
    const oslam_camera_t none = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // (nothing is projected: the search reads the bounds and the grid of the block only)
    const float level0[1] = {1.0f};
    fill_window_cam(a.cam, &none, bounds, level0, 1, 1.0f);
    a.nnratio = nnratio;
    a.check_ori = check_orientation ? 1 : 0;
    hipLaunchKernelGGL(k_search_init, dim3(n_problems), dim3(kThreads), h->lds, (hipStream_t)stream, a);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

}  // namespace

extern "C" {

void oslam_init_match_destroy(oslam_init_match_t* h) {
    if (!h) return;
    delete h;
}

int oslam_init_match_create(oslam_init_match_t** out, int max_problems, int max_keypoints, int max_keys1_total, int device) {
    OSLAM_CHECK(create_proj("oslam_init_match_create", "F2's", out, max_problems, max_keypoints, max_keys1_total, device, {(const void*)k_search_init}));
    int rc = (*out)->ticks.alloc(4 * sizeof(long long));
    if (rc == OSLAM_OK && hipMemset((*out)->ticks.ptr(), 0, 4 * sizeof(long long)) != hipSuccess) { set_error("oslam_init_match_create: hipMemset failed"); rc = OSLAM_E_HIP; }
    if (rc != OSLAM_OK) { delete *out; *out = nullptr; }
    return rc;
}

int oslam_init_match_last_phase_ticks(oslam_init_match_t* h, int64_t ticks[4]) {
    if (!h || !ticks) { set_error("oslam_init_match_last_phase_ticks: NULL argument"); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    OSLAM_HIP_CHECK(hipDeviceSynchronize());
    OSLAM_HIP_CHECK(hipMemcpy(ticks, h->ticks.ptr(), 4 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return OSLAM_OK;
}

int oslam_match_search_for_initialization_batch_device(oslam_init_match_t* h, int n_problems, const oslam_init_match_problem_t* d_problems,
                                                       const oslam_init_match_f1_rows_t* frames1, const oslam_init_match_f2_rows_t* frames2, const float bounds[4], float nnratio,
                                                       int check_orientation, float* d_prev_matched, int32_t* d_matches12, int32_t* d_n_matches, int32_t* d_n_removed,
                                                       int32_t* d_n_displaced, int32_t* d_n_overflow, void* stream) {
    return launch("oslam_match_search_for_initialization_batch_device", h, n_problems, d_problems, frames1, frames2, bounds, nnratio, check_orientation, d_prev_matched,
                  d_matches12, d_n_matches, d_n_removed, d_n_displaced, d_n_overflow, stream);
}

// The host-pointer entry point: the records checked, one block up, launch(), the outputs down
int oslam_match_search_for_initialization_batch(oslam_init_match_t* h, int n_problems, const oslam_init_match_problem_t* problems, const oslam_init_match_f1_rows_t* f1,
                                                const oslam_init_match_f2_rows_t* f2, const float bounds[4], float nnratio, int check_orientation, float* prev_matched,
                                                int32_t* matches12, int32_t* n_matches, int32_t* n_removed, int32_t* n_displaced, int32_t* n_overflow) {
    const char* fn = "oslam_match_search_for_initialization_batch";
    OSLAM_CHECK(check_call(fn, h, n_problems, f1, f2, bounds, nnratio));
    if (n_problems == 0) return OSLAM_OK;
    if (!problems || !n_matches || (f1->n_rows > 0 && (!prev_matched || !matches12))) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    const InitExtent ext = {h->max_kps, f1->n_rows, f2->n_rows};
    for (int b = 0; b < n_problems; b++) {
        const oslam_init_match_problem_t& p = problems[b];
        if (!record_counts_fit(p, ext)) {
            set_error("%s: problem %d has %d and %d keys (F2: at most %d): none may be negative", fn, b, p.n1, p.n2, ext.max_kps);
            return OSLAM_E_CAPACITY;
        }
        if (!record_lies_inside(p, ext)) {
            set_error("%s: problem %d (off1 %d, off2 %d) lies outside the %d frames-1 rows / %d frames-2 rows", fn, b, p.off1, p.off2, ext.rows1, ext.rows2);
            return OSLAM_E_INVALID;
        }
        if (p.windowSize < 0) { set_error("%s: problem %d has windowSize %d", fn, b, p.windowSize); return OSLAM_E_INVALID; }
    }
    std::lock_guard<std::mutex> lock(h->mu);
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t np = (size_t)n_problems, M1 = (size_t)f1->n_rows, M2 = (size_t)f2->n_rows;
    oslam::StageLayout lay;   // one block, inputs then what is read and written: one upload, one download
    const auto fProb = lay.add<oslam_init_match_problem_t>(np);
    const auto fK1 = lay.add<oslam_keypoint_t>(M1), fK2 = lay.add<oslam_keypoint_t>(M2);
    const auto fD1 = lay.add<uint8_t>(M1 * 32), fD2 = lay.add<uint8_t>(M2 * 32);
    const auto fPrev = lay.add<float>(M1 * 2);
    const auto fM12 = lay.add<int32_t>(M1), fCount = lay.add<int32_t>(np), fRem = lay.add<int32_t>(np, n_removed != nullptr), fDisp = lay.add<int32_t>(np, n_displaced != nullptr),
               fOver = lay.add<int32_t>(np, n_overflow != nullptr);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fProb, ph, problems); put(fK1, ph, f1->keysUn); put(fK2, ph, f2->keysUn); put(fD1, ph, f1->desc); put(fD2, ph, f2->desc);
    // the caller's rows travel too: rows no problem owns, and those of a problem the kernel leaves alone, come back as they were
    put(fPrev, ph, (const float*)prev_matched); put(fM12, ph, (const int32_t*)matches12); put(fCount, ph, (const int32_t*)n_matches); put(fRem, ph, (const int32_t*)n_removed);
    put(fDisp, ph, (const int32_t*)n_displaced); put(fOver, ph, (const int32_t*)n_overflow);
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, nullptr));
    const oslam_init_match_f1_rows_t d1 = {f1->n_rows, at(fK1, pd), at(fD1, pd)};
    const oslam_init_match_f2_rows_t d2 = {f2->n_rows, at(fK2, pd), at(fD2, pd)};
    OSLAM_CHECK(launch(fn, h, n_problems, at(fProb, pd), &d1, &d2, bounds, nnratio, check_orientation, at(fPrev, pd), at(fM12, pd), at(fCount, pd), at(fRem, pd), at(fDisp, pd),
                       at(fOver, pd), nullptr));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fPrev.off, pd + fPrev.off, lay.total() - fPrev.off, hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(fPrev, ph, prev_matched); get(fM12, ph, matches12); get(fCount, ph, n_matches); get(fRem, ph, n_removed); get(fDisp, ph, n_displaced); get(fOver, ph, n_overflow);
    return OSLAM_OK;
}

}  // extern "C"
