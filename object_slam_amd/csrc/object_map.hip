// object_map.hip — the object layer's map maintenance for batches on gfx950 (include/oslam_hip.h, "Object map maintenance"):
//  - Object3D::RejectOutliers (reference src/ObjectTypes.cc:152-162: RejectOutliersTEST5 :590-628, RejectOutliersTEST7 :661-764), the new-object path of
//    Tracking::UpdateCurrentObject (src/Tracking.cc:1113-1199) and Object3D::CalculateCenterAndSize (:805-833): k_object_map, one workgroup per point list.
//    The float sums that the reference runs in list order are run in list order by one wavefront over rows staged in LDS; the all-pairs work of the Euclidean
//    clustering is where the other lanes go: positions and one component label per point live in LDS, and the components are found by rounds of minimum
//    hooking onto roots followed by pointer jumping, so the number of all-pairs rounds is logarithmic in the length of a chain of points.
//  - Map::ObjectMapRegularization's merge sets (src/Map.cc:47-112): k_merge_sets, one workgroup per map: all pair ratios in parallel, then one wavefront
//    replays the set construction in pair order, a set per lane.
// No atomics on global memory, no inter-workgroup synchronisation: every output is bit-identical from run to run.  Product code; never includes oracle/.
#include <cfloat>
#include <cmath>
#include <mutex>

#include "common.h"
#include "stage_layout.h"

using oslam::set_error;
using namespace oslam;

namespace {

constexpr int kThreads = 1024;   // of k_object_map
constexpr int kPer = 4;          // points per thread of one staged chunk: kPer * kThreads >= OSLAM_OBJMAP_MAX_CLUSTER_POINTS
constexpr int kMergeThreads = 256;
constexpr int kMaxObj = OSLAM_OBJMAP_MAX_OBJECTS;
constexpr int kOpReject = 0, kOpExtent = 1;
static_assert(kPer * kThreads >= OSLAM_OBJMAP_MAX_CLUSTER_POINTS, "a chunk is kPer points per thread");
static_assert(sizeof(oslam_objmap_result_t) == 80, "the records are part of the ABI");

}  // namespace

struct oslam_objmap {
    int device = 0, max_problems = 0, cap = 0, max_obj = 0;
    oslam::StagePair io;          // staging of the host-pointer entry points
    std::mutex mu;
    bool timing = false;          // oslam_objmap_set_timing: events before and after the launch
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~oslam_objmap() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

namespace {

struct MapArgs {
    const oslam_objmap_problem_t* problems;
    const float* pos;
    const int32_t *lcnt, *lsum;
    uint8_t* keep;
    int32_t* cluster;
    oslam_objmap_result_t* res;
    int n_rows, cap, op;
};

__host__ __device__ inline bool problem_valid(const oslam_objmap_problem_t& P, int n_rows, int op) {
    return P.n >= 0 && P.off >= 0 && P.off <= n_rows - P.n && (op == kOpExtent || P.mode == OSLAM_OBJMAP_MODE_UPDATE || P.mode == OSLAM_OBJMAP_MODE_NEW_OBJECT);
}
__host__ __device__ inline bool problem_streams(const oslam_objmap_problem_t& P, int op) {   // no clustering: any n
    return op == kOpExtent || (P.mode == OSLAM_OBJMAP_MODE_UPDATE && P.n > OSLAM_OBJMAP_TEST5_ABOVE);
}

__device__ __forceinline__ float quiet(float v) { return v != v ? __int_as_float(0x7fc00000) : v; }   // every NaN written is this one

// Object3D::isMpBad (:143-148) over MapPoint::GetLabelProb (src/MapPoint.cc:109-137)
__device__ __forceinline__ bool label_bad(int cnt, int sum) {
    const float prob = sum == 0 ? 0.0f : (float)((double)cnt / (double)sum);
    return (double)prob < 0.5;
}

// cv::norm of the float vector (x, y, z): squares and sum in double
__device__ __forceinline__ double norm3(float x, float y, float z) { return sqrt((double)x * (double)x + (double)y * (double)y + (double)z * (double)z); }

// lane k's value in every lane; k is the same in all lanes
__device__ __forceinline__ float lane_value(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }

extern __shared__ float s_dyn[];   // [4][cap]: x, y, z and one word per point

__global__ __launch_bounds__(kThreads) void k_object_map(MapArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const oslam_objmap_problem_t P = a.problems[b];
    oslam_objmap_result_t* R = a.res + b;
    if (!problem_valid(P, a.n_rows, a.op)) {   // a refusal: the status and nothing else
        if (tid == 0) R->status = OSLAM_OBJMAP_REFUSED_RECORD;
        return;
    }
    const bool extent = a.op == kOpExtent, streams = problem_streams(P, a.op), update = P.mode == OSLAM_OBJMAP_MODE_UPDATE;
    const int n = P.n, cap = a.cap;
    if (!streams && n > cap) {
        if (tid == 0) R->status = OSLAM_OBJMAP_REFUSED_CAPACITY;
        return;
    }
    float *sx = s_dyn, *sy = sx + cap, *sz = sy + cap, *sw = sz + cap;
    int* si = (int*)sw;
    const float* pos = a.pos + 3 * (size_t)P.off;
    __shared__ float s_stat[4];   // CandidatesCenter, CandidatesStdDev
    __shared__ int s_int[4];      // N_candidates, the clusters, the two "something changed" flags

    // ---- the scan in list order (:674-696): a chunk of rows is staged by all threads (x, y, z, and square * square or -1 for a bad row), then the first wavefront adds.
    //      The clustering paths have one chunk, which stays staged. ----
    float cx = 0.0f, cy = 0.0f, cz = 0.0f, thr = 0.0f, stddev = 0.0f;
    int nc = 0;
    if (!extent) {
        float ax = 0.0f, ay = 0.0f, az = 0.0f, sq = 0.0f;   // (the first wavefront's)
        int cnt = 0;
        for (int c0 = 0; c0 < n || c0 == 0; c0 += cap) {
            const int m = min(cap, n - c0);
            for (int k = 0; k < kPer; k++) {
                const int l = tid + k * kThreads;
                if (l >= m) break;
                const int r = c0 + l;
                const float x = pos[3 * (size_t)r], y = pos[3 * (size_t)r + 1], z = pos[3 * (size_t)r + 2];
                const bool bad = update && label_bad(a.lcnt[P.off + r], a.lsum[P.off + r]);
                const float square = (float)norm3(x, y, z);
                sx[l] = bad ? NAN : x; sy[l] = y; sz[l] = z;   // (a NaN is no point's neighbour)
                sw[l] = bad ? -1.0f : square * square;
            }
            __syncthreads();
            if (tid < 64) {   // 64 rows a step into the lanes' registers; the adds run in list order over broadcasts of them, the same in every lane
                for (int l0 = 0; l0 < m; l0 += 64) {
                    const int l = l0 + tid;
                    float w = -1.0f, x = 0.0f, y = 0.0f, z = 0.0f;
                    if (l < m) { w = sw[l]; x = sx[l]; y = sy[l]; z = sz[l]; }
                    const int rows = min(64, m - l0);
                    for (int k = 0; k < rows; k++) {
                        const float wk = lane_value(w, k);
                        if (wk == -1.0f) continue;
                        ax = ax + lane_value(x, k); ay = ay + lane_value(y, k); az = az + lane_value(z, k);
                        sq = sq + wk;
                        cnt++;
                    }
                }
            }
            if (streams) __syncthreads();   // the next chunk overwrites this one
        }
        if (tid == 0) {
            const float inv = (float)(1.0 / (double)cnt);   // Mat / double
            ax = ax * inv; ay = ay * inv; az = az * inv;
            const double nrm = norm3(ax, ay, az);
            s_stat[0] = ax; s_stat[1] = ay; s_stat[2] = az;
            s_stat[3] = (float)sqrt((double)sq / (double)cnt - nrm * nrm);   // the simplified variance: negative far from the origin, the root NaN
            s_int[0] = cnt;
        }
        __syncthreads();
        cx = s_stat[0]; cy = s_stat[1]; cz = s_stat[2]; stddev = s_stat[3]; nc = s_int[0];
        thr = 3.0f * stddev;
    }

    // ---- pcl::EuclideanClusterExtraction (:711-720), tolerance 0.1: the connected components of "d2 < tol2" over the finite candidates ----
    float px[kPer], py[kPer], pz[kPer];
    bool cand[kPer], incl[kPer];
    int root[kPer], size[kPer];
    int rounds = 0, ncl = 0;
    if (!streams) {
        for (int k = 0; k < kPer; k++) {
            const int l = tid + k * kThreads;
            cand[k] = incl[k] = false; root[k] = -1; size[k] = 0; px[k] = py[k] = pz[k] = 0.0f;
            if (l < n) {
                px[k] = sx[l]; py[k] = sy[l]; pz[k] = sz[l];
                cand[k] = !(sw[l] == -1.0f);
                incl[k] = cand[k] && isfinite(px[k]) && isfinite(py[k]) && isfinite(pz[k]);   // the kd-tree skips a non-finite point
            }
        }
        __syncthreads();
        for (int k = 0; k < kPer; k++) {
            const int l = tid + k * kThreads;
            if (l < n) si[l] = incl[k] ? l : -1;
        }
        if (tid == 0) s_int[2] = 0;
        __syncthreads();
        const float tol2 = (float)(0.1 * 0.1);
        while (true) {
            rounds++;
            // every point: the smallest label among its neighbours.  Labels are only read here; every point names its root.
            int old[kPer], best[kPer];
            for (int k = 0; k < kPer; k++) { old[k] = incl[k] ? si[tid + k * kThreads] : -1; best[k] = old[k]; }
            for (int j = 0; j < n; j++) {
                const int pj = si[j];   // (the same j in every lane: a broadcast)
                if (pj < 0) continue;
                const float xj = sx[j], yj = sy[j], zj = sz[j];
#pragma unroll
                for (int k = 0; k < kPer; k++) {
                    const float dx = px[k] - xj, dy = py[k] - yj, dz = pz[k] - zj;
                    const float d2 = dx * dx + dy * dy + dz * dz;   // FLANN L2_Simple<float>
                    if (d2 < tol2 && pj < best[k]) best[k] = pj;     // (a point outside the clustering never lowers its label of -1)
                }
            }
            __syncthreads();
            // every root hooks onto the smallest label its members saw: integer minima in LDS, whose outcome no order changes
            bool hooked = false;
            for (int k = 0; k < kPer; k++)
                if (incl[k] && best[k] < old[k]) { atomicMin(&si[old[k]], best[k]); hooked = true; }
            if (hooked) s_int[2] = 1;
            __syncthreads();
            const bool any = s_int[2] != 0;
            __syncthreads();
            if (!any) break;
            // pointer jumping until every point names its root again.  Labels fall along every pointer, so the fixed point is the same whatever the
            // order in which lanes read and write.
            while (true) {
                if (tid == 0) { s_int[2] = 0; s_int[3] = 0; }
                __syncthreads();
                bool moved = false;
                for (int k = 0; k < kPer; k++) {
                    if (!incl[k]) continue;
                    const int l = tid + k * kThreads, p = si[l], g = si[p];
                    if (g != p) { si[l] = g; moved = true; }
                }
                if (moved) s_int[3] = 1;
                __syncthreads();
                const bool again = s_int[3] != 0;
                __syncthreads();
                if (!again) break;
            }
        }
        for (int k = 0; k < kPer; k++) root[k] = incl[k] ? si[tid + k * kThreads] : -1;
        // the clusters' sizes, in the words that held x (the positions are in registers)
        int* cntw = (int*)sx;
        if (tid == 0) s_int[1] = 0;
        __syncthreads();
        for (int k = 0; k < kPer; k++) { const int l = tid + k * kThreads; if (l < n) cntw[l] = 0; }
        __syncthreads();
        for (int k = 0; k < kPer; k++)
            if (incl[k]) { atomicAdd(&cntw[root[k]], 1); if (root[k] == tid + k * kThreads) atomicAdd(&s_int[1], 1); }
        __syncthreads();
        for (int k = 0; k < kPer; k++) size[k] = incl[k] ? cntw[root[k]] : 0;
        ncl = s_int[1];
        __syncthreads();
    }
    const bool shortcut = !extent && !streams && !update && ncl == 1 && nc > 5;   // src/Tracking.cc:1158

    // ---- the rules (:734-758), then CalculateCenterAndSize (:805-833) of what is kept: staged by all threads, added in list order by the first wavefront ----
    float fx = 0.0f, fy = 0.0f, fz = 0.0f, mnx = INFINITY, mny = INFINITY, mnz = INFINITY, mxx = -INFINITY, mxy = -INFINITY, mxz = -INFINITY;
    int nk = 0;
    for (int c0 = 0; c0 < n; c0 += cap) {
        const int m = min(cap, n - c0);
        for (int k = 0; k < kPer; k++) {
            const int l = tid + k * kThreads;
            if (l >= m) break;
            const int r = c0 + l;
            float x, y, z;
            bool kp = true;
            if (streams) {
                x = pos[3 * (size_t)r]; y = pos[3 * (size_t)r + 1]; z = pos[3 * (size_t)r + 2];
                if (!extent) {   // RejectOutliersTEST5 (:618-625)
                    kp = !label_bad(a.lcnt[P.off + r], a.lsum[P.off + r]);
                    if (kp && (float)norm3(cx - x, cy - y, cz - z) > thr) kp = false;
                }
            } else {
                x = px[k]; y = py[k]; z = pz[k];
                kp = cand[k];
                if (kp && incl[k] && !shortcut) {
                    const float ratio = (float)((double)size[k] / (double)nc);
                    if ((double)ratio < 0.1 && nc > 15) kp = false;
                    else if ((float)norm3(x - cx, y - cy, z - cz) > thr) kp = false;
                }
            }
            if (!extent) { a.keep[P.off + r] = kp ? 1 : 0; a.cluster[P.off + r] = streams ? -1 : root[k]; }
            sx[l] = x; sy[l] = y; sz[l] = z; si[l] = kp ? 1 : 0;
        }
        __syncthreads();
        if (tid < 64) {
            for (int l0 = 0; l0 < m; l0 += 64) {
                const int l = l0 + tid;
                int kept = 0;
                float vx = 0.0f, vy = 0.0f, vz = 0.0f;
                if (l < m) { kept = si[l]; vx = sx[l]; vy = sy[l]; vz = sz[l]; }
                const unsigned long long mask = __ballot(kept != 0);
                const int rows = min(64, m - l0);
                for (int k = 0; k < rows; k++) {
                    if (!((mask >> k) & 1ull)) continue;
                    const float x = lane_value(vx, k), y = lane_value(vy, k), z = lane_value(vz, k);
                    fx = fx + x; fy = fy + y; fz = fz + z;
                    if (x < mnx) mnx = x;
                    if (x > mxx) mxx = x;
                    if (y < mny) mny = y;
                    if (y > mxy) mxy = y;
                    if (z < mnz) mnz = z;
                    if (z > mxz) mxz = z;
                    nk++;
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        R->status = OSLAM_OBJMAP_DONE;
        R->n_kept = nk;
        if (!extent) {
            R->n_candidates = nc; R->n_clusters = ncl; R->rounds = rounds;
            R->path = streams ? OSLAM_OBJMAP_PATH_TEST5 : (shortcut ? OSLAM_OBJMAP_PATH_SHORTCUT : OSLAM_OBJMAP_PATH_TEST7);
            R->std_dev = quiet(stddev);
            R->candidates_center[0] = quiet(cx); R->candidates_center[1] = quiet(cy); R->candidates_center[2] = quiet(cz);
        }
        if (nk > 0) {   // (an empty list leaves the members as they were, :808)
            const float d = (float)nk;   // Eigen::Vector3f / double
            R->center[0] = quiet(fx / d); R->center[1] = quiet(fy / d); R->center[2] = quiet(fz / d);
            R->bbox[0] = mxx; R->bbox[1] = mxy; R->bbox[2] = mxz; R->bbox[3] = mnx; R->bbox[4] = mny; R->bbox[5] = mnz;
        }
    }
}

// ------------------------------------------------------------------ merge sets ------------------------------------------------------------------

struct MergeArgs {
    const oslam_objmap_merge_problem_t* problems;
    const int32_t *label, *track;
    const float* bbox;
    int bbox_stride, n_rows, n_pairs, max_obj;
    float* ratio;
    uint8_t* member;
    int32_t *target, *n_sets, *status;
};

__host__ __device__ inline bool merge_valid(const oslam_objmap_merge_problem_t& P, int n_rows, int n_pairs) {
    return P.n >= 0 && P.off_obj >= 0 && P.off_obj <= n_rows - P.n && P.off_pair >= 0 && P.off_pair <= n_pairs && (long long)P.n * P.n <= (long long)(n_pairs - P.off_pair);
}

// ObjectMatcher::Compute3DOverlapRatio (src/ObjectMatcher.cc:844-873); boxes as max x, y, z, min x, y, z
__device__ __forceinline__ float overlap_ratio(const float* b1, const float* b2) {
    const float area1 = (b1[0] - b1[3]) * (b1[1] - b1[4]) * (b1[2] - b1[5]);
    const float area2 = (b2[0] - b2[3]) * (b2[1] - b2[4]) * (b2[2] - b2[5]);
    const float MinX = b1[3] < b2[3] ? b2[3] : b1[3], MaxX = b2[0] < b1[0] ? b2[0] : b1[0];   // std::max(a, b), std::min(a, b)
    const float MinY = b1[4] < b2[4] ? b2[4] : b1[4], MaxY = b2[1] < b1[1] ? b2[1] : b1[1];
    const float MinZ = b1[5] < b2[5] ? b2[5] : b1[5], MaxZ = b2[2] < b1[2] ? b2[2] : b1[2];
    if (MinX >= MaxX || MinY >= MaxY || MinZ >= MaxZ) return 0.0f;
    const float inter = (MaxX - MinX) * (MaxY - MinY) * (MaxZ - MinZ);
    const float q1 = inter / area1, q2 = inter / area2;
    return q1 < q2 ? q2 : q1;
}

__global__ __launch_bounds__(kMergeThreads) void k_merge_sets(MergeArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const oslam_objmap_merge_problem_t P = a.problems[b];
    if (!merge_valid(P, a.n_rows, a.n_pairs)) {
        if (tid == 0) a.status[b] = OSLAM_OBJMAP_REFUSED_RECORD;
        return;
    }
    const int n = P.n;
    if (n > a.max_obj) {
        if (tid == 0) a.status[b] = OSLAM_OBJMAP_REFUSED_CAPACITY;
        return;
    }
    __shared__ float s_box[kMaxObj][6];
    __shared__ int s_label[kMaxObj], s_track[kMaxObj];
    __shared__ unsigned int s_merge[kMaxObj][kMaxObj / 32];   // bit j of row i: pair (i, j) merges
    for (int t = tid; t < n * 6; t += kMergeThreads) s_box[t / 6][t % 6] = a.bbox[(size_t)(P.off_obj + t / 6) * a.bbox_stride + t % 6];
    for (int t = tid; t < n; t += kMergeThreads) { s_label[t] = a.label[P.off_obj + t]; s_track[t] = a.track[P.off_obj + t]; }
    for (int t = tid; t < n * (kMaxObj / 32); t += kMergeThreads) s_merge[t / (kMaxObj / 32)][t % (kMaxObj / 32)] = 0u;
    __syncthreads();

    // ---- phase 1: every pair's ratio and CheckIfMerge (src/Map.cc:47-65); none depends on a set ----
    for (int p = tid; p < n * n; p += kMergeThreads) {
        const int i = p / n, j = p % n;
        if (i >= j) continue;
        const float r = overlap_ratio(s_box[i], s_box[j]);
        a.ratio[P.off_pair + p] = quiet(r);
        if (s_label[i] == s_label[j] && s_track[i] != s_track[j] && (double)r > 0.4) atomicOr(&s_merge[i][j >> 5], 1u << (j & 31));
    }
    __syncthreads();

    // ---- phase 2: the loop over the pairs with its sets (:72-100), one wavefront, lane s = set s (a new set needs a pair none of whose indices is in a
    //      set, so there are at most n / 2 <= 64); its members are bits of two words ----
    if (tid < 64) {
        const int lane = tid;
        unsigned long long m0 = 0ull, m1 = 0ull;
        int nsets = 0;
        for (int i = 0; i < n; i++) {
            const unsigned long long bi0 = i < 64 ? 1ull << i : 0ull, bi1 = i < 64 ? 0ull : 1ull << (i - 64);
            for (int w = 0; w < kMaxObj / 32; w++) {
                unsigned int bits = s_merge[i][w];
                while (bits) {
                    const int j = 32 * w + __ffs(bits) - 1;
                    bits &= bits - 1;
                    const unsigned long long bj0 = j < 64 ? 1ull << j : 0ull, bj1 = j < 64 ? 0ull : 1ull << (j - 64);
                    const bool has = lane < nsets && (((m0 & (bi0 | bj0)) | (m1 & (bi1 | bj1))) != 0ull);
                    if (has) { m0 |= bi0 | bj0; m1 |= bi1 | bj1; }
                    if (!__ballot(has)) {
                        if (lane == nsets) { m0 = bi0 | bj0; m1 = bi1 | bj1; }
                        nsets++;
                    }
                }
            }
        }
        if (lane < nsets) {
            // MergeObject's target (:116-129): the largest mTrackID, the first among equals
            int best = -1, bestId = 0;
            for (int o = 0; o < n; o++) {
                const bool in = ((o < 64 ? m0 >> o : m1 >> (o - 64)) & 1ull) != 0ull;
                a.member[(size_t)P.off_pair + (size_t)lane * n + o] = in ? 1 : 0;
                if (in && (best < 0 || s_track[o] > bestId)) { best = o; bestId = s_track[o]; }
            }
            a.target[P.off_obj + lane] = best;
        }
        if (lane == 0) { a.n_sets[b] = nsets; a.status[b] = OSLAM_OBJMAP_DONE; }
    }
}

// ------------------------------------------------------------------ host ------------------------------------------------------------------

int check_call(const char* fn, const oslam_objmap* h, int n_problems, int n_rows) {
    if (!h) { set_error("%s: handle is NULL", fn); return OSLAM_E_INVALID; }
    if (n_problems < 0 || n_rows < 0) { set_error("%s: %d problems, %d rows: none may be negative", fn, n_problems, n_rows); return OSLAM_E_CAPACITY; }
    if (n_problems > h->max_problems) { set_error("%s: %d problems exceed the handle's %d", fn, n_problems, h->max_problems); return OSLAM_E_CAPACITY; }
    return OSLAM_OK;
}

// what a host entry point can see and a device one cannot: the records
int check_problems(const char* fn, const oslam_objmap* h, int n_problems, const oslam_objmap_problem_t* problems, int n_rows, int op) {
    for (int b = 0; b < n_problems; b++) {
        const oslam_objmap_problem_t& P = problems[b];
        if (!problem_valid(P, n_rows, op)) { set_error("%s: problem %d (rows %d + %d of %d, mode %d) is not valid", fn, b, P.off, P.n, n_rows, P.mode); return OSLAM_E_INVALID; }
        if (!problem_streams(P, op) && P.n > h->cap) { set_error("%s: problem %d clusters %d points, above the handle's max_cluster_points %d", fn, b, P.n, h->cap); return OSLAM_E_CAPACITY; }
    }
    return OSLAM_OK;
}

int launch_map(const char* fn, oslam_objmap* h, int op, int n_problems, const oslam_objmap_problem_t* d_problems, int n_rows, const float* d_pos, const int32_t* d_lcnt,
               const int32_t* d_lsum, uint8_t* d_keep, int32_t* d_cluster, oslam_objmap_result_t* d_results, bool labels_needed, hipStream_t stream) {
    OSLAM_CHECK(check_call(fn, h, n_problems, n_rows));
    if (n_problems == 0) return OSLAM_OK;
    if (!d_problems || !d_results || (n_rows > 0 && (!d_pos || (op == kOpReject && (!d_keep || !d_cluster || (labels_needed && (!d_lcnt || !d_lsum))))))) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    MapArgs a;
    a.problems = d_problems; a.pos = d_pos; a.lcnt = d_lcnt; a.lsum = d_lsum; a.keep = d_keep; a.cluster = d_cluster; a.res = d_results;
    a.n_rows = n_rows; a.cap = h->cap; a.op = op;
    if (h->timing) OSLAM_HIP_CHECK(hipEventRecord(h->ev[0], stream));
    hipLaunchKernelGGL(k_object_map, dim3(n_problems), dim3(kThreads), (size_t)h->cap * 16, stream, a);
    if (h->timing) OSLAM_HIP_CHECK(hipEventRecord(h->ev[1], stream));
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int run_map_host(const char* fn, oslam_objmap* h, int op, int n_problems, const oslam_objmap_problem_t* problems, int n_rows, const float* pos, const int32_t* lcnt,
                 const int32_t* lsum, uint8_t* keep, int32_t* cluster, oslam_objmap_result_t* results) {
    OSLAM_CHECK(check_call(fn, h, n_problems, n_rows));
    if (n_problems == 0) return OSLAM_OK;
    if (!problems || !results) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_CHECK(check_problems(fn, h, n_problems, problems, n_rows, op));
    bool labels_needed = false;
    for (int b = 0; b < n_problems && op == kOpReject; b++) labels_needed |= problems[b].mode == OSLAM_OBJMAP_MODE_UPDATE && problems[b].n > 0;
    const bool rej = op == kOpReject;
    if (n_rows > 0 && (!pos || (rej && (!keep || !cluster || (labels_needed && (!lcnt || !lsum)))))) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    std::lock_guard<std::mutex> lock(h->mu);
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t np = (size_t)n_problems, nr = (size_t)n_rows;
    const bool labels = rej && lcnt && lsum;
    oslam::StageLayout lay;   // inputs, then what is read and written: one upload, one download
    const auto fProb = lay.add<oslam_objmap_problem_t>(np);
    const auto fPos = lay.add<float>(nr * 3);
    const auto fLc = lay.add<int32_t>(nr, labels), fLs = lay.add<int32_t>(nr, labels);
    const auto fKeep = lay.add<uint8_t>(nr, rej);   // from here on: read and written
    const auto fClu = lay.add<int32_t>(nr, rej);
    const auto fRes = lay.add<oslam_objmap_result_t>(np);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fProb, ph, problems); put(fPos, ph, pos); put(fLc, ph, lcnt); put(fLs, ph, lsum);
    put(fKeep, ph, (const uint8_t*)keep); put(fClu, ph, (const int32_t*)cluster); put(fRes, ph, (const oslam_objmap_result_t*)results);   // rows no problem owns come back as they were
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, nullptr));
    OSLAM_CHECK(launch_map(fn, h, op, n_problems, at(fProb, pd), n_rows, at(fPos, pd), at(fLc, pd), at(fLs, pd), at(fKeep, pd), at(fClu, pd), at(fRes, pd), labels_needed, nullptr));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fKeep.off, pd + fKeep.off, lay.total() - fKeep.off, hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(fKeep, ph, keep); get(fClu, ph, cluster); get(fRes, ph, results);
    return OSLAM_OK;
}

int launch_merge(const char* fn, oslam_objmap* h, int n_problems, const oslam_objmap_merge_problem_t* d_problems, int n_rows, const int32_t* d_label, const int32_t* d_track,
                 const float* d_bbox, int bbox_stride, int n_pairs, float* d_ratio, uint8_t* d_member, int32_t* d_target, int32_t* d_n_sets, int32_t* d_status, hipStream_t stream) {
    OSLAM_CHECK(check_call(fn, h, n_problems, n_rows));
    if (n_pairs < 0) { set_error("%s: n_pairs is negative", fn); return OSLAM_E_CAPACITY; }
    if (bbox_stride < 6) { set_error("%s: bbox_stride %d is below 6", fn, bbox_stride); return OSLAM_E_INVALID; }
    if (n_problems == 0) return OSLAM_OK;
    if (!d_problems || !d_n_sets || !d_status || (n_rows > 0 && (!d_label || !d_track || !d_bbox || !d_target)) || (n_pairs > 0 && (!d_ratio || !d_member))) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    MergeArgs a;
    a.problems = d_problems; a.label = d_label; a.track = d_track; a.bbox = d_bbox; a.bbox_stride = bbox_stride; a.n_rows = n_rows; a.n_pairs = n_pairs; a.max_obj = h->max_obj;
    a.ratio = d_ratio; a.member = d_member; a.target = d_target; a.n_sets = d_n_sets; a.status = d_status;
    if (h->timing) OSLAM_HIP_CHECK(hipEventRecord(h->ev[0], stream));
    hipLaunchKernelGGL(k_merge_sets, dim3(n_problems), dim3(kMergeThreads), 0, stream, a);
    if (h->timing) OSLAM_HIP_CHECK(hipEventRecord(h->ev[1], stream));
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

}  // namespace

extern "C" {

void oslam_objmap_destroy(oslam_objmap_t* h) {
    if (!h) return;
    delete h;
}

int oslam_objmap_create(oslam_objmap_t** out, int max_problems, int max_cluster_points, int max_objects) {
    if (!out) { set_error("oslam_objmap_create: out is NULL"); return OSLAM_E_INVALID; }
    *out = nullptr;
    if (max_problems < 1 || max_cluster_points < OSLAM_OBJMAP_MIN_CLUSTER_POINTS || max_cluster_points > OSLAM_OBJMAP_MAX_CLUSTER_POINTS || max_objects < 1 || max_objects > kMaxObj) {
        set_error("oslam_objmap_create: bad argument (max_cluster_points is %d .. %d, max_objects 1 .. %d)", OSLAM_OBJMAP_MIN_CLUSTER_POINTS, OSLAM_OBJMAP_MAX_CLUSTER_POINTS, kMaxObj);
        return OSLAM_E_INVALID;
    }
    if (oslam_device_count() <= 0) return oslam::no_device("oslam_objmap_create");
    oslam_objmap* h = new oslam_objmap;
    h->max_problems = max_problems; h->cap = max_cluster_points; h->max_obj = max_objects;
    if (hipGetDevice(&h->device) != hipSuccess) { set_error("oslam_objmap_create: hipGetDevice failed"); delete h; return OSLAM_E_HIP; }
    *out = h;
    return OSLAM_OK;
}

int oslam_objmap_set_timing(oslam_objmap_t* h, int on) {
    if (!h) { set_error("oslam_objmap_set_timing: handle is NULL"); return OSLAM_E_INVALID; }
    if (on)
        for (hipEvent_t& e : h->ev) if (!e) OSLAM_HIP_CHECK(hipEventCreate(&e));
    h->timing = on != 0;
    return OSLAM_OK;
}

int oslam_objmap_last_kernel_ms(oslam_objmap_t* h, float ms[2]) {
    if (!h || !ms || !h->timing) { set_error("oslam_objmap_last_kernel_ms: timing is not on"); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipEventSynchronize(h->ev[1]));
    OSLAM_HIP_CHECK(hipEventElapsedTime(&ms[0], h->ev[0], h->ev[1]));
    ms[1] = 0.0f;
    return OSLAM_OK;
}

int oslam_objmap_reject_outliers_device(oslam_objmap_t* h, int n_problems, const oslam_objmap_problem_t* d_problems, int n_rows, const float* d_pos, const int32_t* d_label_cnt,
                                        const int32_t* d_label_sum, uint8_t* d_keep, int32_t* d_cluster, oslam_objmap_result_t* d_results, void* stream) {
    return launch_map("oslam_objmap_reject_outliers_device", h, kOpReject, n_problems, d_problems, n_rows, d_pos, d_label_cnt, d_label_sum, d_keep, d_cluster, d_results, true,
                      (hipStream_t)stream);
}

int oslam_objmap_reject_outliers(oslam_objmap_t* h, int n_problems, const oslam_objmap_problem_t* problems, int n_rows, const float* pos, const int32_t* label_cnt,
                                 const int32_t* label_sum, uint8_t* keep, int32_t* cluster, oslam_objmap_result_t* results) {
    return run_map_host("oslam_objmap_reject_outliers", h, kOpReject, n_problems, problems, n_rows, pos, label_cnt, label_sum, keep, cluster, results);
}

int oslam_objmap_center_and_size_device(oslam_objmap_t* h, int n_problems, const oslam_objmap_problem_t* d_problems, int n_rows, const float* d_pos,
                                        oslam_objmap_result_t* d_results, void* stream) {
    return launch_map("oslam_objmap_center_and_size_device", h, kOpExtent, n_problems, d_problems, n_rows, d_pos, nullptr, nullptr, nullptr, nullptr, d_results, false, (hipStream_t)stream);
}

int oslam_objmap_center_and_size(oslam_objmap_t* h, int n_problems, const oslam_objmap_problem_t* problems, int n_rows, const float* pos, oslam_objmap_result_t* results) {
    return run_map_host("oslam_objmap_center_and_size", h, kOpExtent, n_problems, problems, n_rows, pos, nullptr, nullptr, nullptr, nullptr, results);
}

int oslam_objmap_merge_sets_device(oslam_objmap_t* h, int n_problems, const oslam_objmap_merge_problem_t* d_problems, int n_rows, const int32_t* d_label,
                                   const int32_t* d_track_id, const float* d_bbox, int bbox_stride, int n_pairs, float* d_ratio, uint8_t* d_member, int32_t* d_target,
                                   int32_t* d_n_sets, int32_t* d_status, void* stream) {
    return launch_merge("oslam_objmap_merge_sets_device", h, n_problems, d_problems, n_rows, d_label, d_track_id, d_bbox, bbox_stride, n_pairs, d_ratio, d_member, d_target, d_n_sets,
                        d_status, (hipStream_t)stream);
}

int oslam_objmap_merge_sets(oslam_objmap_t* h, int n_problems, const oslam_objmap_merge_problem_t* problems, int n_rows, const int32_t* label, const int32_t* track_id,
                            const float* bbox, int bbox_stride, int n_pairs, float* ratio, uint8_t* member, int32_t* target, int32_t* n_sets, int32_t* status) {
    const char* fn = "oslam_objmap_merge_sets";
    OSLAM_CHECK(check_call(fn, h, n_problems, n_rows));
    if (n_pairs < 0) { set_error("%s: n_pairs is negative", fn); return OSLAM_E_CAPACITY; }
    if (bbox_stride < 6) { set_error("%s: bbox_stride %d is below 6", fn, bbox_stride); return OSLAM_E_INVALID; }
    if (n_problems == 0) return OSLAM_OK;
    if (!problems || !n_sets || !status || (n_rows > 0 && (!label || !track_id || !bbox || !target)) || (n_pairs > 0 && (!ratio || !member))) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    for (int b = 0; b < n_problems; b++) {
        if (!merge_valid(problems[b], n_rows, n_pairs)) { set_error("%s: problem %d (rows %d + %d of %d, pairs from %d of %d) is not valid", fn, b, problems[b].off_obj, problems[b].n, n_rows, problems[b].off_pair, n_pairs); return OSLAM_E_INVALID; }
        if (problems[b].n > h->max_obj) { set_error("%s: problem %d has %d objects, above the handle's %d", fn, b, problems[b].n, h->max_obj); return OSLAM_E_CAPACITY; }
    }
    std::lock_guard<std::mutex> lock(h->mu);
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t np = (size_t)n_problems, nr = (size_t)n_rows, nq = (size_t)n_pairs;
    const size_t nbox = nr ? (nr - 1) * (size_t)bbox_stride + 6 : 0;   // the floats from the first row's box to the end of the last one's
    oslam::StageLayout lay;
    const auto fProb = lay.add<oslam_objmap_merge_problem_t>(np);
    const auto fLab = lay.add<int32_t>(nr), fTrk = lay.add<int32_t>(nr);
    const auto fBox = lay.add<float>(nbox);
    const auto fRat = lay.add<float>(nq);   // from here on: read and written
    const auto fMem = lay.add<uint8_t>(nq);
    const auto fTgt = lay.add<int32_t>(nr);
    const auto fNs = lay.add<int32_t>(np), fSt = lay.add<int32_t>(np);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fProb, ph, problems); put(fLab, ph, label); put(fTrk, ph, track_id); put(fBox, ph, bbox);
    put(fRat, ph, (const float*)ratio); put(fMem, ph, (const uint8_t*)member); put(fTgt, ph, (const int32_t*)target); put(fNs, ph, (const int32_t*)n_sets); put(fSt, ph, (const int32_t*)status);
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, nullptr));
    OSLAM_CHECK(launch_merge(fn, h, n_problems, at(fProb, pd), n_rows, at(fLab, pd), at(fTrk, pd), at(fBox, pd), bbox_stride, n_pairs, at(fRat, pd), at(fMem, pd), at(fTgt, pd), at(fNs, pd),
                             at(fSt, pd), nullptr));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fRat.off, pd + fRat.off, lay.total() - fRat.off, hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(fRat, ph, ratio); get(fMem, ph, member); get(fTgt, ph, target); get(fNs, ph, n_sets); get(fSt, ph, status);
    return OSLAM_OK;
}

}  // extern "C"
