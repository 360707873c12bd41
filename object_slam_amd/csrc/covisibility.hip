// covisibility.hip — the covisibility graph of many independent sequences resident on gfx950 (include/oslam_hip.h, "Covisibility graph"): the point-side
// observation lists (MapPoint::mObservations, reference src/MapPoint.cc:201-271), every keyframe's mConnectedKeyFrameWeights as a row of K weights, which
// part of that row is mvpOrderedConnectedKeyFrames, the spanning-tree parent and the bad flags (src/KeyFrame.cc:123-208, :289-398, :553-567), with
// KeyFrame::UpdateConnections, the covisibility queries and Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1496-1604) as kernels over that state.
// Whatever changes a graph runs in ONE workgroup per graph, which takes the graph's records in record order; the queries run one workgroup per record.
// Counting is integer atomicAdd / atomicMax / atomicOr on LDS, lists are placed by ballot and rank: no atomics on global memory, nothing whose result
// depends on the order the hardware runs anything in.  Product code; never includes oracle/.
#include <climits>
#include <mutex>
#include <vector>

#include "common.h"
#include "stage_layout.h"

using oslam::set_error;

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTh = 15;            // th of UpdateConnections (src/KeyFrame.cc:330)
constexpr int kLocalLimit = 80;    // src/Tracking.cc:1550
constexpr int kBest = 10;          // GetBestCovisibilityKeyFrames(10), src/Tracking.cc:1555
constexpr uint32_t kPtCnt = 0xffu, kPtBad = OSLAM_COVIS_PT_BAD << 8, kPtOvf = OSLAM_COVIS_PT_OVERFLOW << 8;
constexpr uint32_t kKfAll = OSLAM_COVIS_KF_ORDERED_ALL, kKfConnected = OSLAM_COVIS_KF_CONNECTED, kKfBad = OSLAM_COVIS_KF_IS_BAD;
static_assert(OSLAM_COVIS_MAX_OBS == 64, "an observation list is at most one entry per lane");
static_assert(OSLAM_COVIS_MAX_KEYFRAMES <= 2048, "three rows of K ints and two bitsets in LDS");

// the resident state as the kernels see it; graph g owns slice g of every array
struct CovisState {
    int2* obs;          // [G][P][C] (keyframe id, keypoint index), ascending keyframe id
    uint32_t* pmeta;    // [G][P] count | bad << 8 | overflow << 9
    int32_t* weights;   // [G][K][K] row k = mConnectedKeyFrameWeights of k, 0 = absent
    uint32_t* kmeta;    // [G][K] OSLAM_COVIS_KF_*
    int32_t* parent;    // [G][K] mpParent, -1 = none
    int n_graphs, K, P, C, W;
};

size_t lds_bytes(int K, int W) { return ((size_t)3 * K + 2 * W) * 4; }

}  // namespace

struct oslam_covis {
    int device = 0;
    size_t lds = 0;
    CovisState st{};
    oslam::DeviceBuffer obs, pmeta, weights, kmeta, parent, unsorted;
    hipStream_t stream = nullptr;
    oslam::StagePair io;
    std::mutex mu;
    ~oslam_covis() { if (stream) (void)hipStreamDestroy(stream); }
};

namespace {

// ---- what the workgroup kernels share -------------------------------------------------------------------------------------------------------------
struct Shared {
    int wcnt[kWaves];
    int nnz, nq, tmp;
    unsigned long long lo, hi, key;
};

// Ordered compaction of one value per thread: the position of a thread that hits, in thread order after `base`; *total = the hits.  All threads call it.
__device__ int compact(bool hit, int base, Shared& s, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s.wcnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < kWaves; w++) { const int c = s.wcnt[w]; before += w < wave ? c : 0; all += c; }
    __syncthreads();   // (wcnt is free again)
    *total = all;
    return base + before + __popcll(m & ((1ull << lane) - 1ull));
}

// Of a row of weights (global or LDS): the entries, the entries >= th, and the maximum as the reference takes it in two places: s.lo names the LOWEST id of
// the maximum weight (pKFmax of the strict '>' walked in ascending id, src/KeyFrame.cc:336), s.hi the HIGHEST (the front of the list sorted by (weight, id)
// and reversed, :354-361).  Integer maxima and sums: any order.  All threads call it; the results are in s after it returns.
__device__ void row_stats(const int32_t* row, int K, Shared& s) {
    if (threadIdx.x == 0) { s.nnz = 0; s.nq = 0; s.lo = 0; s.hi = 0; }
    __syncthreads();
    int nnz = 0, nq = 0;
    unsigned long long lo = 0, hi = 0;
    for (int o = threadIdx.x; o < K; o += kThreads) {
        const int w = row[o];
        if (w > 0) {
            nnz++; nq += w >= kTh ? 1 : 0;
            const unsigned long long klo = ((unsigned long long)w << 32) | (0xffffffffu - (uint32_t)o), khi = ((unsigned long long)w << 32) | (uint32_t)o;
            lo = klo > lo ? klo : lo; hi = khi > hi ? khi : hi;
        }
    }
    if (nnz) { atomicAdd(&s.nnz, nnz); atomicAdd(&s.nq, nq); atomicMax(&s.lo, lo); atomicMax(&s.hi, hi); }
    __syncthreads();
}
__device__ inline int lo_id(const Shared& s) { return (int)(0xffffffffu - (uint32_t)s.lo); }
__device__ inline int hi_id(const Shared& s) { return (int)(uint32_t)s.hi; }

// Is entry (w, o) of a row in mvpOrderedConnectedKeyFrames?  Every entry once an UpdateBestCovisibles has run (all); after the keyframe's own
// UpdateConnections the entries >= th, or the single pKFmax when none is (src/KeyFrame.cc:341-352).
__device__ inline bool in_ordered(int w, int o, bool all, int nq, int lo) { return w > 0 && (all || w >= kTh || (nq == 0 && o == lo)); }

// mvpOrderedConnectedKeyFrames / mvOrderedWeights of a row, cut as GetBestCovisibilityKeyFrames(max_n) and GetCovisiblesByWeight(min_w) cut it: members in
// descending (weight, id), each placed by its rank among the members.  s_q, s_qw: K ints of LDS each.  Returns the entries written (uniform).
__device__ int emit_ordered(const int32_t* row, bool all, int K, int max_n, int min_w, int32_t* out_ids, int32_t* out_w, int* s_q, int* s_qw, Shared& s) {
    row_stats(row, K, s);
    const int nq = s.nq, lo = lo_id(s);
    int m = 0;
    for (int o0 = 0; o0 < K; o0 += kThreads) {
        const int o = o0 + threadIdx.x, w = o < K ? row[o] : 0;
        const bool hit = o < K && in_ordered(w, o, all, nq, lo);
        int n;
        const int pos = compact(hit, m, s, &n);
        if (hit) { s_q[pos] = o; s_qw[pos] = w; }
        m += n;
    }
    if (threadIdx.x == 0) s.tmp = 0;
    __syncthreads();
    int limit = m;
    if (min_w > 0) {   // upper_bound(w, weightComp) (src/KeyFrame.cc:191-198): the entries >= w — and none at all when that is every entry
        int c = 0;
        for (int i = threadIdx.x; i < m; i += kThreads) c += s_qw[i] >= min_w ? 1 : 0;
        if (c) atomicAdd(&s.tmp, c);
        __syncthreads();
        limit = s.tmp == m ? 0 : s.tmp;
    }
    limit = limit < max_n ? limit : (max_n > 0 ? max_n : 0);
    for (int i = threadIdx.x; i < m; i += kThreads) {
        const int w = s_qw[i], o = s_q[i];
        int r = 0;
        for (int j = 0; j < m; j++) { const int wj = s_qw[j]; r += (wj > w || (wj == w && s_q[j] > o)) ? 1 : 0; }
        if (r < limit) { out_ids[r] = o; out_w[r] = w; }
    }
    __syncthreads();
    return limit;
}

// ---- events ---------------------------------------------------------------------------------------------------------------------------------------
// *unsorted becomes 1 when the records' graphs do not ascend (every writer writes the same value)
__global__ __launch_bounds__(kThreads) void k_covis_sorted(const oslam_covis_event_t* ev, int n, int32_t* unsorted) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i + 1 < n && ev[i].graph > ev[i + 1].graph) *unsorted = 1;
}

// One wavefront per graph: finds the graph's events (a binary search when the records ascend by graph, otherwise a pass over all of them: the same events
// in the same order either way) and applies them one after the other, the list of a point one entry per lane.
__global__ __launch_bounds__(64) void k_covis_apply(CovisState st, const oslam_covis_event_t* ev, int n, const int32_t* unsorted, int32_t* n_overflow) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int K = st.K, P = st.P, C = st.C;
    int lo = 0, hi = n;
    if (*unsorted == 0) {
        int a = 0, b = n;
        while (a < b) { const int mid = (a + b) >> 1; if (ev[mid].graph < g) a = mid + 1; else b = mid; }
        lo = a; b = n;
        while (a < b) { const int mid = (a + b) >> 1; if (ev[mid].graph <= g) a = mid + 1; else b = mid; }
        hi = a;
    }
    int2* obs = st.obs + (size_t)g * P * C;
    uint32_t* pmeta = st.pmeta + (size_t)g * P;
    int32_t* weights = st.weights + (size_t)g * K * K;
    uint32_t* kmeta = st.kmeta + (size_t)g * K;
    int32_t* parent = st.parent + (size_t)g * K;
    int novf = 0;
    for (int c0 = lo; c0 < hi; c0 += 64) {
        const int i = c0 + lane;
        unsigned long long todo = __ballot(i < hi && ev[i].graph == g);
        while (todo) {   // (uniform)
            const int j = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const oslam_covis_event_t e = ev[c0 + j];
            const int a = e.a, b = e.b;
            if (e.type == OSLAM_COVIS_EV_OBS_ADD || e.type == OSLAM_COVIS_EV_OBS_ERASE) {
                if (a >= 0 && a < P && b >= 0 && b < K) {
                    int2* ob = obs + (size_t)a * C;
                    const uint32_t meta = pmeta[a];
                    const int cnt = (int)(meta & kPtCnt);
                    const int2 mine = lane < cnt ? ob[lane] : make_int2(INT_MAX, 0);
                    const unsigned long long same = __ballot(mine.x == b);
                    if (e.type == OSLAM_COVIS_EV_OBS_ADD) {   // MapPoint::AddObservation (src/MapPoint.cc:201-212)
                        if (same) {
                        } else if (cnt >= C) {
                            if (lane == 0) pmeta[a] = meta | kPtOvf;
                            novf++;
                        } else {
                            const int pos = __popcll(__ballot(mine.x < b));
                            if (lane >= pos && lane < cnt) ob[lane + 1] = mine;
                            if (lane == 0) { ob[pos] = make_int2(b, e.c); pmeta[a] = meta + 1; }
                        }
                    } else if (same) {                     // MapPoint::EraseObservation (:214-240) without its SetBadFlag
                        const int pos = __ffsll((long long)same) - 1;
                        if (lane > pos && lane < cnt) ob[lane - 1] = mine;
                        if (lane == 0) pmeta[a] = meta - 1;
                    }
                }
            } else if (e.type == OSLAM_COVIS_EV_POINT_BAD) {   // MapPoint::SetBadFlag (:254-263)
                if (a >= 0 && a < P && lane == 0) pmeta[a] = kPtBad;
            } else if (e.type == OSLAM_COVIS_EV_CONN_ADD) {   // KeyFrame::AddConnection (src/KeyFrame.cc:123-136)
                if (a >= 0 && a < K && b >= 0 && b < K && e.c > 0 && lane == 0) {
                    int32_t* w = weights + (size_t)a * K + b;
                    if (*w != e.c) { *w = e.c; kmeta[a] |= kKfAll; }
                }
            } else if (e.type == OSLAM_COVIS_EV_CONN_ERASE) {   // KeyFrame::EraseConnection (:553-567)
                if (a >= 0 && a < K && b >= 0 && b < K && lane == 0) {
                    int32_t* w = weights + (size_t)a * K + b;
                    if (*w != 0) { *w = 0; kmeta[a] |= kKfAll; }
                }
            } else if (e.type == OSLAM_COVIS_EV_KF_BAD) {
                if (a >= 0 && a < K && lane == 0) kmeta[a] |= kKfBad;
            } else if (e.type == OSLAM_COVIS_EV_PARENT_SET) {   // KeyFrame::ChangeParent (:393-398)
                if (a >= 0 && a < K && b >= 0 && b < K && lane == 0) parent[a] = b;
            }
            __syncthreads();   // the next event of this graph sees this one's stores
        }
    }
    if (lane == 0) n_overflow[g] = novf;
}

// ---- the observers of a list of points, counted into LDS ------------------------------------------------------------------------------------------
// s_cnt[kf] += 1 per observation of every point of pts[0 .. n) that is not bad (duplicates count once per occurrence), leaving out keyframe `self`
// (-1: nobody).  null_out, if given: 1 where the point is bad.  Returns nothing; *s_ovf becomes 1 when a point with the overflow bit was read.
__device__ void count_observers(const CovisState& st, int g, const int32_t* pts, int n, int self, int* s_cnt, int* s_ovf, uint8_t* null_out) {
    const int2* obs = st.obs + (size_t)g * st.P * st.C;
    const uint32_t* pmeta = st.pmeta + (size_t)g * st.P;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const int p = pts[i];
        bool bad = false;
        if (p >= 0 && p < st.P) {
            const uint32_t meta = pmeta[p];
            bad = (meta & kPtBad) != 0u;
            if (!bad) {
                if (meta & kPtOvf) *s_ovf = 1;
                const int cnt = (int)(meta & kPtCnt);
                const int2* ob = obs + (size_t)p * st.C;
                for (int j = 0; j < cnt && j < st.C; j++) {
                    const int kf = ob[j].x;
                    if (kf != self && kf >= 0 && kf < st.K) atomicAdd(&s_cnt[kf], 1);
                }
            }
        }
        if (null_out) null_out[i] = bad ? 1 : 0;
    }
}

__device__ inline bool bit(const uint32_t* bits, int i) { return (bits[i >> 5] >> (i & 31)) & 1u; }

// ---- KeyFrame::UpdateConnections ------------------------------------------------------------------------------------------------------------------
struct UpdateArgs {
    CovisState st;
    const oslam_covis_update_t* recs;
    int n, n_points, n_excl;
    const int32_t* points; const int32_t* excl;
    int32_t *status, *ord_ids, *ord_w, *n_ord, *parent, *links, *n_links;
};

// One workgroup per graph; it takes the records that name its graph in record order, each start to end: the histogram of the observers in LDS, the
// AddConnections into the other rows, the keyframe's own row, then the outputs read back from the state.
__global__ __launch_bounds__(kThreads) void k_covis_update(UpdateArgs a) {
    const int g = blockIdx.x, tid = threadIdx.x;
    const CovisState& st = a.st;
    const int K = st.K, W = st.W;
    extern __shared__ __align__(16) uint8_t smem[];
    int* s_cnt = (int*)smem;                         // [K] KFcounter
    int* s_q = s_cnt + K;                            // [K], [K] the members of an ordered list
    int* s_qw = s_q + K;
    uint32_t* s_before = (uint32_t*)(s_qw + K);      // [W] the ordered list before the update
    uint32_t* s_excl = s_before + W;                 // [W] the record's exclude ids
    __shared__ Shared s;
    __shared__ int s_list[kThreads];
    __shared__ int s_ovf;

    int32_t* weights = st.weights + (size_t)g * K * K;
    uint32_t* kmeta = st.kmeta + (size_t)g * K;
    int32_t* parent = st.parent + (size_t)g * K;

    for (int r0 = 0; r0 < a.n; r0 += kThreads) {
        int nm;
        {
            const int r = r0 + tid;
            const int rg = r < a.n ? a.recs[r].graph : 0;
            const bool hit = r < a.n && (rg == g || (g == 0 && (rg < 0 || rg >= st.n_graphs)));   // (graph 0's workgroup answers the records that name no graph)
            const int pos = compact(hit, 0, s, &nm);
            if (hit) s_list[pos] = r;
            __syncthreads();
        }
        for (int x = 0; x < nm; x++) {   // (uniform)
            const int r = s_list[x];
            const oslam_covis_update_t rec = a.recs[r];
            const int k = rec.keyframe;
            const bool ok = rec.graph == g && k >= 0 && k < K && rec.n_pts >= 0 && rec.pts_off >= 0 && rec.pts_off <= a.n_points - rec.n_pts && rec.n_excl >= 0 && rec.excl_off >= 0 &&
                            rec.excl_off <= a.n_excl - rec.n_excl;
            if (!ok) {   // (what the host entry point refuses as a whole)
                if (tid == 0) { a.status[r] = -2; a.n_ord[r] = 0; a.n_links[r] = 0; a.parent[r] = -1; }
                continue;
            }
            int32_t* row = weights + (size_t)k * K;
            for (int o = tid; o < K; o += kThreads) s_cnt[o] = 0;
            for (int o = tid; o < 2 * W; o += kThreads) s_before[o] = 0u;   // (s_excl follows s_before)
            if (tid == 0) s_ovf = 0;
            __syncthreads();
            count_observers(st, g, a.points + rec.pts_off, rec.n_pts, k, s_cnt, &s_ovf, nullptr);
            for (int i = tid; i < rec.n_excl; i += kThreads) {
                const int id = a.excl[rec.excl_off + i];
                if (id >= 0 && id < K) atomicOr(&s_excl[id >> 5], 1u << (id & 31));
            }
            __syncthreads();
            if (s_ovf) {   // (uniform) a list that lost observations: the graph stays as it is
                if (tid == 0) { a.status[r] = -3; a.n_ord[r] = 0; a.n_links[r] = 0; a.parent[r] = parent[k]; }
                __syncthreads();
                continue;
            }
            // vpPreviousNeighbors (src/LoopClosing.cc:552)
            const uint32_t meta = kmeta[k];
            row_stats(row, K, s);
            {
                const int nq = s.nq, lo = lo_id(s);
                for (int o = tid; o < K; o += kThreads)
                    if (in_ordered(row[o], o, (meta & kKfAll) != 0u, nq, lo)) atomicOr(&s_before[o >> 5], 1u << (o & 31));
            }
            __syncthreads();
            row_stats(s_cnt, K, s);
            const bool empty = s.nnz == 0;   // "This should not happen" (src/KeyFrame.cc:323): nothing changes
            if (!empty) {
                const int nq = s.nq, lo = lo_id(s), front = nq > 0 ? hi_id(s) : lo;
                for (int o = tid; o < K; o += kThreads) {
                    const int c = s_cnt[o];
                    if (c > 0 && (c >= kTh || (nq == 0 && o == lo))) {   // (mit->first)->AddConnection(this, mit->second) (:344, :351); o != k
                        int32_t* w = weights + (size_t)o * K + k;
                        if (*w != c) { *w = c; kmeta[o] |= kKfAll; }
                    }
                    row[o] = c;   // mConnectedKeyFrameWeights = KFcounter (:367)
                }
                if (tid == 0) {
                    uint32_t m2 = meta & ~kKfAll;
                    if (!(meta & kKfConnected) && k != 0) { parent[k] = front; m2 |= kKfConnected; }   // mbFirstConnection && mnId != 0 (:371-376)
                    kmeta[k] = m2;
                }
            }
            __syncthreads();   // the state is as the record leaves it
            const int n_ord = emit_ordered(row, (kmeta[k] & kKfAll) != 0u, K, K, 0, a.ord_ids + (size_t)r * K, a.ord_w + (size_t)r * K, s_q, s_qw, s);
            // LoopConnections[pKFi] (src/LoopClosing.cc:556-564): the keys of the row, minus the previous neighbours, minus the exclude ids
            int n_links = 0;
            for (int o0 = 0; o0 < K; o0 += kThreads) {
                const int o = o0 + tid;
                const bool hit = o < K && row[o] > 0 && !bit(s_before, o) && !bit(s_excl, o);
                int n;
                const int pos = compact(hit, n_links, s, &n);
                if (hit) a.links[(size_t)r * K + pos] = o;
                n_links += n;
            }
            if (tid == 0) { a.status[r] = empty ? 1 : 0; a.n_ord[r] = n_ord; a.n_links[r] = n_links; a.parent[r] = parent[k]; }
            __syncthreads();
        }
        __syncthreads();
    }
}

// ---- queries: one workgroup per record ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_covis_covisibles(CovisState st, const oslam_covis_query_t* recs, int32_t* ids, int32_t* w, int32_t* n_out) {
    const int r = blockIdx.x, K = st.K;
    extern __shared__ __align__(16) uint8_t smem[];
    int* s_q = (int*)smem;
    int* s_qw = s_q + K;
    __shared__ Shared s;
    const oslam_covis_query_t q = recs[r];
    if (q.graph < 0 || q.graph >= st.n_graphs || q.keyframe < 0 || q.keyframe >= K) {   // (uniform)
        if (threadIdx.x == 0) n_out[r] = -2;
        return;
    }
    const int32_t* row = st.weights + ((size_t)q.graph * K + q.keyframe) * K;
    const bool all = (st.kmeta[(size_t)q.graph * K + q.keyframe] & kKfAll) != 0u;
    const int n = emit_ordered(row, all, K, q.max_n, q.min_w, ids + (size_t)r * K, w + (size_t)r * K, s_q, s_qw, s);
    if (threadIdx.x == 0) n_out[r] = n;
}

__global__ __launch_bounds__(kThreads) void k_covis_connected_rows(CovisState st, const oslam_covis_key_t* recs, uint32_t* bits) {
    const int r = blockIdx.x, K = st.K, W = st.W;
    __shared__ uint32_t s_bits[OSLAM_COVIS_MAX_KEYFRAMES / 32];
    const oslam_covis_key_t q = recs[r];
    if (q.graph < 0 || q.graph >= st.n_graphs || q.keyframe < 0 || q.keyframe >= K) return;   // (uniform)
    for (int i = threadIdx.x; i < W; i += kThreads) s_bits[i] = 0u;
    __syncthreads();
    const int32_t* row = st.weights + ((size_t)q.graph * K + q.keyframe) * K;
    for (int o = threadIdx.x; o < K; o += kThreads)
        if (row[o] > 0) atomicOr(&s_bits[o >> 5], 1u << (o & 31));
    __syncthreads();
    for (int i = threadIdx.x; i < W; i += kThreads) bits[(size_t)r * W + i] = s_bits[i];
}

struct LocalArgs {
    CovisState st;
    const oslam_covis_local_t* recs;
    int n_points;
    const int32_t* points;
    int32_t *list, *n_list, *ref_kf;
    uint8_t* null_out;
};

// Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1496-1604) for one frame.  The vote and the voters are parallel; the neighbour loop is the reference's,
// one voter after the other, each of its three searches a pass of the whole workgroup.
__global__ __launch_bounds__(kThreads) void k_covis_local(LocalArgs a) {
    const int r = blockIdx.x, tid = threadIdx.x;
    const CovisState& st = a.st;
    const int K = st.K, W = st.W;
    extern __shared__ __align__(16) uint8_t smem[];
    int* s_cnt = (int*)smem;                     // [K] keyframeCounter
    int* s_voters = s_cnt + K;                   // [K] the voters, ascending id
    int* s_row = s_voters + K;                   // [K] the ordered list of the voter at hand, as weights by id
    uint32_t* s_inc = (uint32_t*)(s_row + K);    // [W] mnTrackReferenceForFrame == mCurrentFrame.mnId
    __shared__ Shared s;
    __shared__ int s_ovf, s_min;

    const oslam_covis_local_t rec = a.recs[r];
    const int g = rec.graph;
    if (g < 0 || g >= st.n_graphs || rec.n_pts < 0 || rec.pts_off < 0 || rec.pts_off > a.n_points - rec.n_pts) {   // (uniform)
        if (tid == 0) a.n_list[r] = -2;
        return;
    }
    const int32_t* weights = st.weights + (size_t)g * K * K;
    const uint32_t* kmeta = st.kmeta + (size_t)g * K;
    const int32_t* parent = st.parent + (size_t)g * K;
    int32_t* list = a.list + (size_t)r * K;

    for (int o = tid; o < K; o += kThreads) s_cnt[o] = 0;
    for (int o = tid; o < W; o += kThreads) s_inc[o] = 0u;
    if (tid == 0) { s_ovf = 0; s.nnz = 0; s.lo = 0; }
    __syncthreads();
    count_observers(st, g, a.points + rec.pts_off, rec.n_pts, -1, s_cnt, &s_ovf, a.null_out + rec.pts_off);
    __syncthreads();
    if (s_ovf) {   // (uniform)
        if (tid == 0) a.n_list[r] = -3;
        return;
    }
    // the voters that are not bad in ascending id (:1528-1543), pKFmax by the strict '>'
    int nv = 0;
    for (int o0 = 0; o0 < K; o0 += kThreads) {
        const int o = o0 + tid, c = o < K ? s_cnt[o] : 0;
        const bool hit = c > 0 && !(kmeta[o] & kKfBad);
        if (c > 0) atomicAdd(&s.nnz, 1);
        if (hit) atomicMax(&s.lo, ((unsigned long long)c << 32) | (0xffffffffu - (uint32_t)o));
        int n;
        const int pos = compact(hit, nv, s, &n);
        if (hit) { s_voters[pos] = o; list[pos] = o; atomicOr(&s_inc[o >> 5], 1u << (o & 31)); }
        nv += n;
    }
    __syncthreads();
    if (s.nnz == 0) {   // keyframeCounter.empty() (:1518): nothing else is written
        if (tid == 0) a.n_list[r] = -1;
        return;
    }
    const int ref = nv > 0 ? lo_id(s) : -1;
    __syncthreads();   // (s is reused below)
    int nl = nv;
    for (int i = 0; i < nv; i++) {   // (uniform throughout: nl, the found ids and the breaks are the same in every thread)
        if (nl > kLocalLimit) break;
        const int v = s_voters[i];
        // the first of GetBestCovisibilityKeyFrames(10) that is neither bad nor included (:1555-1569): the ordered list from its front, one maximum per round
        const int32_t* row = weights + (size_t)v * K;
        row_stats(row, K, s);
        {
            const bool all = (kmeta[v] & kKfAll) != 0u;
            const int nq = s.nq, lo = lo_id(s);
            for (int o = tid; o < K; o += kThreads) { const int w = row[o]; s_row[o] = in_ordered(w, o, all, nq, lo) ? w : 0; }
        }
        unsigned long long prev = ~0ull;
        for (int round = 0; round < kBest; round++) {
            if (tid == 0) s.key = 0;
            __syncthreads();
            unsigned long long best = 0;
            for (int o = tid; o < K; o += kThreads) {
                const int w = s_row[o];
                const unsigned long long key = ((unsigned long long)w << 32) | (uint32_t)o;
                if (w > 0 && key < prev && key > best) best = key;
            }
            if (best) atomicMax(&s.key, best);
            __syncthreads();
            prev = s.key;
            if (prev == 0) break;   // the list has ended
            const int id = (int)(uint32_t)prev;
            if (!(kmeta[id] & kKfBad) && !bit(s_inc, id)) {
                __syncthreads();
                if (tid == 0) { list[nl] = id; s_inc[id >> 5] |= 1u << (id & 31); }
                nl++;
                break;
            }
            __syncthreads();
        }
        // the first child in ascending id that is neither bad nor included (:1571-1584)
        if (tid == 0) s_min = INT_MAX;
        __syncthreads();
        for (int o = tid; o < K; o += kThreads)
            if (parent[o] == v && !(kmeta[o] & kKfBad) && !bit(s_inc, o)) atomicMin(&s_min, o);
        __syncthreads();
        const int child = s_min;
        if (child != INT_MAX) {
            if (tid == 0) { list[nl] = child; s_inc[child >> 5] |= 1u << (child & 31); }
            nl++;
        }
        __syncthreads();
        // the parent, and with it the end of the OUTER loop (:1586-1595)
        const int p = parent[v];
        if (p >= 0 && p < K && !bit(s_inc, p)) {
            if (tid == 0) list[nl] = p;
            nl++;
            break;
        }
    }
    if (tid == 0) { a.n_list[r] = nl; a.ref_kf[r] = ref; }
}

// ---- launches -------------------------------------------------------------------------------------------------------------------------------------
int launch_apply(oslam_covis* h, int n, const oslam_covis_event_t* d_ev, int32_t* d_n_overflow, hipStream_t stream) {
    OSLAM_HIP_CHECK(hipMemsetAsync(h->unsorted.ptr(), 0, 4, stream));
    if (n > 1) hipLaunchKernelGGL(k_covis_sorted, dim3(oslam::div_up(n, kThreads)), dim3(kThreads), 0, stream, d_ev, n, h->unsorted.as<int32_t>());
    hipLaunchKernelGGL(k_covis_apply, dim3(h->st.n_graphs), dim3(64), 0, stream, h->st, d_ev, n, h->unsorted.as<int32_t>(), d_n_overflow);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int launch_update(oslam_covis* h, const UpdateArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(k_covis_update, dim3(h->st.n_graphs), dim3(kThreads), h->lds, stream, a);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int launch_local(oslam_covis* h, int n, const LocalArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(k_covis_local, dim3(n), dim3(kThreads), h->lds, stream, a);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int check_counts(const char* fn, const oslam_covis* h, int n, int n2 = 0, int n3 = 0) {
    if (!h) { set_error("%s: NULL handle", fn); return OSLAM_E_INVALID; }
    if (n < 0 || n2 < 0 || n3 < 0) { set_error("%s: a count is negative", fn); return OSLAM_E_INVALID; }
    return OSLAM_OK;
}

bool span_ok(int off, int n, int total) { return n >= 0 && off >= 0 && off <= total - n; }

}  // namespace

extern "C" {

void oslam_covis_destroy(oslam_covis_t* h) {
    if (!h) return;
    delete h;
}

static int covis_clear(oslam_covis* h, size_t g0, size_t ng) {
    const size_t K = (size_t)h->st.K, P = (size_t)h->st.P, C = (size_t)h->st.C;
    OSLAM_HIP_CHECK(hipMemsetAsync(h->obs.bytes() + g0 * P * C * 8, 0, ng * P * C * 8, h->stream));
    OSLAM_HIP_CHECK(hipMemsetAsync(h->pmeta.bytes() + g0 * P * 4, 0, ng * P * 4, h->stream));
    OSLAM_HIP_CHECK(hipMemsetAsync(h->weights.bytes() + g0 * K * K * 4, 0, ng * K * K * 4, h->stream));
    OSLAM_HIP_CHECK(hipMemsetAsync(h->kmeta.bytes() + g0 * K * 4, 0, ng * K * 4, h->stream));
    OSLAM_HIP_CHECK(hipMemsetAsync(h->parent.bytes() + g0 * K * 4, 0xff, ng * K * 4, h->stream));   // -1: no parent
    return OSLAM_OK;
}

int oslam_covis_create(oslam_covis_t** out, int n_graphs, int max_keyframes, int max_points, int obs_cap, int device) {
    const char* fn = "oslam_covis_create";
    if (!out) { set_error("%s: out is NULL", fn); return OSLAM_E_INVALID; }
    *out = nullptr;
    if (n_graphs < 1 || max_keyframes < 1 || max_keyframes > OSLAM_COVIS_MAX_KEYFRAMES || max_points < 1 || obs_cap < 1 || obs_cap > OSLAM_COVIS_MAX_OBS) {
        set_error("%s: n_graphs %d, max_keyframes %d (1 .. %d), max_points %d or obs_cap %d (1 .. %d) out of range", fn, n_graphs, max_keyframes, OSLAM_COVIS_MAX_KEYFRAMES,
                  max_points, obs_cap, OSLAM_COVIS_MAX_OBS);
        return OSLAM_E_INVALID;
    }
    const size_t G = (size_t)n_graphs, K = (size_t)max_keyframes, P = (size_t)max_points, C = (size_t)obs_cap;
    if (G * K * K > (1ull << 34) || G * P * C > (1ull << 34)) { set_error("%s: %zu graphs of this size are more than the handle holds", fn, G); return OSLAM_E_INVALID; }
    const int ndev = oslam_device_count();
    if (ndev <= 0) return oslam::no_device(fn);
    if (device < 0 || device >= ndev) { set_error("%s: device out of range", fn); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(device));
    oslam_covis* h = new oslam_covis;
    h->device = device;
    const int W = oslam::div_up(max_keyframes, 32);
    h->lds = lds_bytes(max_keyframes, W);
    int rc = OSLAM_OK;
    if ((rc = h->obs.alloc(G * P * C * 8)) || (rc = h->pmeta.alloc(G * P * 4)) || (rc = h->weights.alloc(G * K * K * 4)) || (rc = h->kmeta.alloc(G * K * 4)) ||
        (rc = h->parent.alloc(G * K * 4)) || (rc = h->unsorted.alloc(4))) {
        delete h;
        return rc;
    }
    h->st = CovisState{h->obs.as<int2>(), h->pmeta.as<uint32_t>(), h->weights.as<int32_t>(), h->kmeta.as<uint32_t>(), h->parent.as<int32_t>(), n_graphs, max_keyframes,
                       max_points, obs_cap, W};
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) {
        rc = covis_clear(h, 0, G);
        if (rc == OSLAM_OK) e = hipStreamSynchronize(h->stream);
    }
    if (e != hipSuccess || rc != OSLAM_OK) {
        if (e != hipSuccess) set_error("%s: %s", fn, hipGetErrorString(e));
        delete h;
        return rc ? rc : OSLAM_E_HIP;
    }
    *out = h;
    return OSLAM_OK;
}

int oslam_covis_reset(oslam_covis_t* h, int n, const int32_t* graphs) {
    const char* fn = "oslam_covis_reset";
    if (!h || n < 0 || (n > 0 && !graphs)) { set_error("%s: bad argument", fn); return OSLAM_E_INVALID; }
    if (n == 0) return OSLAM_OK;
    std::lock_guard<std::mutex> lock(h->mu);
    for (int r = 0; r < n; r++)
        if (graphs[r] < 0 || graphs[r] >= h->st.n_graphs) { set_error("%s: record %d names graph %d of %d", fn, r, graphs[r], h->st.n_graphs); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    for (int r = 0; r < n; r++) OSLAM_CHECK(covis_clear(h, (size_t)graphs[r], 1));
    OSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    return OSLAM_OK;
}

int oslam_covis_apply(oslam_covis_t* h, int n_events, const oslam_covis_event_t* events, int32_t* n_overflow_out) {
    const char* fn = "oslam_covis_apply";
    OSLAM_CHECK(check_counts(fn, h, n_events));
    if (!n_overflow_out || (n_events > 0 && !events)) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    std::lock_guard<std::mutex> lock(h->mu);
    const int K = h->st.K, P = h->st.P, G = h->st.n_graphs;
    for (int i = 0; i < n_events; i++) {
        const oslam_covis_event_t& e = events[i];
        const bool kf_a = e.a >= 0 && e.a < K, kf_b = e.b >= 0 && e.b < K, pt_a = e.a >= 0 && e.a < P;
        bool ok = e.graph >= 0 && e.graph < G;
        switch (e.type) {
            case OSLAM_COVIS_EV_OBS_ADD: case OSLAM_COVIS_EV_OBS_ERASE: ok = ok && pt_a && kf_b; break;
            case OSLAM_COVIS_EV_POINT_BAD: ok = ok && pt_a; break;
            case OSLAM_COVIS_EV_CONN_ADD: ok = ok && kf_a && kf_b && e.c > 0; break;
            case OSLAM_COVIS_EV_CONN_ERASE: case OSLAM_COVIS_EV_PARENT_SET: ok = ok && kf_a && kf_b; break;
            case OSLAM_COVIS_EV_KF_BAD: ok = ok && kf_a; break;
            default: ok = false;
        }
        if (!ok) { set_error("%s: event %d {graph %d, type %d, %d, %d, %d} names an id outside the handle or has an unknown type", fn, i, e.graph, e.type, e.a, e.b, e.c); return OSLAM_E_INVALID; }
    }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    oslam::StageLayout lay;
    const auto fEv = lay.add<oslam_covis_event_t>((size_t)n_events);
    const auto fOv = lay.add<int32_t>((size_t)G);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fEv, ph, events);
    if (fEv.bytes) OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, fEv.end(), hipMemcpyHostToDevice, h->stream));
    OSLAM_CHECK(launch_apply(h, n_events, at(fEv, pd), at(fOv, pd), h->stream));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fOv.off, pd + fOv.off, fOv.bytes, hipMemcpyDeviceToHost, h->stream));
    OSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    get(fOv, ph, n_overflow_out);
    return OSLAM_OK;
}

int oslam_covis_apply_device(oslam_covis_t* h, int n_events, const oslam_covis_event_t* d_events, int32_t* d_n_overflow_out, void* stream) {
    const char* fn = "oslam_covis_apply_device";
    OSLAM_CHECK(check_counts(fn, h, n_events));
    if (!d_n_overflow_out || (n_events > 0 && !d_events)) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    return launch_apply(h, n_events, d_events, d_n_overflow_out, (hipStream_t)stream);
}

int oslam_covis_update_connections(oslam_covis_t* h, int n, const oslam_covis_update_t* recs, int n_points_total, const int32_t* points, int n_excl_total,
                                   const int32_t* exclude, int32_t* status, int32_t* ordered_ids, int32_t* ordered_w, int32_t* n_ordered, int32_t* parent,
                                   int32_t* new_links, int32_t* n_new_links) {
    const char* fn = "oslam_covis_update_connections";
    OSLAM_CHECK(check_counts(fn, h, n, n_points_total, n_excl_total));
    if (n == 0) return OSLAM_OK;
    if (!recs || !status || !ordered_ids || !ordered_w || !n_ordered || !parent || !new_links || !n_new_links || (n_points_total > 0 && !points) ||
        (n_excl_total > 0 && !exclude)) {
        set_error("%s: NULL argument", fn);
        return OSLAM_E_INVALID;
    }
    std::lock_guard<std::mutex> lock(h->mu);
    const int K = h->st.K, P = h->st.P;
    for (int r = 0; r < n; r++) {
        const oslam_covis_update_t& R = recs[r];
        if (R.graph < 0 || R.graph >= h->st.n_graphs || R.keyframe < 0 || R.keyframe >= K) { set_error("%s: record %d names graph %d, keyframe %d", fn, r, R.graph, R.keyframe); return OSLAM_E_INVALID; }
        if (!span_ok(R.pts_off, R.n_pts, n_points_total) || !span_ok(R.excl_off, R.n_excl, n_excl_total)) { set_error("%s: record %d lies outside the arrays", fn, r); return OSLAM_E_INVALID; }
        for (int i = 0; i < R.n_pts; i++)
            if (points[R.pts_off + i] >= P) { set_error("%s: record %d's point %d is id %d of %d", fn, r, i, points[R.pts_off + i], P); return OSLAM_E_INVALID; }
        for (int i = 0; i < R.n_excl; i++)
            if (exclude[R.excl_off + i] < 0 || exclude[R.excl_off + i] >= K) { set_error("%s: record %d's exclude id %d is keyframe %d of %d", fn, r, i, exclude[R.excl_off + i], K); return OSLAM_E_INVALID; }
    }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t N = (size_t)n;
    oslam::StageLayout lay;   // one block, inputs then outputs: one upload, one launch, one download
    const auto fRec = lay.add<oslam_covis_update_t>(N);
    const auto fPts = lay.add<int32_t>((size_t)n_points_total);
    const auto fEx = lay.add<int32_t>((size_t)n_excl_total);
    const auto fSt = lay.add<int32_t>(N);
    const auto fOi = lay.add<int32_t>(N * K), fOw = lay.add<int32_t>(N * K);
    const auto fNo = lay.add<int32_t>(N), fPa = lay.add<int32_t>(N);
    const auto fLi = lay.add<int32_t>(N * K);
    const auto fNl = lay.add<int32_t>(N);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fRec, ph, recs); put(fPts, ph, points); put(fEx, ph, exclude);
    // the caller's output rows travel too: what the kernel does not write comes back as it was
    put(fSt, ph, status); put(fOi, ph, ordered_ids); put(fOw, ph, ordered_w); put(fNo, ph, n_ordered); put(fPa, ph, parent); put(fLi, ph, new_links); put(fNl, ph, n_new_links);
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, h->stream));
    UpdateArgs a{h->st, at(fRec, pd), n, n_points_total, n_excl_total, at(fPts, pd), at(fEx, pd), at(fSt, pd), at(fOi, pd), at(fOw, pd), at(fNo, pd), at(fPa, pd), at(fLi, pd), at(fNl, pd)};
    OSLAM_CHECK(launch_update(h, a, h->stream));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fSt.off, pd + fSt.off, lay.total() - fSt.off, hipMemcpyDeviceToHost, h->stream));
    OSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    get(fSt, ph, status); get(fOi, ph, ordered_ids); get(fOw, ph, ordered_w); get(fNo, ph, n_ordered); get(fPa, ph, parent); get(fLi, ph, new_links); get(fNl, ph, n_new_links);
    return OSLAM_OK;
}

int oslam_covis_update_connections_device(oslam_covis_t* h, int n, const oslam_covis_update_t* d_recs, int n_points_total, const int32_t* d_points, int n_excl_total,
                                          const int32_t* d_exclude, int32_t* d_status, int32_t* d_ordered_ids, int32_t* d_ordered_w, int32_t* d_n_ordered,
                                          int32_t* d_parent, int32_t* d_new_links, int32_t* d_n_new_links, void* stream) {
    const char* fn = "oslam_covis_update_connections_device";
    OSLAM_CHECK(check_counts(fn, h, n, n_points_total, n_excl_total));
    if (n == 0) return OSLAM_OK;
    if (!d_recs || !d_status || !d_ordered_ids || !d_ordered_w || !d_n_ordered || !d_parent || !d_new_links || !d_n_new_links || (n_points_total > 0 && !d_points) ||
        (n_excl_total > 0 && !d_exclude)) {
        set_error("%s: NULL argument", fn);
        return OSLAM_E_INVALID;
    }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    UpdateArgs a{h->st, d_recs, n, n_points_total, n_excl_total, d_points, d_exclude, d_status, d_ordered_ids, d_ordered_w, d_n_ordered, d_parent, d_new_links, d_n_new_links};
    return launch_update(h, a, (hipStream_t)stream);
}

int oslam_covis_covisibles(oslam_covis_t* h, int n, const oslam_covis_query_t* recs, int32_t* ids, int32_t* weights, int32_t* n_out) {
    const char* fn = "oslam_covis_covisibles";
    OSLAM_CHECK(check_counts(fn, h, n));
    if (n == 0) return OSLAM_OK;
    if (!recs || !ids || !weights || !n_out) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    std::lock_guard<std::mutex> lock(h->mu);
    const int K = h->st.K;
    for (int r = 0; r < n; r++)
        if (recs[r].graph < 0 || recs[r].graph >= h->st.n_graphs || recs[r].keyframe < 0 || recs[r].keyframe >= K) {
            set_error("%s: record %d names graph %d, keyframe %d", fn, r, recs[r].graph, recs[r].keyframe);
            return OSLAM_E_INVALID;
        }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t N = (size_t)n;
    oslam::StageLayout lay;
    const auto fRec = lay.add<oslam_covis_query_t>(N);
    const auto fIds = lay.add<int32_t>(N * K), fW = lay.add<int32_t>(N * K);
    const auto fN = lay.add<int32_t>(N);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fRec, ph, recs); put(fIds, ph, ids); put(fW, ph, weights); put(fN, ph, n_out);
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_covis_covisibles, dim3(n), dim3(kThreads), h->lds, h->stream, h->st, at(fRec, pd), at(fIds, pd), at(fW, pd), at(fN, pd));
    OSLAM_HIP_CHECK(hipGetLastError());
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fIds.off, pd + fIds.off, lay.total() - fIds.off, hipMemcpyDeviceToHost, h->stream));
    OSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    get(fIds, ph, ids); get(fW, ph, weights); get(fN, ph, n_out);
    return OSLAM_OK;
}

int oslam_covis_covisibles_device(oslam_covis_t* h, int n, const oslam_covis_query_t* d_recs, int32_t* d_ids, int32_t* d_weights, int32_t* d_n_out, void* stream) {
    const char* fn = "oslam_covis_covisibles_device";
    OSLAM_CHECK(check_counts(fn, h, n));
    if (n == 0) return OSLAM_OK;
    if (!d_recs || !d_ids || !d_weights || !d_n_out) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_covis_covisibles, dim3(n), dim3(kThreads), h->lds, (hipStream_t)stream, h->st, d_recs, d_ids, d_weights, d_n_out);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int oslam_covis_connected_rows(oslam_covis_t* h, int n, const oslam_covis_key_t* recs, uint32_t* bits) {
    const char* fn = "oslam_covis_connected_rows";
    OSLAM_CHECK(check_counts(fn, h, n));
    if (n == 0) return OSLAM_OK;
    if (!recs || !bits) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    std::lock_guard<std::mutex> lock(h->mu);
    for (int r = 0; r < n; r++)
        if (recs[r].graph < 0 || recs[r].graph >= h->st.n_graphs || recs[r].keyframe < 0 || recs[r].keyframe >= h->st.K) {
            set_error("%s: record %d names graph %d, keyframe %d", fn, r, recs[r].graph, recs[r].keyframe);
            return OSLAM_E_INVALID;
        }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t N = (size_t)n, W = (size_t)h->st.W;
    oslam::StageLayout lay;
    const auto fRec = lay.add<oslam_covis_key_t>(N);
    const auto fBits = lay.add<uint32_t>(N * W);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fRec, ph, recs);
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, fRec.end(), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_covis_connected_rows, dim3(n), dim3(kThreads), 0, h->stream, h->st, at(fRec, pd), at(fBits, pd));
    OSLAM_HIP_CHECK(hipGetLastError());
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fBits.off, pd + fBits.off, fBits.bytes, hipMemcpyDeviceToHost, h->stream));
    OSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    get(fBits, ph, bits);
    return OSLAM_OK;
}

int oslam_covis_connected_rows_device(oslam_covis_t* h, int n, const oslam_covis_key_t* d_recs, uint32_t* d_bits, void* stream) {
    const char* fn = "oslam_covis_connected_rows_device";
    OSLAM_CHECK(check_counts(fn, h, n));
    if (n == 0) return OSLAM_OK;
    if (!d_recs || !d_bits) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_covis_connected_rows, dim3(n), dim3(kThreads), 0, (hipStream_t)stream, h->st, d_recs, d_bits);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int oslam_covis_local_keyframes(oslam_covis_t* h, int n, const oslam_covis_local_t* recs, int n_points_total, const int32_t* points, int32_t* list, int32_t* n_list,
                                int32_t* ref_kf, uint8_t* null_out) {
    const char* fn = "oslam_covis_local_keyframes";
    OSLAM_CHECK(check_counts(fn, h, n, n_points_total));
    if (n == 0) return OSLAM_OK;
    if (!recs || !list || !n_list || !ref_kf || (n_points_total > 0 && (!points || !null_out))) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    std::lock_guard<std::mutex> lock(h->mu);
    const int K = h->st.K, P = h->st.P;
    for (int r = 0; r < n; r++) {
        const oslam_covis_local_t& R = recs[r];
        if (R.graph < 0 || R.graph >= h->st.n_graphs || !span_ok(R.pts_off, R.n_pts, n_points_total)) { set_error("%s: record %d names graph %d or lies outside the points", fn, r, R.graph); return OSLAM_E_INVALID; }
        for (int i = 0; i < R.n_pts; i++)
            if (points[R.pts_off + i] >= P) { set_error("%s: record %d's point %d is id %d of %d", fn, r, i, points[R.pts_off + i], P); return OSLAM_E_INVALID; }
    }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t N = (size_t)n;
    oslam::StageLayout lay;
    const auto fRec = lay.add<oslam_covis_local_t>(N);
    const auto fPts = lay.add<int32_t>((size_t)n_points_total);
    const auto fList = lay.add<int32_t>(N * K);
    const auto fNl = lay.add<int32_t>(N), fRef = lay.add<int32_t>(N);
    const auto fNull = lay.add<uint8_t>((size_t)n_points_total);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fRec, ph, recs); put(fPts, ph, points); put(fList, ph, list); put(fNl, ph, n_list); put(fRef, ph, ref_kf); put(fNull, ph, null_out);
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, h->stream));
    LocalArgs a{h->st, at(fRec, pd), n_points_total, at(fPts, pd), at(fList, pd), at(fNl, pd), at(fRef, pd), at(fNull, pd)};
    OSLAM_CHECK(launch_local(h, n, a, h->stream));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fList.off, pd + fList.off, lay.total() - fList.off, hipMemcpyDeviceToHost, h->stream));
    OSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    get(fList, ph, list); get(fNl, ph, n_list); get(fRef, ph, ref_kf); get(fNull, ph, null_out);
    return OSLAM_OK;
}

int oslam_covis_local_keyframes_device(oslam_covis_t* h, int n, const oslam_covis_local_t* d_recs, int n_points_total, const int32_t* d_points, int32_t* d_list,
                                       int32_t* d_n_list, int32_t* d_ref_kf, uint8_t* d_null_out, void* stream) {
    const char* fn = "oslam_covis_local_keyframes_device";
    OSLAM_CHECK(check_counts(fn, h, n, n_points_total));
    if (n == 0) return OSLAM_OK;
    if (!d_recs || !d_list || !d_n_list || !d_ref_kf || (n_points_total > 0 && (!d_points || !d_null_out))) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    LocalArgs a{h->st, d_recs, n_points_total, d_points, d_list, d_n_list, d_ref_kf, d_null_out};
    return launch_local(h, n, a, (hipStream_t)stream);
}

int oslam_covis_get_state(oslam_covis_t* h, int graph, int32_t* weights, int32_t* parents, uint32_t* kf_flags, int n_points, const int32_t* points, int32_t* obs,
                          int32_t* obs_count, uint32_t* point_flags) {
    const char* fn = "oslam_covis_get_state";
    OSLAM_CHECK(check_counts(fn, h, n_points));
    if (graph < 0 || graph >= h->st.n_graphs) { set_error("%s: graph %d of %d", fn, graph, h->st.n_graphs); return OSLAM_E_INVALID; }
    if (n_points > 0 && (!points || !obs || !obs_count || !point_flags)) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    std::lock_guard<std::mutex> lock(h->mu);
    const size_t K = (size_t)h->st.K, P = (size_t)h->st.P, C = (size_t)h->st.C, g = (size_t)graph;
    for (int i = 0; i < n_points; i++)
        if (points[i] < 0 || (size_t)points[i] >= P) { set_error("%s: point %d is id %d of %zu", fn, i, points[i], P); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    oslam::StageLayout lay;
    const auto fW = lay.add<int32_t>(K * K, weights != nullptr);
    const auto fPa = lay.add<int32_t>(K, parents != nullptr);
    const auto fKm = lay.add<uint32_t>(K, kf_flags != nullptr);
    const auto fPm = lay.add<uint32_t>(P, n_points > 0);
    const auto fOb = lay.add<int32_t>(P * C * 2, n_points > 0);
    OSLAM_CHECK(h->io.h.grow(lay.total(), 4096));
    uint8_t* ph = h->io.h.bytes();
    if (fW.bytes) OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fW.off, h->weights.bytes() + g * K * K * 4, fW.bytes, hipMemcpyDeviceToHost, h->stream));
    if (fPa.bytes) OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fPa.off, h->parent.bytes() + g * K * 4, fPa.bytes, hipMemcpyDeviceToHost, h->stream));
    if (fKm.bytes) OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fKm.off, h->kmeta.bytes() + g * K * 4, fKm.bytes, hipMemcpyDeviceToHost, h->stream));
    if (fPm.bytes) OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fPm.off, h->pmeta.bytes() + g * P * 4, fPm.bytes, hipMemcpyDeviceToHost, h->stream));
    if (fOb.bytes) OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fOb.off, h->obs.bytes() + g * P * C * 8, fOb.bytes, hipMemcpyDeviceToHost, h->stream));
    OSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    get(fW, ph, weights); get(fPa, ph, parents); get(fKm, ph, kf_flags);
    for (int i = 0; i < n_points; i++) {
        const size_t p = (size_t)points[i];
        const uint32_t meta = at(fPm, ph)[p];
        obs_count[i] = (int32_t)(meta & kPtCnt);
        point_flags[i] = meta >> 8;
        memcpy(obs + (size_t)i * C * 2, at(fOb, ph) + p * C * 2, C * 8);
    }
    return OSLAM_OK;
}

}  // extern "C"
