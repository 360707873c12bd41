// loop_detect.hip — LoopClosing::DetectLoop (reference src/LoopClosing.cc:104-230) for many independent sequences resident on gfx950 (include/oslam_hip.h,
// "LoopClosing::DetectLoop"): a detector handle over a borrowed KeyFrameDatabase handle.  Per database it keeps the connected-keyframe bitset of every
// keyframe and mvConsistentGroups (bitsets with counters, two banks).  The consistency update is one launch of k_loopdet_update, one workgroup per query:
// the previous groups in LDS, one wavefront per candidate holding its row one word per lane and meeting every previous group with one ballot, first(g) by an
// integer LDS atomicMin, one wavefront turning the masks into list positions with a scan, all threads copying the pushed groups into the other bank.  detect
// chains the kfdb's loop query (its bound derived in the kernel) with that update on one stream.  No atomics on global memory, nothing whose result depends
// on the order the hardware runs anything in.  Product code; never includes oracle/.
#include <climits>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "common.h"
#include "kfdb_state.h"
#include "stage_layout.h"

using oslam::set_error;

namespace {

constexpr int kThreads = 512, kWaves = kThreads / 64;
constexpr int kMaxGroups = OSLAM_LOOPDET_MAX_GROUPS;
static_assert(kMaxGroups == 64, "a candidate's consistency with the previous groups is one 64-bit mask");
static_assert(OSLAM_KFDB_MAX_KEYFRAMES <= 64 * 32, "a row is at most one word per lane");

// the resident state as the kernels see it
struct LoopdetState {
    uint32_t* rows;      // [n_db][K][W] connected bitsets
    uint32_t* gbits;     // [n_db][2][G][W] the groups' bitsets, two banks
    int32_t* gcnt;       // [n_db][2][G] their consistency counters
    int32_t* ngroups;    // [n_db] groups in the current bank
    int32_t* bank;       // [n_db] the current bank
    int n_db, K, W, G, th;
};

}  // namespace

struct oslam_loopdet {
    oslam_kfdb* db = nullptr;
    int device = 0;
    size_t lds = 0;
    LoopdetState st{};
    oslam::DeviceBuffer rows, gbits, gcnt, ngroups, bank;
    hipStream_t stream = nullptr;   // the kfdb's
    oslam::StagePair io;
    std::mutex mu;
};

namespace {

// One workgroup (one wavefront) per record: the record's ids into a row in LDS (integer OR: any order), the row to its place.  n < 0: a later record of the
// call names the same keyframe and this one is skipped.
__global__ __launch_bounds__(64) void k_loopdet_set_rows(LoopdetState st, const oslam_loopdet_conn_t* recs, const int32_t* ids) {
    const oslam_loopdet_conn_t r = recs[blockIdx.x];
    if (r.n < 0) return;   // (uniform)
    __shared__ uint32_t s_row[64];
    const int lane = threadIdx.x;
    s_row[lane] = 0;
    __syncthreads();
    for (int j = lane; j < r.n; j += 64) {
        const int id = ids[r.off + j];
        if (id >= 0 && id < st.K) atomicOr(&s_row[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
    if (lane < st.W) st.rows[((size_t)r.database * st.K + r.keyframe) * st.W + lane] = s_row[lane];
}

struct UpdateArgs {
    LoopdetState st;
    const oslam_loopdet_update_t* recs;   // update_consistency: the records and the packed candidates
    const oslam_kfdb_query_t* queries;    // detect (recs == NULL): the queries, their n_cand and candidate rows [q][K] as k_kfdb_query left them
    const int32_t* q_n_cand;
    int n_q, n_cand_total;
    const int32_t* cand;
    int32_t* enough; int32_t* n_enough; int32_t* n_groups;
};

size_t lds_bytes(int K, int W, int G) { return (size_t)K * 12 + (size_t)G * W * 4; }

__global__ __launch_bounds__(kThreads) void k_loopdet_update(UpdateArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.st.K, W = a.st.W, G = a.st.G;

    extern __shared__ __align__(16) uint8_t smem[];
    unsigned long long* s_mask = (unsigned long long*)smem;   // [K] bit g: candidate i is consistent with previous group g
    int* s_base = (int*)(s_mask + K);                         // [K] groups pushed before candidate i
    uint32_t* s_prev = (uint32_t*)(s_base + K);               // [G][W] the previous groups
    __shared__ int s_prevcnt[kMaxGroups], s_first[kMaxGroups], s_src[kMaxGroups], s_newcnt[kMaxGroups];
    __shared__ int s_bad, s_total;
    __shared__ unsigned long long s_hot;

    // ---- the record ----
    int d, nc;
    size_t cand_off;
    bool ok;
    if (a.recs) {
        const oslam_loopdet_update_t r = a.recs[b];
        d = r.database; nc = r.n_cand; cand_off = (size_t)(r.cand_off > 0 ? r.cand_off : 0);
        ok = nc >= 0 && nc <= K && r.cand_off >= 0 && r.cand_off <= a.n_cand_total - nc;
    } else {
        d = a.queries[b].database; nc = a.q_n_cand[b]; cand_off = (size_t)b * K;
        ok = nc >= 0 && nc <= K;   // (-2: the kfdb refused the query, both queries of a pair on one database included)
    }
    ok = ok && d >= 0 && d < a.st.n_db;
    const int32_t* cand = a.cand + cand_off;
    if (tid == 0) { s_bad = ok ? 0 : 1; s_total = 0; }
    if (tid < kMaxGroups) s_first[tid] = INT_MAX;
    __syncthreads();
    if (ok) {
        if (a.recs)
            for (int i = tid; i < a.n_q; i += kThreads)
                if (i != b && a.recs[i].database == d) s_bad = 1;   // two queries on one database: both are refused
        for (int i = tid; i < nc; i += kThreads) {
            const int id = cand[i];
            if (id < 0 || id >= K) s_bad = 1;
        }
    }
    __syncthreads();
    if (s_bad) {   // (uniform)
        if (tid == 0) a.n_enough[b] = -2;
        return;
    }
    if (nc == 0) {   // mvConsistentGroups.clear() (:145-151)
        if (tid == 0) { a.st.ngroups[d] = 0; a.n_enough[b] = 0; a.n_groups[b] = 0; }
        return;
    }

    // ---- the previous groups ----
    const int bank = a.st.bank[d], ng = a.st.ngroups[d];
    {
        const uint32_t* pb = a.st.gbits + ((size_t)d * 2 + bank) * G * W;
        const int32_t* pc = a.st.gcnt + ((size_t)d * 2 + bank) * G;
        for (int i = tid; i < ng * W; i += kThreads) s_prev[i] = pb[i];
        if (tid < ng) s_prevcnt[tid] = pc[tid];
    }
    __syncthreads();
    if (wave == 0) {   // the groups a candidate is "enough" with: nCurrentConsistency >= mnCovisibilityConsistencyTh (:195)
        const unsigned long long hot = __ballot(lane < ng ? s_prevcnt[lane] + 1 >= a.st.th : false);
        if (lane == 0) s_hot = hot;
    }

    // ---- C(i, .): a wavefront per candidate, its group one word per lane ----
    const uint32_t* rows = a.st.rows + (size_t)d * K * W;
    for (int i = wave; i < nc; i += kWaves) {
        const int c = cand[i];
        uint32_t w = lane < W ? rows[(size_t)c * W + lane] : 0u;
        if (lane == (c >> 5)) w |= 1u << (c & 31);   // spCandidateGroup.insert(pCandidateKF) (:166)
        unsigned long long m = 0;
        for (int g = 0; g < ng; g++) {
            const bool hit = lane < W && (w & s_prev[g * W + lane]) != 0u;
            if (__ballot(hit)) m |= 1ull << g;
        }
        if (lane == 0) s_mask[i] = m;
        if (lane < ng && ((m >> lane) & 1ull)) atomicMin(&s_first[lane], i);   // first(g) (an integer minimum: any order)
    }
    __syncthreads();

    // ---- list positions: candidate i pushes one group per g with first(g) == i, or one fresh group when it met none ----
    if (wave == 0) {
        int run = 0;
        for (int i0 = 0; i0 < nc; i0 += 64) {
            const int i = i0 + lane;
            int p = 0;
            if (i < nc) {
                const unsigned long long m = s_mask[i];
                if (m == 0) p = 1;
                else
                    for (int g = 0; g < ng; g++) p += (((m >> g) & 1ull) && s_first[g] == i) ? 1 : 0;
            }
            int x = p;   // inclusive scan over the wavefront
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(x, o);
                if (lane >= o) x += y;
            }
            if (i < nc) s_base[i] = run + x - p;
            run += __shfl(x, 63);
        }
        if (lane == 0) s_total = run;
    }
    __syncthreads();
    const int total = s_total;
    if (total > G) {   // (uniform) the new list does not fit: nothing changes
        if (tid == 0) a.n_enough[b] = -3;
        return;
    }
    if (tid < ng) {
        const int f = s_first[tid];
        if (f != INT_MAX) {
            int rank = 0;
            for (int g = 0; g < tid; g++) rank += s_first[g] == f ? 1 : 0;
            const int pos = s_base[f] + rank;
            s_src[pos] = f; s_newcnt[pos] = s_prevcnt[tid] + 1;
        }
    }
    for (int i = tid; i < nc; i += kThreads)
        if (s_mask[i] == 0) { const int pos = s_base[i]; s_src[pos] = i; s_newcnt[pos] = 0; }
    __syncthreads();

    // ---- vCurrentConsistentGroups into the other bank ----
    {
        uint32_t* nb = a.st.gbits + ((size_t)d * 2 + (bank ^ 1)) * G * W;
        int32_t* ncnt = a.st.gcnt + ((size_t)d * 2 + (bank ^ 1)) * G;
        for (int x = tid; x < total * W; x += kThreads) {
            const int p = x / W, wi = x - p * W;
            const int c = cand[s_src[p]];
            uint32_t v = rows[(size_t)c * W + wi];
            if (wi == (c >> 5)) v |= 1u << (c & 31);
            nb[x] = v;
        }
        if (tid < total) ncnt[tid] = s_newcnt[tid];
    }
    // ---- mvpEnoughConsistentCandidates in candidate order: one wavefront compacts 64 candidates at a time ----
    if (wave == 0) {
        const unsigned long long hot = s_hot;
        int nout = 0;
        for (int i0 = 0; i0 < nc; i0 += 64) {
            const int i = i0 + lane;
            const bool keep = i < nc && (s_mask[i] & hot) != 0ull;
            const unsigned long long mask = __ballot(keep);
            if (keep) a.enough[(size_t)b * K + nout + __popcll(mask & ((1ull << lane) - 1ull))] = cand[i];
            nout += __popcll(mask);
        }
        if (lane == 0) {
            a.n_enough[b] = nout; a.n_groups[b] = total;
            a.st.ngroups[d] = total; a.st.bank[d] = bank ^ 1;   // mvConsistentGroups = vCurrentConsistentGroups (:212)
        }
    }
}

int launch_update(oslam_loopdet* h, int n_queries, const oslam_loopdet_update_t* d_recs, const oslam_kfdb_query_t* d_queries, const int32_t* d_q_n_cand, int n_cand_total,
                  const int32_t* d_cand, int32_t* d_enough, int32_t* d_n_enough, int32_t* d_n_groups, hipStream_t stream) {
    UpdateArgs a;
    a.st = h->st; a.recs = d_recs; a.queries = d_queries; a.q_n_cand = d_q_n_cand; a.n_q = n_queries; a.n_cand_total = n_cand_total; a.cand = d_cand;
    a.enough = d_enough; a.n_enough = d_n_enough; a.n_groups = d_n_groups;
    hipLaunchKernelGGL(k_loopdet_update, dim3(n_queries), dim3(kThreads), h->lds, stream, a);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int check_update_call(const char* fn, const oslam_loopdet* h, int n_queries, int n_cand_total) {
    if (!h) { set_error("%s: NULL handle", fn); return OSLAM_E_INVALID; }
    if (n_queries < 0 || n_cand_total < 0) { set_error("%s: a count is negative", fn); return OSLAM_E_INVALID; }
    if (n_queries > h->st.n_db) { set_error("%s: %d queries for %d databases (one query per database and call)", fn, n_queries, h->st.n_db); return OSLAM_E_INVALID; }
    return OSLAM_OK;
}

}  // namespace

extern "C" {

void oslam_loopdet_destroy(oslam_loopdet_t* h) {
    if (!h) return;
    delete h;
}

int oslam_loopdet_create(oslam_loopdet_t** out, oslam_kfdb_t* kfdb, int max_groups, int consistency_th) {
    const char* fn = "oslam_loopdet_create";
    if (!out) { set_error("%s: out is NULL", fn); return OSLAM_E_INVALID; }
    *out = nullptr;
    if (!kfdb) { set_error("%s: NULL KeyFrameDatabase handle", fn); return OSLAM_E_INVALID; }
    if (max_groups < 1 || max_groups > kMaxGroups || consistency_th < 1) {
        set_error("%s: max_groups %d outside 1 .. %d, or consistency_th %d < 1", fn, max_groups, kMaxGroups, consistency_th);
        return OSLAM_E_INVALID;
    }
    OSLAM_HIP_CHECK(hipSetDevice(kfdb->device));
    oslam_loopdet* h = new oslam_loopdet;
    h->db = kfdb; h->device = kfdb->device; h->stream = kfdb->stream;
    const int n_db = kfdb->st.n_db, K = kfdb->st.K, W = oslam::div_up(K, 32), G = max_groups;
    h->lds = lds_bytes(K, W, G);
    const size_t row_bytes = (size_t)n_db * K * W * 4, gb_bytes = (size_t)n_db * 2 * G * W * 4, gc_bytes = (size_t)n_db * 2 * G * 4, db_bytes = (size_t)n_db * 4;
    int rc = OSLAM_OK;
    if ((rc = h->rows.alloc(row_bytes)) || (rc = h->gbits.alloc(gb_bytes)) || (rc = h->gcnt.alloc(gc_bytes)) || (rc = h->ngroups.alloc(db_bytes)) || (rc = h->bank.alloc(db_bytes))) {
        delete h;
        return rc;
    }
    hipError_t e = hipMemsetAsync(h->rows.ptr(), 0, row_bytes, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->gbits.ptr(), 0, gb_bytes, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->gcnt.ptr(), 0, gc_bytes, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->ngroups.ptr(), 0, db_bytes, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->bank.ptr(), 0, db_bytes, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        set_error("%s: %s", fn, hipGetErrorString(e));
        delete h;
        return OSLAM_E_HIP;
    }
    h->st = LoopdetState{h->rows.as<uint32_t>(), h->gbits.as<uint32_t>(), h->gcnt.as<int32_t>(), h->ngroups.as<int32_t>(), h->bank.as<int32_t>(), n_db, K, W, G, consistency_th};
    *out = h;
    return OSLAM_OK;
}

int oslam_loopdet_set_connected(oslam_loopdet_t* h, int n, const oslam_loopdet_conn_t* recs, int n_ids_total, const int32_t* ids) {
    const char* fn = "oslam_loopdet_set_connected";
    if (!h || n < 0 || n_ids_total < 0 || (n > 0 && !recs) || (n_ids_total > 0 && !ids)) { set_error("%s: bad argument", fn); return OSLAM_E_INVALID; }
    if (n == 0) return OSLAM_OK;
    std::lock_guard<std::mutex> lock(h->mu);
    for (int r = 0; r < n; r++) {
        const oslam_loopdet_conn_t& c = recs[r];
        if (c.database < 0 || c.database >= h->st.n_db || c.keyframe < 0 || c.keyframe >= h->st.K) {
            set_error("%s: record %d names database %d, keyframe %d", fn, r, c.database, c.keyframe);
            return OSLAM_E_INVALID;
        }
        if (c.n < 0 || c.off < 0 || c.off > n_ids_total - c.n) { set_error("%s: record %d's ids lie outside the %d given", fn, r, n_ids_total); return OSLAM_E_INVALID; }
    }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    oslam::StageLayout lay;
    const auto fRec = lay.add<oslam_loopdet_conn_t>((size_t)n);
    const auto fIds = lay.add<int32_t>((size_t)n_ids_total);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fRec, ph, recs); put(fIds, ph, ids);
    // record order: of the records that name one keyframe only the last is applied (the workgroups of a launch run in no order)
    oslam_loopdet_conn_t* sr = at(fRec, ph);
    std::map<std::pair<int32_t, int32_t>, int> last;
    for (int r = n - 1; r >= 0; r--)
        if (!last.emplace(std::make_pair(sr[r].database, sr[r].keyframe), r).second) sr[r].n = -1;
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_loopdet_set_rows, dim3(n), dim3(64), 0, h->stream, h->st, at(fRec, pd), at(fIds, pd));
    OSLAM_HIP_CHECK(hipGetLastError());
    OSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    return OSLAM_OK;
}

int oslam_loopdet_reset(oslam_loopdet_t* h, int n, const int32_t* databases) {
    const char* fn = "oslam_loopdet_reset";
    if (!h || n < 0 || (n > 0 && !databases)) { set_error("%s: bad argument", fn); return OSLAM_E_INVALID; }
    if (n == 0) return OSLAM_OK;
    std::lock_guard<std::mutex> lock(h->mu);
    for (int r = 0; r < n; r++)
        if (databases[r] < 0 || databases[r] >= h->st.n_db) { set_error("%s: record %d names database %d of %d", fn, r, databases[r], h->st.n_db); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t row_bytes = (size_t)h->st.K * h->st.W * 4;
    for (int r = 0; r < n; r++) {
        const size_t d = (size_t)databases[r];
        OSLAM_HIP_CHECK(hipMemsetAsync(h->rows.bytes() + d * row_bytes, 0, row_bytes, h->stream));
        OSLAM_HIP_CHECK(hipMemsetAsync(h->ngroups.bytes() + d * 4, 0, 4, h->stream));
    }
    OSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    return OSLAM_OK;
}

int oslam_loopdet_get_groups(oslam_loopdet_t* h, int database, int32_t* n_out, int32_t* consistency_out, uint32_t* bits_out) {
    const char* fn = "oslam_loopdet_get_groups";
    if (!h || !n_out || !consistency_out || !bits_out) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    if (database < 0 || database >= h->st.n_db) { set_error("%s: database %d of %d", fn, database, h->st.n_db); return OSLAM_E_INVALID; }
    std::lock_guard<std::mutex> lock(h->mu);
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t G = (size_t)h->st.G, W = (size_t)h->st.W, d = (size_t)database;
    oslam::StageLayout lay;
    const auto fN = lay.add<int32_t>(1), fBank = lay.add<int32_t>(1);
    const auto fCnt = lay.add<int32_t>(G);
    const auto fBits = lay.add<uint32_t>(G * W);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t* ph = h->io.h.bytes();
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fN.off, h->ngroups.bytes() + d * 4, 4, hipMemcpyDeviceToHost, h->stream));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fBank.off, h->bank.bytes() + d * 4, 4, hipMemcpyDeviceToHost, h->stream));
    OSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    const size_t bank = (size_t)(*at(fBank, ph) & 1);
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fCnt.off, h->gcnt.bytes() + (d * 2 + bank) * G * 4, fCnt.bytes, hipMemcpyDeviceToHost, h->stream));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fBits.off, h->gbits.bytes() + (d * 2 + bank) * G * W * 4, fBits.bytes, hipMemcpyDeviceToHost, h->stream));
    OSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    get(fN, ph, n_out); get(fCnt, ph, consistency_out); get(fBits, ph, bits_out);
    return OSLAM_OK;
}

int oslam_loopdet_update_consistency(oslam_loopdet_t* h, int n_queries, const oslam_loopdet_update_t* recs, int n_cand_total, const int32_t* cand, int32_t* enough,
                                     int32_t* n_enough, int32_t* n_groups) {
    const char* fn = "oslam_loopdet_update_consistency";
    OSLAM_CHECK(check_update_call(fn, h, n_queries, n_cand_total));
    if (n_queries == 0) return OSLAM_OK;
    if (!recs || !enough || !n_enough || !n_groups || (n_cand_total > 0 && !cand)) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    std::lock_guard<std::mutex> lock(h->mu);
    const int K = h->st.K;
    std::vector<uint8_t> seen(h->st.n_db, 0);
    for (int q = 0; q < n_queries; q++) {
        const oslam_loopdet_update_t& R = recs[q];
        if (R.database < 0 || R.database >= h->st.n_db) { set_error("%s: query %d names database %d of %d", fn, q, R.database, h->st.n_db); return OSLAM_E_INVALID; }
        if (seen[R.database]) { set_error("%s: query %d is the second on database %d in this call (updates of one database are sequential)", fn, q, R.database); return OSLAM_E_INVALID; }
        seen[R.database] = 1;
        if (R.n_cand < 0 || R.n_cand > K || R.cand_off < 0 || R.cand_off > n_cand_total - R.n_cand) {
            set_error("%s: query %d's %d candidates at %d lie outside the %d given, or are more than a database's %d keyframes", fn, q, R.n_cand, R.cand_off, n_cand_total, K);
            return OSLAM_E_INVALID;
        }
        for (int i = 0; i < R.n_cand; i++)
            if (cand[R.cand_off + i] < 0 || cand[R.cand_off + i] >= K) { set_error("%s: query %d's candidate %d is keyframe %d of %d", fn, q, i, cand[R.cand_off + i], K); return OSLAM_E_INVALID; }
    }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t nq = (size_t)n_queries;
    oslam::StageLayout lay;   // one block, inputs then outputs: one upload, one download
    const auto fRec = lay.add<oslam_loopdet_update_t>(nq);
    const auto fCand = lay.add<int32_t>((size_t)n_cand_total);
    const auto fEn = lay.add<int32_t>(nq * K);
    const auto fNe = lay.add<int32_t>(nq), fNg = lay.add<int32_t>(nq);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fRec, ph, recs); put(fCand, ph, cand);
    put(fEn, ph, enough); put(fNe, ph, n_enough); put(fNg, ph, n_groups);   // what the kernel does not write comes back as it was
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, h->stream));
    OSLAM_CHECK(launch_update(h, n_queries, at(fRec, pd), nullptr, nullptr, n_cand_total, at(fCand, pd), at(fEn, pd), at(fNe, pd), at(fNg, pd), h->stream));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fEn.off, pd + fEn.off, lay.total() - fEn.off, hipMemcpyDeviceToHost, h->stream));
    OSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    get(fEn, ph, enough); get(fNe, ph, n_enough); get(fNg, ph, n_groups);
    return OSLAM_OK;
}

int oslam_loopdet_update_consistency_device(oslam_loopdet_t* h, int n_queries, const oslam_loopdet_update_t* d_recs, int n_cand_total, const int32_t* d_cand,
                                            int32_t* d_enough, int32_t* d_n_enough, int32_t* d_n_groups, void* stream) {
    const char* fn = "oslam_loopdet_update_consistency_device";
    OSLAM_CHECK(check_update_call(fn, h, n_queries, n_cand_total));
    if (n_queries == 0) return OSLAM_OK;
    if (!d_recs || !d_enough || !d_n_enough || !d_n_groups || (n_cand_total > 0 && !d_cand)) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    return launch_update(h, n_queries, d_recs, nullptr, nullptr, n_cand_total, d_cand, d_enough, d_n_enough, d_n_groups, (hipStream_t)stream);
}

int oslam_loopdet_detect(oslam_loopdet_t* h, const oslam_voc_t* voc, int n_queries, const oslam_kfdb_query_t* queries, int n_words_total, const uint32_t* ids,
                         const double* vals, int n_conn_total, const int32_t* conn, int32_t* cand, float* cand_acc, int32_t* n_cand, int32_t* diag, float* conn_score,
                         float* min_score, int32_t* enough, int32_t* n_enough, int32_t* n_groups) {
    const char* fn = "oslam_loopdet_detect";
    if (!h) { set_error("%s: NULL handle", fn); return OSLAM_E_INVALID; }
    oslam_kfdb* db = h->db;
    OSLAM_CHECK(oslam::kfdb_check_query_call(fn, db, voc, n_queries, n_words_total, n_conn_total));
    if (n_queries == 0) return OSLAM_OK;
    if (!queries || !cand || !cand_acc || !n_cand || !diag || !min_score || !enough || !n_enough || !n_groups || (n_words_total > 0 && (!ids || !vals)) ||
        (n_conn_total > 0 && (!conn || !conn_score))) {
        set_error("%s: NULL argument", fn);
        return OSLAM_E_INVALID;
    }
    std::lock_guard<std::mutex> lock(h->mu);
    std::lock_guard<std::mutex> lock_db(db->mu);   // (the query reads the database's state on its stream)
    OSLAM_CHECK(oslam::kfdb_check_queries(fn, db, true, n_queries, queries, n_words_total, ids, n_conn_total));
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const int K = h->st.K;
    const size_t nq = (size_t)n_queries, NW = (size_t)n_words_total, NC = (size_t)n_conn_total;
    oslam::StageLayout lay;   // one block, inputs then outputs: one upload, two launches, one download
    const auto fQ = lay.add<oslam_kfdb_query_t>(nq);
    const auto fIds = lay.add<uint32_t>(NW);
    const auto fVals = lay.add<double>(NW);
    const auto fConn = lay.add<int32_t>(NC);
    const auto fCand = lay.add<int32_t>(nq * K);
    const auto fAcc = lay.add<float>(nq * K);
    const auto fN = lay.add<int32_t>(nq), fDiag = lay.add<int32_t>(nq * 5);
    const auto fCs = lay.add<float>(NC);
    const auto fMs = lay.add<float>(nq);
    const auto fEn = lay.add<int32_t>(nq * K);
    const auto fNe = lay.add<int32_t>(nq), fNg = lay.add<int32_t>(nq);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fQ, ph, queries); put(fIds, ph, ids); put(fVals, ph, vals); put(fConn, ph, conn);
    // the caller's output rows travel too: what the kernels do not write comes back as it was
    put(fCand, ph, cand); put(fAcc, ph, cand_acc); put(fN, ph, n_cand); put(fDiag, ph, diag); put(fCs, ph, conn_score); put(fMs, ph, min_score);
    put(fEn, ph, enough); put(fNe, ph, n_enough); put(fNg, ph, n_groups);
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, h->stream));
    OSLAM_CHECK(oslam::kfdb_launch_query(db, true, n_queries, at(fQ, pd), n_words_total, at(fIds, pd), at(fVals, pd), n_conn_total, at(fConn, pd), at(fCand, pd), at(fAcc, pd),
                                         at(fN, pd), at(fDiag, pd), at(fCs, pd), at(fMs, pd), h->stream));
    OSLAM_CHECK(launch_update(h, n_queries, nullptr, at(fQ, pd), at(fN, pd), 0, at(fCand, pd), at(fEn, pd), at(fNe, pd), at(fNg, pd), h->stream));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fCand.off, pd + fCand.off, lay.total() - fCand.off, hipMemcpyDeviceToHost, h->stream));
    OSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    get(fCand, ph, cand); get(fAcc, ph, cand_acc); get(fN, ph, n_cand); get(fDiag, ph, diag); get(fCs, ph, conn_score); get(fMs, ph, min_score);
    get(fEn, ph, enough); get(fNe, ph, n_enough); get(fNg, ph, n_groups);
    return OSLAM_OK;
}

int oslam_loopdet_detect_device(oslam_loopdet_t* h, const oslam_voc_t* voc, int n_queries, const oslam_kfdb_query_t* d_queries, int n_words_total, const uint32_t* d_ids,
                                const double* d_vals, int n_conn_total, const int32_t* d_conn, int32_t* d_cand, float* d_cand_acc, int32_t* d_n_cand, int32_t* d_diag,
                                float* d_conn_score, float* d_min_score, int32_t* d_enough, int32_t* d_n_enough, int32_t* d_n_groups, void* stream) {
    const char* fn = "oslam_loopdet_detect_device";
    if (!h) { set_error("%s: NULL handle", fn); return OSLAM_E_INVALID; }
    OSLAM_CHECK(oslam::kfdb_check_query_call(fn, h->db, voc, n_queries, n_words_total, n_conn_total));
    if (n_queries == 0) return OSLAM_OK;
    if (!d_queries || !d_cand || !d_cand_acc || !d_n_cand || !d_diag || !d_min_score || !d_enough || !d_n_enough || !d_n_groups || (n_words_total > 0 && (!d_ids || !d_vals)) ||
        (n_conn_total > 0 && (!d_conn || !d_conn_score))) {
        set_error("%s: NULL argument", fn);
        return OSLAM_E_INVALID;
    }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    OSLAM_CHECK(oslam::kfdb_launch_query(h->db, true, n_queries, d_queries, n_words_total, d_ids, d_vals, n_conn_total, d_conn, d_cand, d_cand_acc, d_n_cand, d_diag, d_conn_score,
                                         d_min_score, (hipStream_t)stream));
    return launch_update(h, n_queries, nullptr, d_queries, d_n_cand, 0, d_cand, d_enough, d_n_enough, d_n_groups, (hipStream_t)stream);
}

}  // extern "C"
