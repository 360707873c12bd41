// keyframe_db.hip — ORB_SLAM2::KeyFrameDatabase (reference src/KeyFrameDatabase.cc:33-309) for many independent databases resident on gfx950
// (include/oslam_hip.h, "KeyFrameDatabase").  The BowVectors of the keyframes live in chunks of 128 words of one pool; the host owns the free list
// and the chunk tables' contents, small kernels apply the mutations.  A query call is one launch of k_kfdb_query, one workgroup per query: the query
// vector in LDS, a count pass over the word ids of every present slot (16 lanes per keyframe, binary search in LDS), the workgroup maximum, a score
// pass over the survivors and the connected ids, a bitonic sort of the survivors by (smallest common word, add serial) in LDS, then accumulation,
// threshold and dedup.  No inverted file, no atomics on global memory, nothing whose result depends on the order the hardware runs anything in (the
// LDS atomics are integer max / min / add, and list positions taken with them are sorted afterwards).  For loop_detect.hip a loop query can derive its
// bound from the connected scores itself (kfdb_state.h: kfdb_launch_query with a min_score array).  Product code; never includes oracle/.
#include <algorithm>
#include <climits>
#include <cmath>
#include <mutex>
#include <vector>

#include "common.h"
#include "kfdb_state.h"
#include "lane_ops.h"
#include "stage_layout.h"

using oslam::KfdbState;   // (the resident state and the handle: kfdb_state.h, shared with loop_detect.hip)
using oslam::set_error;

namespace {

constexpr int kThreads = 512, kGroup = 16, kGroups = kThreads / kGroup;
constexpr int kChunk = OSLAM_KFDB_CHUNK, kCovis = OSLAM_KFDB_COVIS;
constexpr int kMutThreads = 256;

struct AddRec { int32_t slot, n_words, word_off, chunk_off; uint32_t serial; };

// One workgroup per record: the staged words into the slot's chunks, the chunk table, the slot's fields.
__global__ __launch_bounds__(kMutThreads) void k_kfdb_add(KfdbState st, const AddRec* recs, const uint32_t* ids, const double* vals, const int32_t* chunk_list) {
    const AddRec r = recs[blockIdx.x];
    const int nc = (r.n_words + kChunk - 1) / kChunk;
    int32_t* ch = st.chunks + (size_t)r.slot * st.MC;
    for (int i = threadIdx.x; i < nc; i += kMutThreads) ch[i] = chunk_list[r.chunk_off + i];
    for (int i = threadIdx.x; i < r.n_words; i += kMutThreads) {
        const size_t at = (size_t)chunk_list[r.chunk_off + i / kChunk] * kChunk + i % kChunk;
        st.pool_ids[at] = ids[r.word_off + i];
        st.pool_vals[at] = vals[r.word_off + i];
    }
    if (threadIdx.x < kCovis) st.covis[(size_t)r.slot * kCovis + threadIdx.x] = -1;
    if (threadIdx.x == 0) { st.nwords[r.slot] = r.n_words; st.serial[r.slot] = r.serial; st.reloc[r.slot] = 0.0f; }
}

// (database, keyframe); keyframe < 0: every slot of the database
__global__ __launch_bounds__(kMutThreads) void k_kfdb_erase(KfdbState st, const oslam_kfdb_key_t* recs) {
    const oslam_kfdb_key_t r = recs[blockIdx.x];
    const size_t base = (size_t)r.database * st.K;
    if (r.keyframe >= 0) { if (threadIdx.x == 0) st.nwords[base + r.keyframe] = -1; return; }
    for (int k = threadIdx.x; k < st.K; k += kMutThreads) st.nwords[base + k] = -1;
}

__global__ void k_kfdb_covis(KfdbState st, const oslam_kfdb_covis_t* recs, int n) {
    // (one thread per record, in one workgroup: a keyframe named twice keeps its last list, as record order asks)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int i = 0; i < n; i++) {
        const oslam_kfdb_covis_t& r = recs[i];
        int32_t* c = st.covis + ((size_t)r.database * st.K + r.keyframe) * kCovis;
        for (int j = 0; j < kCovis; j++) c[j] = j < r.n ? r.ids[j] : -1;
    }
}

struct QueryArgs {
    KfdbState st;
    const oslam_kfdb_query_t* q;
    int n_q, n_words_total, n_conn_total, loop, P;
    const uint32_t* ids; const double* vals; const int32_t* conn;
    int32_t* cand; float* cand_acc; int32_t* n_cand; int32_t* diag; float* conn_score;
    float* min_score;   // not NULL: the bound of a loop query is derived from its connected scores and written here
};

size_t lds_bytes(int K, int MW, int P) {
    // query vals 8 + ids 4 per word; sort keys 8 + slots 4 per entry; words, minw, score, acc, best, first 4 each and a flag byte per slot
    return (size_t)MW * 12 + (size_t)P * 12 + (size_t)K * 25 + 64;
}

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, true); }
// minimum over a row of 16 lanes, in every lane of the row (DPP row_ror:8, 4, 2, 1 as in k_voc_transform)
__device__ __forceinline__ uint32_t row16_min(uint32_t v) {
    v = min(v, dpp_u32<0x128>(v));
    v = min(v, dpp_u32<0x124>(v));
    v = min(v, dpp_u32<0x122>(v));
    v = min(v, dpp_u32<0x121>(v));
    return v;
}

// For four words at once, the number of entries of the ascending s[0 .. n - 1] below each: a branch-free descent of a fixed number of steps (top = the
// largest power of two <= n), so that the four chains of dependent LDS reads overlap instead of queueing behind each other.
__device__ __forceinline__ void lower_bound4(const uint32_t* s, int n, int top, const uint32_t (&w)[4], int (&lo)[4]) {
#pragma unroll
    for (int u = 0; u < 4; u++) lo[u] = 0;
    for (int st = top; st > 0; st >>= 1) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int m = lo[u] + st;
            if (m <= n && s[m - 1] < w[u]) lo[u] = m;
        }
    }
}

constexpr uint8_t kConn = 1, kScored = 2;

__global__ __launch_bounds__(kThreads) void k_kfdb_query(QueryArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const oslam_kfdb_query_t Q = a.q[b];
    const int K = a.st.K, MW = a.st.MW, MC = a.st.MC;
    const bool loop = a.loop != 0, derive = loop && a.min_score != nullptr;
    const int nq = Q.n_words, ncn = loop ? Q.n_conn : 0;

    extern __shared__ __align__(16) uint8_t smem[];
    double* s_qv = (double*)smem;                                         // [MW] the query's values
    unsigned long long* s_key = (unsigned long long*)(s_qv + MW);         // [P] (smallest common word << 32) | add serial
    uint32_t* s_qi = (uint32_t*)(s_key + a.P);                            // [MW] the query's word ids
    int* s_ent = (int*)(s_qi + MW);                                       // [P] the slot of an entry
    int* s_words = s_ent + a.P;                                           // [K] common words; -1: the slot is not present
    uint32_t* s_minw = (uint32_t*)(s_words + K);                          // [K] smallest common word
    float* s_score = (float*)(s_minw + K);                                // [K] si
    float* s_acc = s_score + K;                                           // [K] accScore of entry e
    int* s_best = (int*)(s_acc + K);                                      // [K] pBestKF of entry e
    int* s_first = s_best + K;                                            // [K] first retained entry whose pBestKF is the slot
    uint8_t* s_flag = (uint8_t*)(s_first + K);                            // [K] kConn | kScored
    __shared__ int s_bad, s_max, s_nshare, s_nscore, s_m, s_minkey;
    __shared__ float s_red[kThreads];

    // ---- the record, the query vector ----
    bool ok = Q.database >= 0 && Q.database < a.st.n_db && nq >= 0 && nq <= MW && Q.word_off >= 0 && Q.word_off <= a.n_words_total - nq;
    if (loop) ok = ok && ncn >= 0 && Q.conn_off >= 0 && Q.conn_off <= a.n_conn_total - ncn;
    if (tid == 0) { s_bad = ok ? 0 : 1; s_max = 0; s_nshare = 0; s_nscore = 0; s_m = 0; s_minkey = 0x3f800000; }   // (the bits of 1.0f)
    __syncthreads();
    if (ok) {
        for (int i = tid; i < a.n_q; i += kThreads)
            if (i != b && a.q[i].database == Q.database) s_bad = 1;   // two queries on one database: both are refused
        const uint32_t* gi = a.ids + Q.word_off;
        const double* gv = a.vals + Q.word_off;
        for (int i = tid; i < nq; i += kThreads) {
            const uint32_t w = gi[i];
            s_qi[i] = w; s_qv[i] = gv[i];
            if (i > 0 && gi[i - 1] >= w) s_bad = 1;   // not strictly ascending
        }
        for (int k = tid; k < K; k += kThreads) { s_flag[k] = 0; s_first[k] = INT_MAX; }
    }
    __syncthreads();
    if (s_bad) {   // (uniform)
        if (tid == 0) a.n_cand[b] = -2;
        return;
    }
    for (int j = tid; j < ncn; j += kThreads) {
        const int id = a.conn[Q.conn_off + j];
        if (id >= 0 && id < K) s_flag[id] = kConn;
    }
    __syncthreads();

    // ---- count pass: word ids only.  Group g of 16 lanes takes slots g, g + 32, ...; the lane exchanges are outside every divergent branch ----
    const size_t base = (size_t)Q.database * K;
    const int g = tid / kGroup, c = tid % kGroup;
    int top = 1;   // the largest power of two <= nq (nq <= 2400; not used for an empty query)
    while (2 * top <= nq) top *= 2;
    for (int s0 = 0; s0 < K; s0 += kGroups) {
        const int slot = s0 + g;
        const int nw = slot < K ? a.st.nwords[base + slot] : -1;
        int cnt = 0;
        uint32_t mn = 0xffffffffu;
        if (nw > 0 && nq > 0) {
            const int32_t* ch = a.st.chunks + (base + slot) * MC;
            for (int c0 = 0; c0 < nw; c0 += kChunk) {
                const uint32_t* p = a.st.pool_ids + (size_t)ch[c0 / kChunk] * kChunk;
                const int m = min(kChunk, nw - c0);
                for (int o = c; o < m; o += 4 * kGroup) {
                    uint32_t w[4];
                    int lo[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) w[u] = o + u * kGroup < m ? p[o + u * kGroup] : 0xffffffffu;
                    lower_bound4(s_qi, nq, top, w, lo);
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        if (o + u * kGroup < m && lo[u] < nq && s_qi[lo[u]] == w[u]) { cnt++; mn = min(mn, w[u]); }
                }
            }
        }
        cnt = oslam::row16_sum_i32(cnt);
        mn = row16_min(mn);
        if (c == 0 && slot < K) { s_words[slot] = nw >= 0 ? cnt : -1; s_minw[slot] = mn; }
    }
    __syncthreads();

    // ---- lKFsSharingWords.size() and maxCommonWords (integers: any order) ----
    {
        int lmax = 0, ln = 0;
        for (int k = tid; k < K; k += kThreads)
            if (s_words[k] > 0 && !(s_flag[k] & kConn)) { ln++; lmax = max(lmax, s_words[k]); }
        if (ln) { atomicAdd(&s_nshare, ln); atomicMax(&s_max, lmax); }
    }
    __syncthreads();
    const int maxCommon = s_max, minCommon = (int)((float)maxCommon * 0.8f);

    // ---- score pass: the values of the survivors and of the connected ids that are present ----
    for (int s0 = 0; s0 < K; s0 += kGroups) {
        const int slot = s0 + g;
        const int w = slot < K ? s_words[slot] : -1;
        const bool cn = slot < K && (s_flag[slot] & kConn);
        const bool scored = !cn && w > 0 && w > minCommon;
        const bool need = scored || (cn && w >= 0);
        double sum = 0.0;
        if (need && w > 0) {
            const int nw = a.st.nwords[base + slot];
            const int32_t* ch = a.st.chunks + (base + slot) * MC;
            for (int c0 = 0; c0 < nw; c0 += kChunk) {
                const size_t at = (size_t)ch[c0 / kChunk] * kChunk;
                const int m = min(kChunk, nw - c0);
                for (int o = c; o < m; o += 4 * kGroup) {
                    uint32_t ww[4];
                    int lo[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) ww[u] = o + u * kGroup < m ? a.st.pool_ids[at + o + u * kGroup] : 0xffffffffu;
                    lower_bound4(s_qi, nq, top, ww, lo);
#pragma unroll
                    for (int u = 0; u < 4; u++)   // (ascending position: the order of the sum is that of one word at a time)
                        if (o + u * kGroup < m && lo[u] < nq && s_qi[lo[u]] == ww[u]) {
                            const double va = s_qv[lo[u]], vb = a.st.pool_vals[at + o + u * kGroup];
                            sum += fabs(va - vb) - fabs(va) - fabs(vb);
                        }
                }
            }
        }
        sum = oslam::row16_sum(sum);
        if (c == 0 && need) {
            const float si = (float)(-sum / 2.0);
            s_score[slot] = si;
            if (scored) {
                s_flag[slot] = kScored;
                if (!loop) a.st.reloc[base + slot] = si;   // pKFi->mRelocScore = si (:250)
            }
        }
    }
    __syncthreads();
    for (int j = tid; j < ncn; j += kThreads) {
        const int id = a.conn[Q.conn_off + j];
        const bool present = id >= 0 && id < K && s_words[id] >= 0;
        a.conn_score[Q.conn_off + j] = present ? s_score[id] : -1.0f;
        if (derive && present) {   // an integer minimum over keys that order as the floats do (-0 below +0): exact, in any order
            const int bits = __float_as_int(s_score[id]);
            atomicMin(&s_minkey, bits < 0 ? bits ^ 0x7fffffff : bits);
        }
    }
    float minScore = Q.min_score;
    if (derive) {   // (uniform) minScore = min(1, the scores of the connected keyframes that are present) (src/LoopClosing.cc:127-139)
        __syncthreads();
        const int key = s_minkey;
        minScore = __int_as_float(key < 0 ? key ^ 0x7fffffff : key);
        if (tid == 0) a.min_score[b] = minScore;
    }

    // ---- lScoreAndMatch: the scored keyframes (loop: with si >= minScore), then sorted by (smallest common word, add serial) ----
    {
        int ln = 0;
        for (int k = tid; k < K; k += kThreads) {
            if (!(s_flag[k] & kScored)) continue;
            ln++;
            if (loop && !(s_score[k] >= minScore)) continue;
            const int pos = atomicAdd(&s_m, 1);   // (any position: the sort below orders the entries, and their keys differ)
            s_key[pos] = ((unsigned long long)s_minw[k] << 32) | a.st.serial[base + k];
            s_ent[pos] = k;
        }
        if (ln) atomicAdd(&s_nscore, ln);
    }
    __syncthreads();
    const int M = s_m;
    int P2 = 1;
    while (P2 < M) P2 <<= 1;
    for (int i = M + tid; i < P2; i += kThreads) { s_key[i] = ~0ull; s_ent[i] = -1; }
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P2; i += kThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long ki = s_key[i], kl = s_key[l];
                    if ((ki > kl) == ((i & k) == 0)) {
                        s_key[i] = kl; s_key[l] = ki;
                        const int t = s_ent[i]; s_ent[i] = s_ent[l]; s_ent[l] = t;
                    }
                }
            }
            __syncthreads();
        }

    // ---- accumulate by covisibility (:148-173, :262-287) ----
    float lbest = loop ? minScore : 0.0f;   // bestAccScore
    for (int e = tid; e < M; e += kThreads) {
        const int slot = s_ent[e];
        float bestScore = s_score[slot], acc = bestScore;
        int bk = slot;
        const int32_t* nb = a.st.covis + (base + slot) * kCovis;
        for (int n = 0; n < kCovis; n++) {
            const int id = nb[n];
            if (id < 0 || id >= K) continue;
            const uint8_t f = s_flag[id];
            float sc;
            if (loop) {
                if (!(f & kScored)) continue;
                sc = s_score[id];
            } else {
                if (!(s_words[id] > 0)) continue;   // pKF2->mnRelocQuery != F->mnId (:273)
                sc = (f & kScored) ? s_score[id] : a.st.reloc[base + id];   // not scored by this query: what an earlier one left (no query of this launch writes it)
            }
            acc += sc;
            if (sc > bestScore) { bk = id; bestScore = sc; }
        }
        s_acc[e] = acc; s_best[e] = bk;
        if (acc > lbest) lbest = acc;
    }
    s_red[tid] = lbest;
    __syncthreads();
    for (int d = kThreads / 2; d > 0; d >>= 1) {
        if (tid < d) { const float o = s_red[tid + d]; if (o > s_red[tid]) s_red[tid] = o; }
        __syncthreads();
    }
    const float retain = 0.75f * s_red[0];
    for (int e = tid; e < M; e += kThreads)
        if (s_acc[e] > retain) atomicMin(&s_first[s_best[e]], e);
    __syncthreads();
    // ---- output in list order, the first occurrence of every pBestKF: one wavefront compacts 64 entries at a time ----
    if (tid < 64) {
        int nout = 0;
        for (int e0 = 0; e0 < M; e0 += 64) {
            const int e = e0 + tid;
            const bool keep = e < M && s_acc[e] > retain && s_first[s_best[e]] == e;
            const unsigned long long mask = __ballot(keep);
            if (keep) {
                const int pos = nout + __popcll(mask & ((1ull << tid) - 1ull));
                a.cand[(size_t)b * K + pos] = s_best[e];
                a.cand_acc[(size_t)b * K + pos] = s_acc[e];
            }
            nout += __popcll(mask);
        }
        if (tid == 0) {
            a.n_cand[b] = nout;
            int32_t* dg = a.diag + (size_t)b * 5;
            dg[0] = s_nshare; dg[1] = maxCommon; dg[2] = minCommon; dg[3] = s_nscore; dg[4] = M;
        }
    }
}

int check_l1(const char* fn, const oslam_voc_t* voc) {
    if (!voc) { set_error("%s: NULL vocabulary", fn); return OSLAM_E_INVALID; }
    int32_t info[8];
    OSLAM_CHECK(oslam_voc_info(voc, info));
    if (info[2] != 0) {
        set_error("%s: only L1_NORM (scoring 0, the reference vocabulary's) is implemented; this vocabulary has scoring %d", fn, info[2]);
        return OSLAM_E_INVALID;
    }
    return OSLAM_OK;
}

}  // namespace

int oslam::kfdb_check_query_call(const char* fn, const oslam_kfdb* h, const oslam_voc_t* voc, int n_queries, int n_words_total, int n_conn_total) {
    if (!h) { set_error("%s: NULL handle", fn); return OSLAM_E_INVALID; }
    OSLAM_CHECK(check_l1(fn, voc));
    if (n_queries < 0 || n_words_total < 0 || n_conn_total < 0) { set_error("%s: a count is negative", fn); return OSLAM_E_INVALID; }
    if (n_queries > h->st.n_db) { set_error("%s: %d queries for %d databases (one query per database and call)", fn, n_queries, h->st.n_db); return OSLAM_E_INVALID; }
    return OSLAM_OK;
}

int oslam::kfdb_launch_query(oslam_kfdb* h, bool loop, int n_queries, const oslam_kfdb_query_t* d_queries, int n_words_total, const uint32_t* d_ids, const double* d_vals,
                             int n_conn_total, const int32_t* d_conn, int32_t* d_cand, float* d_cand_acc, int32_t* d_n_cand, int32_t* d_diag, float* d_conn_score,
                             float* d_min_score, hipStream_t stream) {
    QueryArgs a;
    a.st = h->st; a.q = d_queries; a.n_q = n_queries; a.n_words_total = n_words_total; a.n_conn_total = n_conn_total; a.loop = loop ? 1 : 0; a.P = h->P;
    a.ids = d_ids; a.vals = d_vals; a.conn = d_conn; a.cand = d_cand; a.cand_acc = d_cand_acc; a.n_cand = d_n_cand; a.diag = d_diag; a.conn_score = d_conn_score; a.min_score = d_min_score;
    hipLaunchKernelGGL(k_kfdb_query, dim3(n_queries), dim3(kThreads), h->lds, stream, a);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int oslam::kfdb_check_queries(const char* fn, const oslam_kfdb* h, bool loop, int n_queries, const oslam_kfdb_query_t* queries, int n_words_total, const uint32_t* ids,
                              int n_conn_total) {
    std::vector<uint8_t> seen(h->st.n_db, 0);
    for (int q = 0; q < n_queries; q++) {
        const oslam_kfdb_query_t& Q = queries[q];
        if (Q.database < 0 || Q.database >= h->st.n_db) { set_error("%s: query %d names database %d of %d", fn, q, Q.database, h->st.n_db); return OSLAM_E_INVALID; }
        if (seen[Q.database]) { set_error("%s: query %d is the second on database %d in this call (queries on one database are sequential)", fn, q, Q.database); return OSLAM_E_INVALID; }
        seen[Q.database] = 1;
        if (Q.n_words > h->st.MW) { set_error("%s: query %d has %d words, the handle holds %d", fn, q, Q.n_words, h->st.MW); return OSLAM_E_CAPACITY; }
        if (Q.n_words < 0 || Q.word_off < 0 || Q.word_off > n_words_total - Q.n_words) { set_error("%s: query %d's words lie outside the %d given", fn, q, n_words_total); return OSLAM_E_INVALID; }
        if (loop && (Q.n_conn < 0 || Q.conn_off < 0 || Q.conn_off > n_conn_total - Q.n_conn)) { set_error("%s: query %d's connected ids lie outside the %d given", fn, q, n_conn_total); return OSLAM_E_INVALID; }
        for (int i = 1; i < Q.n_words; i++)
            if (ids[Q.word_off + i - 1] >= ids[Q.word_off + i]) { set_error("%s: query %d's word ids are not strictly ascending at %d", fn, q, i); return OSLAM_E_INVALID; }
    }
    return OSLAM_OK;
}

namespace {

using oslam::kfdb_check_query_call;

int query_device(const char* fn, oslam_kfdb* h, const oslam_voc_t* voc, bool loop, int n_queries, const oslam_kfdb_query_t* d_queries, int n_words_total, const uint32_t* d_ids,
                 const double* d_vals, int n_conn_total, const int32_t* d_conn, int32_t* d_cand, float* d_cand_acc, int32_t* d_n_cand, int32_t* d_diag, float* d_conn_score,
                 void* stream) {
    OSLAM_CHECK(kfdb_check_query_call(fn, h, voc, n_queries, n_words_total, n_conn_total));
    if (n_queries == 0) return OSLAM_OK;
    if (!d_queries || !d_cand || !d_cand_acc || !d_n_cand || !d_diag || (n_words_total > 0 && (!d_ids || !d_vals)) || (loop && n_conn_total > 0 && (!d_conn || !d_conn_score))) {
        set_error("%s: NULL argument", fn);
        return OSLAM_E_INVALID;
    }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    return oslam::kfdb_launch_query(h, loop, n_queries, d_queries, n_words_total, d_ids, d_vals, n_conn_total, d_conn, d_cand, d_cand_acc, d_n_cand, d_diag, d_conn_score, nullptr,
                                    (hipStream_t)stream);
}

int query_host(const char* fn, oslam_kfdb* h, const oslam_voc_t* voc, bool loop, int n_queries, const oslam_kfdb_query_t* queries, int n_words_total, const uint32_t* ids,
               const double* vals, int n_conn_total, const int32_t* conn, int32_t* cand, float* cand_acc, int32_t* n_cand, int32_t* diag, float* conn_score) {
    OSLAM_CHECK(kfdb_check_query_call(fn, h, voc, n_queries, n_words_total, n_conn_total));
    if (n_queries == 0) return OSLAM_OK;
    if (!queries || !cand || !cand_acc || !n_cand || !diag || (n_words_total > 0 && (!ids || !vals)) || (loop && n_conn_total > 0 && (!conn || !conn_score))) {
        set_error("%s: NULL argument", fn);
        return OSLAM_E_INVALID;
    }
    std::lock_guard<std::mutex> lock(h->mu);
    const int K = h->st.K;
    OSLAM_CHECK(oslam::kfdb_check_queries(fn, h, loop, n_queries, queries, n_words_total, ids, n_conn_total));
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t nq = (size_t)n_queries, W = (size_t)n_words_total, NC = loop ? (size_t)n_conn_total : 0;
    oslam::StageLayout lay;   // one block, inputs then outputs: one upload, one download
    const auto fQ = lay.add<oslam_kfdb_query_t>(nq);
    const auto fIds = lay.add<uint32_t>(W);
    const auto fVals = lay.add<double>(W);
    const auto fConn = lay.add<int32_t>(NC);
    const auto fCand = lay.add<int32_t>(nq * K);
    const auto fAcc = lay.add<float>(nq * K);
    const auto fN = lay.add<int32_t>(nq), fDiag = lay.add<int32_t>(nq * 5);
    const auto fCs = lay.add<float>(NC);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fQ, ph, queries); put(fIds, ph, ids); put(fVals, ph, vals); put(fConn, ph, conn);
    // the caller's output rows travel too: what the kernel does not write comes back as it was
    put(fCand, ph, cand); put(fAcc, ph, cand_acc); put(fN, ph, n_cand); put(fDiag, ph, diag); put(fCs, ph, conn_score);
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, h->stream));
    OSLAM_CHECK(oslam::kfdb_launch_query(h, loop, n_queries, at(fQ, pd), n_words_total, at(fIds, pd), at(fVals, pd), (int)NC, at(fConn, pd), at(fCand, pd), at(fAcc, pd),
                                         at(fN, pd), at(fDiag, pd), at(fCs, pd), nullptr, h->stream));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fCand.off, pd + fCand.off, lay.total() - fCand.off, hipMemcpyDeviceToHost, h->stream));
    OSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    get(fCand, ph, cand); get(fAcc, ph, cand_acc); get(fN, ph, n_cand); get(fDiag, ph, diag); get(fCs, ph, conn_score);
    return OSLAM_OK;
}

void free_slot(oslam_kfdb* h, size_t slot) {
    const int nw = h->h_nwords[slot];
    if (nw < 0) return;
    for (int i = 0; i < oslam::div_up(nw, kChunk); i++) h->free_chunks.push_back(h->h_chunks[slot * h->st.MC + i]);
    h->h_nwords[slot] = -1;
    h->n_present--;
}

// the first `bytes` of the staging block to its device mirror, on the handle's stream (the caller enqueues its kernel behind it and waits)
int stage_up(oslam_kfdb* h, size_t bytes) {
    OSLAM_HIP_CHECK(hipMemcpyAsync(h->io.d.bytes(), h->io.h.bytes(), bytes, hipMemcpyHostToDevice, h->stream));
    return OSLAM_OK;
}

}  // namespace

extern "C" {

void oslam_kfdb_destroy(oslam_kfdb_t* h) {
    if (!h) return;
    delete h;
}

int oslam_kfdb_create(oslam_kfdb_t** out, int n_databases, int max_keyframes, int max_words, long long pool_words, int device) {
    const char* fn = "oslam_kfdb_create";
    if (!out) { set_error("%s: out is NULL", fn); return OSLAM_E_INVALID; }
    *out = nullptr;
    if (n_databases < 1 || max_keyframes < 1 || max_words < 1 || pool_words < 1) { set_error("%s: bad argument", fn); return OSLAM_E_INVALID; }
    if (max_keyframes > OSLAM_KFDB_MAX_KEYFRAMES || max_words > OSLAM_KFDB_MAX_WORDS) {
        set_error("%s: max_keyframes %d > %d or max_words %d > %d (the query vector and the per-slot scratch of a query live in LDS)", fn, max_keyframes, OSLAM_KFDB_MAX_KEYFRAMES,
                  max_words, OSLAM_KFDB_MAX_WORDS);
        return OSLAM_E_INVALID;
    }
    const long long S = (long long)n_databases * max_keyframes, n_chunks = (pool_words + kChunk - 1) / kChunk;
    if (S > (1ll << 28) || n_chunks > (1ll << 24)) { set_error("%s: %lld slots or %lld chunks are more than the handle's index types hold", fn, S, n_chunks); return OSLAM_E_INVALID; }
    const int ndev = oslam_device_count();
    if (ndev <= 0) return oslam::no_device(fn);
    if (device < 0 || device >= ndev) { set_error("%s: device out of range", fn); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(device));
    oslam_kfdb* h = new oslam_kfdb;
    h->device = device;
    const int MC = oslam::div_up(max_words, kChunk);
    int P = 1;
    while (P < max_keyframes) P <<= 1;
    h->P = P;
    h->lds = lds_bytes(max_keyframes, max_words, P);
    h->n_chunks = n_chunks;
    int rc = OSLAM_OK;
    if ((rc = h->nwords.alloc((size_t)S * 4)) || (rc = h->serial.alloc((size_t)S * 4)) || (rc = h->reloc.alloc((size_t)S * 4)) || (rc = h->covis.alloc((size_t)S * kCovis * 4)) ||
        (rc = h->chunks.alloc((size_t)S * MC * 4)) || (rc = h->pool_ids.alloc((size_t)n_chunks * kChunk * 4)) || (rc = h->pool_vals.alloc((size_t)n_chunks * kChunk * 8))) {
        delete h;
        return rc;
    }
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMemsetAsync(h->nwords.ptr(), 0xff, (size_t)S * 4, h->stream);   // -1: not present
    if (e == hipSuccess) e = hipMemsetAsync(h->serial.ptr(), 0, (size_t)S * 4, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->reloc.ptr(), 0, (size_t)S * 4, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->covis.ptr(), 0xff, (size_t)S * kCovis * 4, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->chunks.ptr(), 0, (size_t)S * MC * 4, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->pool_ids.ptr(), 0, (size_t)n_chunks * kChunk * 4, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->pool_vals.ptr(), 0, (size_t)n_chunks * kChunk * 8, h->stream);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_kfdb_query, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lds_bytes(OSLAM_KFDB_MAX_KEYFRAMES, OSLAM_KFDB_MAX_WORDS, OSLAM_KFDB_MAX_KEYFRAMES));   // (the attribute belongs to the kernel)
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        set_error("%s: %s", fn, hipGetErrorString(e));
        delete h;
        return OSLAM_E_HIP;
    }
    h->st = KfdbState{h->nwords.as<int32_t>(), h->serial.as<uint32_t>(), h->reloc.as<float>(), h->covis.as<int32_t>(), h->chunks.as<int32_t>(), h->pool_ids.as<uint32_t>(),
                      h->pool_vals.as<double>(), n_databases, max_keyframes, max_words, MC};
    h->h_nwords.assign((size_t)S, -1);
    h->h_chunks.assign((size_t)S * MC, 0);
    h->next_serial.assign(n_databases, 0);
    h->free_chunks.resize((size_t)n_chunks);
    for (long long i = 0; i < n_chunks; i++) h->free_chunks[i] = (int32_t)(n_chunks - 1 - i);   // (taken from the back: chunk 0 first)
    *out = h;
    return OSLAM_OK;
}

int oslam_kfdb_info(const oslam_kfdb_t* h, int64_t out[3]) {
    if (!h || !out) { set_error("oslam_kfdb_info: NULL argument"); return OSLAM_E_INVALID; }
    out[0] = (int64_t)h->free_chunks.size(); out[1] = h->n_chunks; out[2] = h->n_present;
    return OSLAM_OK;
}

int oslam_kfdb_add(oslam_kfdb_t* h, int n, const oslam_kfdb_add_t* recs, int n_words_total, const uint32_t* ids, const double* vals) {
    const char* fn = "oslam_kfdb_add";
    if (!h || n < 0 || n_words_total < 0 || (n > 0 && !recs) || (n_words_total > 0 && (!ids || !vals))) { set_error("%s: bad argument", fn); return OSLAM_E_INVALID; }
    if (n == 0) return OSLAM_OK;
    std::lock_guard<std::mutex> lock(h->mu);
    const int K = h->st.K, MC = h->st.MC;
    // the whole call is checked against the host's side of the state before any of it is applied
    size_t need = 0;
    std::vector<size_t> slots(n);
    for (int r = 0; r < n; r++) {
        const oslam_kfdb_add_t& A = recs[r];
        if (A.database < 0 || A.database >= h->st.n_db || A.keyframe < 0) { set_error("%s: record %d names database %d, keyframe %d", fn, r, A.database, A.keyframe); return OSLAM_E_INVALID; }
        if (A.keyframe >= K) { set_error("%s: record %d: keyframe %d, a database holds %d", fn, r, A.keyframe, K); return OSLAM_E_CAPACITY; }
        if (A.n_words > h->st.MW) { set_error("%s: record %d has %d words, a keyframe holds %d", fn, r, A.n_words, h->st.MW); return OSLAM_E_CAPACITY; }
        if (A.n_words < 0 || A.word_off < 0 || A.word_off > n_words_total - A.n_words) { set_error("%s: record %d's words lie outside the %d given", fn, r, n_words_total); return OSLAM_E_INVALID; }
        for (int i = 1; i < A.n_words; i++)
            if (ids[A.word_off + i - 1] >= ids[A.word_off + i]) { set_error("%s: record %d's word ids are not strictly ascending at %d", fn, r, i); return OSLAM_E_INVALID; }
        slots[r] = (size_t)A.database * K + A.keyframe;
        if (h->h_nwords[slots[r]] >= 0) { set_error("%s: record %d: keyframe %d of database %d is present already", fn, r, A.keyframe, A.database); return OSLAM_E_INVALID; }
        need += (size_t)oslam::div_up(A.n_words, kChunk);
    }
    {
        std::vector<size_t> sorted(slots);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) { set_error("%s: a keyframe is named twice in the call", fn); return OSLAM_E_INVALID; }
    }
    if (need > h->free_chunks.size()) {
        set_error("%s: the call needs %zu chunks of %d words, the pool has %zu free of %lld", fn, need, kChunk, h->free_chunks.size(), h->n_chunks);
        return OSLAM_E_CAPACITY;
    }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    oslam::StageLayout lay;
    const auto fRec = lay.add<AddRec>((size_t)n);
    const auto fIds = lay.add<uint32_t>((size_t)n_words_total);
    const auto fVals = lay.add<double>((size_t)n_words_total);
    const auto fCh = lay.add<int32_t>(need);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));   // (fails before the state changes)
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    AddRec* ar = at(fRec, ph);
    int32_t* cl = at(fCh, ph);
    int32_t at_chunk = 0;
    for (int r = 0; r < n; r++) {
        const oslam_kfdb_add_t& A = recs[r];
        const int nc = oslam::div_up(A.n_words, kChunk);
        ar[r] = AddRec{(int32_t)slots[r], A.n_words, A.word_off, at_chunk, h->next_serial[A.database]++};
        for (int i = 0; i < nc; i++) {
            const int32_t ck = h->free_chunks.back();
            h->free_chunks.pop_back();
            cl[at_chunk + i] = ck;
            h->h_chunks[slots[r] * MC + i] = ck;
        }
        at_chunk += nc;
        h->h_nwords[slots[r]] = A.n_words;
        h->n_present++;
    }
    put(fIds, ph, ids); put(fVals, ph, vals);
    OSLAM_CHECK(stage_up(h, lay.total()));
    hipLaunchKernelGGL(k_kfdb_add, dim3(n), dim3(kMutThreads), 0, h->stream, h->st, at(fRec, pd), at(fIds, pd), at(fVals, pd), at(fCh, pd));
    OSLAM_HIP_CHECK(hipGetLastError());
    OSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    return OSLAM_OK;
}

static int erase_records(oslam_kfdb* h, int n, const oslam_kfdb_key_t* recs) {   // (checked by the callers; keyframe -1: the whole database)
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    oslam::StageLayout lay;
    const auto fRec = lay.add<oslam_kfdb_key_t>((size_t)n);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    put(fRec, h->io.h.bytes(), recs);
    const int K = h->st.K;
    for (int r = 0; r < n; r++) {
        const size_t base = (size_t)recs[r].database * K;
        if (recs[r].keyframe >= 0) free_slot(h, base + recs[r].keyframe);
        else for (int k = 0; k < K; k++) free_slot(h, base + k);
    }
    OSLAM_CHECK(stage_up(h, lay.total()));
    hipLaunchKernelGGL(k_kfdb_erase, dim3(n), dim3(kMutThreads), 0, h->stream, h->st, at(fRec, h->io.d.bytes()));
    OSLAM_HIP_CHECK(hipGetLastError());
    OSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    return OSLAM_OK;
}

int oslam_kfdb_erase(oslam_kfdb_t* h, int n, const oslam_kfdb_key_t* recs) {
    const char* fn = "oslam_kfdb_erase";
    if (!h || n < 0 || (n > 0 && !recs)) { set_error("%s: bad argument", fn); return OSLAM_E_INVALID; }
    if (n == 0) return OSLAM_OK;
    std::lock_guard<std::mutex> lock(h->mu);
    for (int r = 0; r < n; r++)
        if (recs[r].database < 0 || recs[r].database >= h->st.n_db || recs[r].keyframe < 0 || recs[r].keyframe >= h->st.K) {
            set_error("%s: record %d names database %d, keyframe %d", fn, r, recs[r].database, recs[r].keyframe);
            return OSLAM_E_INVALID;
        }
    return erase_records(h, n, recs);
}

int oslam_kfdb_clear(oslam_kfdb_t* h, int n, const int32_t* databases) {
    const char* fn = "oslam_kfdb_clear";
    if (!h || n < 0 || (n > 0 && !databases)) { set_error("%s: bad argument", fn); return OSLAM_E_INVALID; }
    if (n == 0) return OSLAM_OK;
    std::lock_guard<std::mutex> lock(h->mu);
    std::vector<oslam_kfdb_key_t> recs(n);
    for (int r = 0; r < n; r++) {
        if (databases[r] < 0 || databases[r] >= h->st.n_db) { set_error("%s: record %d names database %d of %d", fn, r, databases[r], h->st.n_db); return OSLAM_E_INVALID; }
        recs[r] = oslam_kfdb_key_t{databases[r], -1};
    }
    return erase_records(h, n, recs.data());
}

int oslam_kfdb_set_covisibility(oslam_kfdb_t* h, int n, const oslam_kfdb_covis_t* recs) {
    const char* fn = "oslam_kfdb_set_covisibility";
    if (!h || n < 0 || (n > 0 && !recs)) { set_error("%s: bad argument", fn); return OSLAM_E_INVALID; }
    if (n == 0) return OSLAM_OK;
    std::lock_guard<std::mutex> lock(h->mu);
    for (int r = 0; r < n; r++) {
        const oslam_kfdb_covis_t& c = recs[r];
        if (c.database < 0 || c.database >= h->st.n_db || c.keyframe < 0 || c.keyframe >= h->st.K || c.n < 0 || c.n > kCovis) {
            set_error("%s: record %d names database %d, keyframe %d, %d ids", fn, r, c.database, c.keyframe, c.n);
            return OSLAM_E_INVALID;
        }
        if (h->h_nwords[(size_t)c.database * h->st.K + c.keyframe] < 0) { set_error("%s: record %d: keyframe %d of database %d is not present", fn, r, c.keyframe, c.database); return OSLAM_E_INVALID; }
    }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    oslam::StageLayout lay;
    const auto fRec = lay.add<oslam_kfdb_covis_t>((size_t)n);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    put(fRec, h->io.h.bytes(), recs);
    OSLAM_CHECK(stage_up(h, lay.total()));
    hipLaunchKernelGGL(k_kfdb_covis, dim3(1), dim3(64), 0, h->stream, h->st, at(fRec, h->io.d.bytes()), n);
    OSLAM_HIP_CHECK(hipGetLastError());
    OSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    return OSLAM_OK;
}

int oslam_kfdb_detect_loop_candidates(oslam_kfdb_t* h, const oslam_voc_t* voc, int n_queries, const oslam_kfdb_query_t* queries, int n_words_total, const uint32_t* ids,
                                      const double* vals, int n_conn_total, const int32_t* conn, int32_t* cand, float* cand_acc, int32_t* n_cand, int32_t* diag,
                                      float* conn_score) {
    return query_host("oslam_kfdb_detect_loop_candidates", h, voc, true, n_queries, queries, n_words_total, ids, vals, n_conn_total, conn, cand, cand_acc, n_cand, diag, conn_score);
}

int oslam_kfdb_detect_relocalization_candidates(oslam_kfdb_t* h, const oslam_voc_t* voc, int n_queries, const oslam_kfdb_query_t* queries, int n_words_total,
                                                const uint32_t* ids, const double* vals, int32_t* cand, float* cand_acc, int32_t* n_cand, int32_t* diag) {
    return query_host("oslam_kfdb_detect_relocalization_candidates", h, voc, false, n_queries, queries, n_words_total, ids, vals, 0, nullptr, cand, cand_acc, n_cand, diag, nullptr);
}

int oslam_kfdb_detect_loop_candidates_device(oslam_kfdb_t* h, const oslam_voc_t* voc, int n_queries, const oslam_kfdb_query_t* d_queries, int n_words_total,
                                             const uint32_t* d_ids, const double* d_vals, int n_conn_total, const int32_t* d_conn, int32_t* d_cand, float* d_cand_acc,
                                             int32_t* d_n_cand, int32_t* d_diag, float* d_conn_score, void* stream) {
    return query_device("oslam_kfdb_detect_loop_candidates_device", h, voc, true, n_queries, d_queries, n_words_total, d_ids, d_vals, n_conn_total, d_conn, d_cand, d_cand_acc,
                        d_n_cand, d_diag, d_conn_score, stream);
}

int oslam_kfdb_detect_relocalization_candidates_device(oslam_kfdb_t* h, const oslam_voc_t* voc, int n_queries, const oslam_kfdb_query_t* d_queries, int n_words_total,
                                                       const uint32_t* d_ids, const double* d_vals, int32_t* d_cand, float* d_cand_acc, int32_t* d_n_cand,
                                                       int32_t* d_diag, void* stream) {
    return query_device("oslam_kfdb_detect_relocalization_candidates_device", h, voc, false, n_queries, d_queries, n_words_total, d_ids, d_vals, 0, nullptr, d_cand, d_cand_acc,
                        d_n_cand, d_diag, nullptr, stream);
}

}  // extern "C"
