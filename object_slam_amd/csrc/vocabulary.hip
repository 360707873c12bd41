// vocabulary.hip — DBoW2 ORB vocabulary (TemplatedVocabulary<FORB::TDescriptor, FORB> as the ORB-SLAM2 fork loads it with loadFromTextFile):
// text loader, host descent, BowVector / FeatureVector assembly, L1 score, and the gfx950 kernel that transforms batches of descriptors
// (include/oslam_hip.h, "ORB vocabulary").  DBoW2 itself is not in the reference tree: format and algorithms are restated from its published
// source; parity with DBoW2 is not pinned by any test.  Product code; never includes oracle/.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "common.h"

using oslam::set_error;

// Nodes are kept in PACKED order: index 0 = the root, then breadth first, the children of a node next to each other in file order.  One descent
// step therefore reads one run of (children x 32) bytes, and the top levels of the tree are the first entries of every array.
struct oslam_voc {
    int k = 0, L = 0, scoring = 0, weighting = 0;
    int n = 0;            // nodes without the root (= node lines of the file); file node ids are 1 .. n
    int n_words = 0, max_depth = 0, max_children = 0;
    // by file node id - 1 (what was read)
    std::vector<int32_t> parent; std::vector<uint8_t> leaf; std::vector<uint8_t> desc; std::vector<double> weight; std::vector<int32_t> word;
    // by packed index, n + 1 entries
    std::vector<uint8_t> p_desc;      // [n + 1][32]
    std::vector<uint2> p_link;        // (packed index of the first child, number of children); 0 children = leaf
    std::vector<uint2> p_ids;         // (file node id, word id or 0xffffffff)
    std::vector<double> p_weight;
    // device images, one per device that asked
    struct Image { uint8_t* desc = nullptr; uint2* link = nullptr; uint2* ids = nullptr; double* weight = nullptr; };   // what voc_image hands out, by value
    struct ImageMem {   // the arrays behind an Image: they live as long as the vocabulary
        oslam::DeviceBuffer desc, link, ids, weight;
        Image view() const { return {desc.bytes(), link.as<uint2>(), ids.as<uint2>(), weight.as<double>()}; }
    };
    mutable std::mutex mu, mu_scratch;
    mutable std::map<int, oslam::DeviceBuffer> scratch;   // staging of the host-pointer entry point (oslam_voc_transform), one per device
    mutable std::map<int, ImageMem> images;
};

namespace {

constexpr int kVocLdsNodes = 1111;   // root + the three top levels of a full k = 10 tree: 35.5 KB of centres + 8.9 KB of links in LDS
constexpr int kVocThreads = 512, kVocGroup = 16, kVocDescPerBlock = 256;

struct VocImg { const uint8_t* desc; const uint2* link; const uint2* ids; const double* weight; int n_lds; };

__device__ __forceinline__ uint32_t hamming256(const uint4& a0, const uint4& a1, const uint4& q0, const uint4& q1) {
    return __popc(a0.x ^ q0.x) + __popc(a0.y ^ q0.y) + __popc(a0.z ^ q0.z) + __popc(a0.w ^ q0.w) + __popc(a1.x ^ q1.x) + __popc(a1.y ^ q1.y) + __popc(a1.z ^ q1.z) +
           __popc(a1.w ^ q1.w);
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, true); }
// minimum over a row of 16 lanes, in every lane of the row: four DPP rotations (row_ror:8, 4, 2, 1), no LDS
__device__ __forceinline__ uint32_t row16_min(uint32_t v) {
    v = min(v, dpp_u32<0x128>(v));
    v = min(v, dpp_u32<0x124>(v));
    v = min(v, dpp_u32<0x122>(v));
    v = min(v, dpp_u32<0x121>(v));
    return v;
}

// TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup) for batches of descriptors.  A GROUP of 16 lanes takes one descriptor: lane c
// takes child c of the current node (two 16-byte loads of one contiguous run, 8 xor + popcount), the key (distance << 8) | c is reduced with DPP row
// rotations — its minimum is the first minimum by construction — and the winner's link (first child, child count), loaded beside its centre, is read
// from the winner's lane.  So a level costs ONE dependent memory access.  The first kVocLdsNodes packed nodes (the top levels) are served from LDS.
// A group whose descriptor reached a leaf stops loading; the wavefront leaves the loop when its four groups have.  WIDE: nodes with 17 .. 32 children
// (k up to 20), two children per lane.
template <bool WIDE>
__global__ __launch_bounds__(kVocThreads) void k_voc_transform(const uint8_t* const* desc_ptrs, const int* counts, int stride, VocImg img, int nid_level, uint32_t* out_word,
                                                               uint32_t* out_node, double* out_weight) {
    __shared__ uint4 s_desc[kVocLdsNodes * 2];
    __shared__ uint2 s_link[kVocLdsNodes];
    const int b = blockIdx.y;
    const int cnt_b = min(counts[b], stride);
    const int first = blockIdx.x * kVocDescPerBlock;
    if (first >= cnt_b) return;   // (uniform over the workgroup)
    const int T = img.n_lds;
    for (int i = threadIdx.x; i < 2 * T; i += kVocThreads) s_desc[i] = ((const uint4*)img.desc)[i];
    for (int i = threadIdx.x; i < T; i += kVocThreads) s_link[i] = img.link[i];
    __syncthreads();
    const int c = threadIdx.x & (kVocGroup - 1), g = threadIdx.x / kVocGroup;
    const int lane_base = (threadIdx.x & 63) & ~(kVocGroup - 1);
    const uint8_t* base = desc_ptrs[b];
    for (int it = 0; it < kVocDescPerBlock / (kVocThreads / kVocGroup); it++) {
        const int kd = first + it * (kVocThreads / kVocGroup) + g;
        const bool active = kd < cnt_b;   // uniform over the group
        uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
        if (active) { const uint4* qp = (const uint4*)(base + (size_t)kd * 32); q0 = qp[0]; q1 = qp[1]; }
        uint32_t cur = 0, node_p = 0;
        uint2 lk = s_link[0];
        int level = 0;
        bool node_set = nid_level <= 0;   // node id 0 = the root
        bool run = active;
        while (__any(run)) {
            uint32_t key = 0xffffffffu;
            uint2 l0 = make_uint2(0, 0), l1 = l0;
            if (run) {
                if ((uint32_t)c < lk.y) {
                    const uint32_t idx = lk.x + c;
                    uint4 a0, a1;
                    if (idx < (uint32_t)T) { a0 = s_desc[2 * idx]; a1 = s_desc[2 * idx + 1]; l0 = s_link[idx]; }
                    else { const uint4* p = (const uint4*)(img.desc + (size_t)idx * 32); a0 = p[0]; a1 = p[1]; l0 = img.link[idx]; }
                    key = (hamming256(a0, a1, q0, q1) << 8) | (uint32_t)c;
                }
                if (WIDE && (uint32_t)(c + kVocGroup) < lk.y) {
                    const uint32_t idx = lk.x + c + kVocGroup;
                    uint4 a0, a1;
                    if (idx < (uint32_t)T) { a0 = s_desc[2 * idx]; a1 = s_desc[2 * idx + 1]; l1 = s_link[idx]; }
                    else { const uint4* p = (const uint4*)(img.desc + (size_t)idx * 32); a0 = p[0]; a1 = p[1]; l1 = img.link[idx]; }
                    key = min(key, (hamming256(a0, a1, q0, q1) << 8) | (uint32_t)(c + kVocGroup));
                }
            }
            // (all lanes of the wavefront take part in the exchanges: they are outside every divergent branch)
            key = row16_min(key);
            const uint32_t w = key & 0xffu;
            const int src = lane_base | (int)(w & (kVocGroup - 1));
            uint2 nl;
            nl.x = (uint32_t)__shfl((int)l0.x, src, 64);
            nl.y = (uint32_t)__shfl((int)l0.y, src, 64);
            if (WIDE) {
                const uint32_t x1 = (uint32_t)__shfl((int)l1.x, src, 64), y1 = (uint32_t)__shfl((int)l1.y, src, 64);
                if (w >= (uint32_t)kVocGroup) { nl.x = x1; nl.y = y1; }
            }
            if (run) {
                cur = lk.x + w;
                lk = nl;
                level++;
                if (level == nid_level) { node_p = cur; node_set = true; }
                if (lk.y == 0) run = false;   // a leaf
            }
        }
        if (active && c == 0) {
            if (!node_set) node_p = cur;   // the leaf lies above nid_level: its own id (oslam_hip.h)
            const size_t o = (size_t)b * stride + kd;
            const uint2 ids = img.ids[cur];
            if (out_word) out_word[o] = ids.y;
            if (out_node) out_node[o] = img.ids[node_p].x;
            if (out_weight) out_weight[o] = img.weight[cur];
        }
    }
}

int voc_fail(int line, const char* what) {
    if (line > 0) set_error("vocabulary: line %d (node %d): %s", line, line - 1, what);
    else set_error("vocabulary: %s", what);
    return OSLAM_E_INVALID;
}

// Checks the tree (the message names the file line = node id + 1) and builds the packed arrays.
int voc_finalize(oslam_voc& v) {
    const int n = v.n;
    if (v.k < 0 || v.k > 20 || v.L < 1 || v.L > 10 || v.scoring < 0 || v.scoring > 5 || v.weighting < 0 || v.weighting > 3)
        return voc_fail(1, "header out of range (0 <= k <= 20, 1 <= L <= 10, scoring 0..5, weighting 0..3)");
    if (n < 1) return voc_fail(2, "no node line: the vocabulary has only its root");
    std::vector<int32_t> nchild((size_t)n + 1, 0), depth((size_t)n + 1, 0);
    for (int i = 1; i <= n; i++) {
        const int p = v.parent[i - 1];
        if (p < 0 || p >= i) return voc_fail(i + 1, "parent_id is not an earlier node");
        if (p > 0 && v.leaf[p - 1]) return voc_fail(i + 1, "its parent is marked as a leaf");
        if (++nchild[p] > v.k) return voc_fail(i + 1, "its parent has more than k children");
        depth[i] = depth[p] + 1;
        v.max_depth = std::max(v.max_depth, depth[i]);
    }
    v.word.assign(n, -1);
    for (int i = 1; i <= n; i++) {
        if (v.leaf[i - 1]) v.word[i - 1] = v.n_words++;
        else if (nchild[i] == 0) return voc_fail(i + 1, "inner node without children");
        v.max_children = std::max(v.max_children, nchild[i]);
    }
    v.max_children = std::max(v.max_children, nchild[0]);
    // children of every node in file order (stable counting sort by parent), then breadth first
    std::vector<int32_t> cstart((size_t)n + 2, 0), clist(n);
    for (int i = 0; i <= n; i++) cstart[i + 1] = cstart[i] + nchild[i];
    { std::vector<int32_t> at(cstart.begin(), cstart.end() - 1); for (int i = 1; i <= n; i++) clist[at[v.parent[i - 1]]++] = i; }
    std::vector<int32_t> order((size_t)n + 1);   // packed index -> file node id
    order[0] = 0;
    v.p_link.assign((size_t)n + 1, make_uint2(0, 0));
    size_t tail = 1;
    for (size_t head = 0; head < tail; head++) {
        const int id = order[head];
        v.p_link[head] = make_uint2((uint32_t)tail, (uint32_t)nchild[id]);
        for (int j = cstart[id]; j < cstart[id + 1]; j++) order[tail++] = clist[j];
    }
    if (tail != (size_t)n + 1) return voc_fail(0, "internal: unreachable nodes");   // (cannot happen: every parent is an earlier node)
    v.p_desc.assign(((size_t)n + 1) * 32, 0); v.p_ids.resize((size_t)n + 1); v.p_weight.assign((size_t)n + 1, 0.0);
    v.p_ids[0] = make_uint2(0, 0xffffffffu);
    for (size_t p = 1; p <= (size_t)n; p++) {
        const int id = order[p];
        memcpy(&v.p_desc[p * 32], &v.desc[(size_t)(id - 1) * 32], 32);
        v.p_ids[p] = make_uint2((uint32_t)id, (uint32_t)v.word[id - 1]);
        v.p_weight[p] = v.weight[id - 1];
        if (v.p_link[p].y == 0) v.p_link[p].x = 0;
    }
    return OSLAM_OK;
}

inline int host_dist(const uint8_t* a, const uint64_t* q) {
    uint64_t c[4];
    memcpy(c, a, 32);
    return __builtin_popcountll(c[0] ^ q[0]) + __builtin_popcountll(c[1] ^ q[1]) + __builtin_popcountll(c[2] ^ q[2]) + __builtin_popcountll(c[3] ^ q[3]);
}

int voc_image(const oslam_voc* v, int device, oslam_voc::Image* out) {
    std::lock_guard<std::mutex> lock(v->mu);
    auto it = v->images.find(device);
    if (it != v->images.end()) { *out = it->second.view(); return OSLAM_OK; }
    int prev = 0;
    OSLAM_HIP_CHECK(hipGetDevice(&prev));
    OSLAM_HIP_CHECK(hipSetDevice(device));
    const size_t m = (size_t)v->n + 1;
    oslam_voc::ImageMem im;
    int rc;
    if ((rc = im.desc.alloc(m * 32)) || (rc = im.link.alloc(m * sizeof(uint2))) || (rc = im.ids.alloc(m * sizeof(uint2))) || (rc = im.weight.alloc(m * sizeof(double)))) {
        (void)hipSetDevice(prev);
        return rc;
    }
    hipError_t e = hipMemcpy(im.desc.ptr(), v->p_desc.data(), m * 32, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(im.link.ptr(), v->p_link.data(), m * sizeof(uint2), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(im.ids.ptr(), v->p_ids.data(), m * sizeof(uint2), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(im.weight.ptr(), v->p_weight.data(), m * sizeof(double), hipMemcpyHostToDevice);
    (void)hipSetDevice(prev);
    if (e != hipSuccess) { set_error("vocabulary upload failed: %s", hipGetErrorString(e)); return OSLAM_E_HIP; }
    *out = im.view();
    v->images[device] = std::move(im);
    return OSLAM_OK;
}

// ---- text parser: the whole file in memory, one pass, no stream extraction per token ----
struct Cursor {
    const char *p, *end;
    void blanks() { while (p < end && (*p == ' ' || *p == '\t' || *p == '\r')) p++; }
    bool at_eol() { blanks(); return p >= end; }
    bool integer(long& out) {   // decimal, optional sign; false when no digit is there
        blanks();
        const char* s = p;
        bool neg = false;
        if (s < end && (*s == '-' || *s == '+')) { neg = *s == '-'; s++; }
        if (s >= end || *s < '0' || *s > '9') return false;
        long val = 0;
        int digits = 0;
        while (s < end && *s >= '0' && *s <= '9') { if (++digits > 10) return false; val = val * 10 + (*s - '0'); s++; }
        if (s < end && *s != ' ' && *s != '\t' && *s != '\r') return false;
        out = neg ? -val : val;
        p = s;
        return true;
    }
    bool real(double& out) {
        blanks();
        if (p >= end) return false;
        char buf[64];
        const char* s = p;
        while (s < end && *s != ' ' && *s != '\t' && *s != '\r') s++;
        const size_t len = (size_t)(s - p);
        if (len == 0 || len >= sizeof(buf)) return false;
        memcpy(buf, p, len);
        buf[len] = 0;
        char* stop = nullptr;
        errno = 0;
        out = strtod(buf, &stop);   // correctly rounded: the value of the decimal text
        if (stop != buf + len) return false;
        p = s;
        return true;
    }
};

}  // namespace

extern "C" {

void oslam_voc_destroy(oslam_voc_t* v) {
    if (!v) return;
    delete v;
}

int oslam_voc_create(oslam_voc_t** out, int k, int L, int scoring, int weighting, int n_nodes, const int32_t* parent, const uint8_t* is_leaf, const uint8_t* desc,
                     const double* weight) {
    if (!out) { set_error("oslam_voc_create: out is NULL"); return OSLAM_E_INVALID; }
    *out = nullptr;
    if (n_nodes < 0 || (n_nodes > 0 && (!parent || !is_leaf || !desc || !weight))) { set_error("oslam_voc_create: bad argument"); return OSLAM_E_INVALID; }
    oslam_voc* v = new oslam_voc;
    v->k = k; v->L = L; v->scoring = scoring; v->weighting = weighting; v->n = n_nodes;
    v->parent.assign(parent, parent + n_nodes);
    v->leaf.resize(n_nodes);
    for (int i = 0; i < n_nodes; i++) v->leaf[i] = is_leaf[i] ? 1 : 0;
    v->desc.assign(desc, desc + (size_t)n_nodes * 32);
    v->weight.assign(weight, weight + n_nodes);
    const int rc = voc_finalize(*v);
    if (rc) { delete v; return rc; }
    *out = v;
    return OSLAM_OK;
}

int oslam_voc_load_text(oslam_voc_t** out, const char* path) {
    if (!out || !path) { set_error("oslam_voc_load_text: bad argument"); return OSLAM_E_INVALID; }
    *out = nullptr;
    FILE* f = fopen(path, "rb");
    if (!f) { set_error("vocabulary: cannot open %s", path); return OSLAM_E_INVALID; }
    std::string txt;
    {
        char buf[1 << 16];
        size_t got;
        while ((got = fread(buf, 1, sizeof(buf), f)) > 0) txt.append(buf, got);
    }
    fclose(f);
    size_t len = txt.size();
    while (len > 0 && (txt[len - 1] == '\n' || txt[len - 1] == '\r' || txt[len - 1] == ' ' || txt[len - 1] == '\t')) len--;   // blank lines at the end are not nodes
    const char *p = txt.data(), *end = p + len;
    std::unique_ptr<oslam_voc> v(new oslam_voc);
    int line = 0;
    while (p < end) {
        const char* eol = (const char*)memchr(p, '\n', (size_t)(end - p));
        if (!eol) eol = end;
        line++;
        Cursor c{p, eol};
        if (line == 1) {
            long h[4];
            for (int i = 0; i < 4; i++)
                if (!c.integer(h[i])) return voc_fail(1, "the header is not `k L scoring weighting`");
            if (!c.at_eol()) return voc_fail(1, "the header is not `k L scoring weighting`");
            if (h[0] < 0 || h[0] > 20 || h[1] < 1 || h[1] > 10 || h[2] < 0 || h[2] > 5 || h[3] < 0 || h[3] > 3)
                return voc_fail(1, "header out of range (0 <= k <= 20, 1 <= L <= 10, scoring 0..5, weighting 0..3)");
            v->k = (int)h[0]; v->L = (int)h[1]; v->scoring = (int)h[2]; v->weighting = (int)h[3];
            // (a full tree has k + k^2 + .. + k^L nodes: reserve up to the reference's 10 6)
            size_t full = 0, pw = 1;
            for (int l = 0; l < v->L && full < (1u << 21); l++) { pw *= (size_t)std::max(v->k, 1); full += pw; }
            full = std::min(full, (size_t)1 << 21);
            v->parent.reserve(full); v->leaf.reserve(full); v->desc.reserve(full * 32); v->weight.reserve(full);
        } else {
            long pid, lf, byte;
            double w;
            if (!c.integer(pid)) return voc_fail(line, "short or malformed line (parent_id)");
            if (pid < 0 || pid >= line - 1) return voc_fail(line, "parent_id is not an earlier node");
            if (!c.integer(lf)) return voc_fail(line, "short or malformed line (is_leaf)");
            if (v->parent.size() >= (size_t)0x7ffffff0) return voc_fail(line, "too many nodes");
            const size_t at = v->desc.size();
            v->desc.resize(at + 32);
            for (int i = 0; i < 32; i++) {
                if (!c.integer(byte)) return voc_fail(line, "short or malformed line (32 descriptor bytes expected)");
                if (byte < 0 || byte > 255) return voc_fail(line, "descriptor byte outside 0..255");
                v->desc[at + i] = (uint8_t)byte;
            }
            if (!c.real(w)) return voc_fail(line, "short or malformed line (weight)");
            if (!c.at_eol()) return voc_fail(line, "more than 35 fields");
            v->parent.push_back((int32_t)pid); v->leaf.push_back(lf > 0 ? 1 : 0); v->weight.push_back(w);
        }
        p = eol < end ? eol + 1 : end;
    }
    if (line == 0) return voc_fail(1, "the file is empty");
    v->n = (int)v->parent.size();
    const int rc = voc_finalize(*v);
    if (rc) return rc;
    *out = v.release();
    return OSLAM_OK;
}

int oslam_voc_info(const oslam_voc_t* v, int32_t out[8]) {
    if (!v || !out) { set_error("oslam_voc_info: bad argument"); return OSLAM_E_INVALID; }
    out[0] = v->k; out[1] = v->L; out[2] = v->scoring; out[3] = v->weighting; out[4] = v->n; out[5] = v->n_words; out[6] = v->max_depth; out[7] = v->max_children;
    return OSLAM_OK;
}

int oslam_voc_get_nodes(const oslam_voc_t* v, int32_t* parent, uint8_t* is_leaf, uint8_t* desc, double* weight, int32_t* word_id) {
    if (!v) { set_error("oslam_voc_get_nodes: bad argument"); return OSLAM_E_INVALID; }
    if (parent) memcpy(parent, v->parent.data(), 4 * (size_t)v->n);
    if (is_leaf) memcpy(is_leaf, v->leaf.data(), (size_t)v->n);
    if (desc) memcpy(desc, v->desc.data(), 32 * (size_t)v->n);
    if (weight) memcpy(weight, v->weight.data(), 8 * (size_t)v->n);
    if (word_id) memcpy(word_id, v->word.data(), 4 * (size_t)v->n);
    return OSLAM_OK;
}

int oslam_voc_transform_host(const oslam_voc_t* v, const uint8_t* desc, int n, int levelsup, uint32_t* word, uint32_t* node, double* weight) {
    if (!v || n < 0 || levelsup < 0 || (n > 0 && !desc)) { set_error("oslam_voc_transform_host: bad argument"); return OSLAM_E_INVALID; }
    const int nid_level = v->L - levelsup;
    for (int i = 0; i < n; i++) {
        uint64_t q[4];
        memcpy(q, desc + (size_t)i * 32, 32);
        uint32_t cur = 0, node_p = 0;
        bool node_set = nid_level <= 0;
        int level = 0;
        do {
            const uint2 lk = v->p_link[cur];
            uint32_t best = lk.x;
            int bd = 1 << 30;
            for (uint32_t j = 0; j < lk.y; j++) {
                const int d = host_dist(&v->p_desc[(size_t)(lk.x + j) * 32], q);
                if (d < bd) { bd = d; best = lk.x + j; }   // strict <: the first minimum wins
            }
            cur = best;
            if (++level == nid_level) { node_p = cur; node_set = true; }
        } while (v->p_link[cur].y != 0);
        if (!node_set) node_p = cur;
        if (word) word[i] = v->p_ids[cur].y;
        if (node) node[i] = v->p_ids[node_p].x;
        if (weight) weight[i] = v->p_weight[cur];
    }
    return OSLAM_OK;
}

int oslam_voc_upload(const oslam_voc_t* v, int device) {
    if (!v) { set_error("oslam_voc_upload: NULL vocabulary"); return OSLAM_E_INVALID; }
    const int ndev = oslam_device_count();
    if (ndev <= 0) { set_error("no HIP device visible: oslam_voc_transform_device has no CPU fallback (oslam_voc_transform_host is the host descent)"); return OSLAM_E_HIP; }
    if (device < 0 || device >= ndev) { set_error("oslam_voc_upload: device out of range"); return OSLAM_E_INVALID; }
    oslam_voc::Image im;
    return voc_image(v, device, &im);
}

int oslam_voc_transform_device(const oslam_voc_t* v, const uint8_t* const* d_desc_ptrs, const int32_t* d_counts, int n, int stride, int levelsup, uint32_t* d_word,
                               uint32_t* d_node, double* d_weight, void* stream) {
    if (!v || !d_desc_ptrs || !d_counts || n < 1 || stride < 1 || levelsup < 0 || (!d_word && !d_node && !d_weight)) {
        set_error("oslam_voc_transform_device: bad argument");
        return OSLAM_E_INVALID;
    }
    if (v->max_children > 2 * kVocGroup) { set_error("oslam_voc_transform_device: a node has more than 32 children"); return OSLAM_E_INVALID; }
    if (oslam_device_count() <= 0) { set_error("no HIP device visible: oslam_voc_transform_device has no CPU fallback (oslam_voc_transform_host is the host descent)"); return OSLAM_E_HIP; }
    int device = 0;
    OSLAM_HIP_CHECK(hipGetDevice(&device));
    oslam_voc::Image im;
    const int rc = voc_image(v, device, &im);
    if (rc) return rc;
    VocImg img;
    img.desc = im.desc; img.link = im.link; img.ids = im.ids; img.weight = im.weight;
    img.n_lds = std::min(v->n + 1, kVocLdsNodes);
    const int nid_level = v->L - levelsup;
    const bool wide = v->max_children > kVocGroup;
    for (int at = 0; at < n; at += 65535) {   // (grid.y limit)
        const int m = std::min(n - at, 65535);
        const size_t o = (size_t)at * stride;
        const dim3 grid(oslam::div_up(stride, kVocDescPerBlock), m);
        if (wide)
            hipLaunchKernelGGL(k_voc_transform<true>, grid, dim3(kVocThreads), 0, (hipStream_t)stream, d_desc_ptrs + at, d_counts + at, stride, img, nid_level,
                               d_word ? d_word + o : nullptr, d_node ? d_node + o : nullptr, d_weight ? d_weight + o : nullptr);
        else
            hipLaunchKernelGGL(k_voc_transform<false>, grid, dim3(kVocThreads), 0, (hipStream_t)stream, d_desc_ptrs + at, d_counts + at, stride, img, nid_level,
                               d_word ? d_word + o : nullptr, d_node ? d_node + o : nullptr, d_weight ? d_weight + o : nullptr);
    }
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int oslam_voc_transform(const oslam_voc_t* v, const uint8_t* desc, int n, int levelsup, uint32_t* word, uint32_t* node, double* weight) {
    if (!v || n < 0 || levelsup < 0 || (n > 0 && !desc)) { set_error("oslam_voc_transform: bad argument"); return OSLAM_E_INVALID; }
    if (oslam_device_count() <= 0) { set_error("no HIP device visible: oslam_voc_transform has no CPU fallback (oslam_voc_transform_host is the host descent)"); return OSLAM_E_HIP; }
    if (n == 0) return OSLAM_OK;
    int device = 0;
    OSLAM_HIP_CHECK(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(v->mu_scratch);   // (host-pointer calls on one vocabulary run one at a time)
    oslam::DeviceBuffer& scratch = v->scratch[device];
    const size_t N = (size_t)n, oDesc = 256, oWord = oDesc + oslam::align_up(32 * N, 256), oNode = oWord + oslam::align_up(4 * N, 256), oWt = oNode + oslam::align_up(4 * N, 256),
                 total = oWt + 8 * N;
    OSLAM_CHECK(scratch.grow(total, 0));
    uint8_t* const sc = scratch.bytes();
    struct { const uint8_t* ptr; int32_t count; } head = {sc + oDesc, n};   // the one-array batch: pointer table at offset 0, count at offset 8
    OSLAM_HIP_CHECK(hipMemcpy(sc, &head, sizeof(head), hipMemcpyHostToDevice));
    OSLAM_HIP_CHECK(hipMemcpy(sc + oDesc, desc, 32 * N, hipMemcpyHostToDevice));
    const int rc = oslam_voc_transform_device(v, (const uint8_t* const*)sc, (const int32_t*)(sc + 8), 1, n, levelsup, (uint32_t*)(sc + oWord), (uint32_t*)(sc + oNode),
                                              (double*)(sc + oWt), nullptr);
    if (rc) return rc;
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    if (word) OSLAM_HIP_CHECK(hipMemcpy(word, sc + oWord, 4 * N, hipMemcpyDeviceToHost));
    if (node) OSLAM_HIP_CHECK(hipMemcpy(node, sc + oNode, 4 * N, hipMemcpyDeviceToHost));
    if (weight) OSLAM_HIP_CHECK(hipMemcpy(weight, sc + oWt, 8 * N, hipMemcpyDeviceToHost));
    return OSLAM_OK;
}

int oslam_voc_vectors(const oslam_voc_t* v, int n, const uint32_t* word, const uint32_t* node, const double* weight, uint32_t* bow_ids, double* bow_vals, int32_t* n_bow,
                      uint32_t* fv_nodes, int32_t* fv_start, int32_t* fv_items, int32_t* n_fv) {
    if (!v || n < 0 || !n_bow || !n_fv || !fv_start || (n > 0 && (!word || !node || !weight || !bow_ids || !bow_vals || !fv_nodes || !fv_items))) {
        set_error("oslam_voc_vectors: bad argument");
        return OSLAM_E_INVALID;
    }
    const bool accumulate = v->weighting == 0 || v->weighting == 1;   // TF_IDF, TF: addWeight; IDF, BINARY: addIfNotExist
    std::vector<std::pair<uint32_t, int32_t>> bw, fv;
    bw.reserve(n); fv.reserve(n);
    for (int i = 0; i < n; i++)
        if (weight[i] > 0) { bw.emplace_back(word[i], i); fv.emplace_back(node[i], i); }
    std::sort(bw.begin(), bw.end());   // (word, feature index): the additions of one word stay in feature order
    std::sort(fv.begin(), fv.end());
    int nb = 0;
    for (size_t j = 0; j < bw.size(); j++) {
        if (j == 0 || bw[j].first != bw[j - 1].first) { bow_ids[nb] = bw[j].first; bow_vals[nb] = weight[bw[j].second]; nb++; }
        else if (accumulate) bow_vals[nb - 1] += weight[bw[j].second];
    }
    if (v->scoring == 0 || v->scoring == 1) {
        double norm = 0.0;
        if (v->scoring == 0) for (int j = 0; j < nb; j++) norm += std::fabs(bow_vals[j]);
        else { for (int j = 0; j < nb; j++) norm += bow_vals[j] * bow_vals[j]; norm = std::sqrt(norm); }
        if (norm > 0.0) for (int j = 0; j < nb; j++) bow_vals[j] /= norm;
    } else if (accumulate && nb > 0) {
        const double nd = (double)nb;
        for (int j = 0; j < nb; j++) bow_vals[j] /= nd;
    }
    int nf = 0;
    for (size_t j = 0; j < fv.size(); j++) {
        if (j == 0 || fv[j].first != fv[j - 1].first) { fv_nodes[nf] = fv[j].first; fv_start[nf] = (int32_t)j; nf++; }
        fv_items[j] = fv[j].second;
    }
    fv_start[nf] = (int32_t)fv.size();
    *n_bow = nb; *n_fv = nf;
    return OSLAM_OK;
}

double oslam_voc_score(const oslam_voc_t* v, int na, const uint32_t* ids_a, const double* vals_a, int nb, const uint32_t* ids_b, const double* vals_b, int* rc) {
    int dummy;
    if (!rc) rc = &dummy;
    if (!v || na < 0 || nb < 0 || (na > 0 && (!ids_a || !vals_a)) || (nb > 0 && (!ids_b || !vals_b))) { set_error("oslam_voc_score: bad argument"); *rc = OSLAM_E_INVALID; return 0.0; }
    if (v->scoring != 0) {
        set_error("oslam_voc_score: only L1_NORM (scoring 0, the reference vocabulary's) is implemented; this vocabulary has scoring %d", v->scoring);
        *rc = OSLAM_E_INVALID;
        return 0.0;
    }
    double s = 0.0;
    int i = 0, j = 0;
    while (i < na && j < nb) {
        if (ids_a[i] == ids_b[j]) { const double a = vals_a[i], b = vals_b[j]; s += std::fabs(a - b) - std::fabs(a) - std::fabs(b); i++; j++; }
        else if (ids_a[i] < ids_b[j]) i++;
        else j++;
    }
    *rc = OSLAM_OK;
    return -s / 2.0;
}

}  // extern "C"
