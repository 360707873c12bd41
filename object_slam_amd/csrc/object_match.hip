// object_match.hip — the object layer's association for batches on gfx950 (include/oslam_hip.h, "Object association"):
//  - Frame::ExtractHSVHistogramsFromMask (reference src/Frame.cc:388-414): k_hsv_hist reads every frame ONCE, converts each pixel once (OpenCV's 8-bit
//    BGR2HSV, restated in the header) and tests it against every mask of its frame; a workgroup owns a band of rows and counts into LDS with integer
//    atomics; its partial counts go to the handle's workspace and k_hsv_combine sums them per bin in band order, in integers, and normalises.
//  - ObjectMatcher::MatchTwoFrame (src/ObjectMatcher.cc:47-440) and ObjectMatcher::MatchMapToFrame (:442-801), the live code only: one launch, one
//    workgroup per problem.  Phase 1, all threads: every pair score, none of which depends on a claim.  Phase 2, one wavefront, lanes across the
//    detections: the sequential loop over objects with its claims, replayed from the score arrays.
// No atomics on global memory, no inter-workgroup synchronisation inside a kernel: every output is bit-identical from run to run.  Product code; never
// includes oracle/.
#include <cfloat>
#include <cmath>
#include <mutex>

#include "common.h"
#include "stage_layout.h"

using oslam::set_error;
using namespace oslam;

namespace {

constexpr int kBins = OSLAM_OBJMATCH_BINS;              // 32 V + 32 S + 30 H
constexpr int kMaxDet = OSLAM_OBJMATCH_MAX_DETECTIONS;  // per frame: a lane of the replaying wavefront each
constexpr int kBandRows = 32;                           // image rows of one workgroup of k_hsv_hist: 640 x 480 is 15 workgroups a frame
constexpr int kThreads = 256;
constexpr int kHsvShift = 12;

struct HsvTables {
    int32_t sdiv[256], hdiv[256];   // RGB2HSV_b's tables
    int16_t col[3][256];            // calcHist's tables as histogram columns: [0] H -> 64 + bin, [1] S -> 32 + bin, [2] V -> bin; -1 = not counted
};

}  // namespace

struct oslam_objmatch {
    int device = 0, max_frames = 0, max_w = 0, max_h = 0, max_det = 0, max_obj = 0, max_obs = 0, max_kps = 0, bands_max = 0;
    oslam::DeviceBuffer tables;   // HsvTables
    oslam::DeviceBuffer ws;       // [max_frames][bands_max][max_det][kBins] int32: the workgroups' partial counts
    oslam::StagePair io;          // staging of the host-pointer entry points
    std::mutex mu;
    bool timing = false;          // oslam_objmatch_set_timing: events before, between and after the launches
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    ~oslam_objmatch() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

namespace {

// ------------------------------------------------------------------ appearance ------------------------------------------------------------------

struct HistArgs {
    const uint8_t* img;     // [n_frames][H][stride]
    const uint8_t* masks;   // [n_masks_total][H][mstride]
    const oslam_objmatch_frame_t* frames;
    const HsvTables* tab;
    int32_t* ws;
    int32_t* counts;        // [n_masks_total][kBins]
    float* hist;
    int W, H, stride, mstride, n_masks_total, max_det, bands;
};

__host__ __device__ inline bool frame_fits(const oslam_objmatch_frame_t& f, int max_det) { return f.n_masks >= 0 && f.n_masks <= max_det; }
__host__ __device__ inline bool frame_lies_inside(const oslam_objmatch_frame_t& f, int n_masks_total) { return f.mask_off >= 0 && f.mask_off <= n_masks_total - f.n_masks; }

struct Cols { int v, s, h; };

// One pixel: RGB2HSV_b with hue range 180, then the three calcHist tables
__device__ __forceinline__ Cols pixel_cols(int b, int g, int r, const int32_t* sdiv, const int32_t* hdiv, const int16_t (*col)[256]) {
    const int v = max(b, max(g, r)), vmin = min(b, min(g, r)), diff = v - vmin;
    const int s = (diff * sdiv[v] + (1 << (kHsvShift - 1))) >> kHsvShift;
    int h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
    h = (h * hdiv[diff] + (1 << (kHsvShift - 1))) >> kHsvShift;   // (arithmetic shift of a signed int)
    h += h < 0 ? 180 : 0;
    return {col[2][v], col[1][s & 255], col[0][h & 255]};
}

__device__ __forceinline__ void count_pixel(int* hm, const Cols& c) {
    if (c.v >= 0) atomicAdd(hm + c.v, 1);
    if (c.s >= 0) atomicAdd(hm + c.s, 1);
    if (c.h >= 0) atomicAdd(hm + c.h, 1);
}

__global__ __launch_bounds__(kThreads) void k_hsv_hist(HistArgs a) {
    const int band = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const oslam_objmatch_frame_t F = a.frames[f];
    if (!(frame_fits(F, a.max_det) && frame_lies_inside(F, a.n_masks_total))) return;   // (the combine pass leaves such a frame alone too)
    const int n = F.n_masks;
    if (n == 0) return;

    __shared__ int s_hist[kMaxDet * kBins];
    __shared__ int32_t s_sdiv[256], s_hdiv[256];
    __shared__ int16_t s_col[3][256];
    for (int t = tid; t < n * kBins; t += kThreads) s_hist[t] = 0;
    s_sdiv[tid] = a.tab->sdiv[tid]; s_hdiv[tid] = a.tab->hdiv[tid];   // (kThreads == 256)
    for (int c = 0; c < 3; c++) s_col[c][tid] = a.tab->col[c][tid];
    __syncthreads();

    const int W = a.W, y0 = band * kBandRows, rows = min(kBandRows, a.H - y0);
    const uint8_t* img = a.img + (size_t)f * a.H * a.stride;
    const size_t mplane = (size_t)a.H * a.mstride;
    const uint8_t* masks = a.masks + (size_t)F.mask_off * mplane;
    // A row is cut into a scalar head (the pixels before the first one that starts on a dword), groups of four pixels = three whole dwords, and a scalar
    // tail.  Slot s of a row: s < groups -> that group; s == groups -> head and tail; above -> nothing.  W / 4 + 1 slots cover every row.
    const int slots = W / 4 + 1;
    for (int it = tid; it < rows * slots; it += kThreads) {
        const int y = y0 + it / slots, s = it % slots;
        const uint8_t* row = img + (size_t)y * a.stride;
        const uint8_t* mrow = masks + (size_t)y * a.mstride;
        const int head = min((int)((uintptr_t)row & 3), W);   // pixel x starts on a dword when x = (row address) mod 4
        const int groups = (W - head) / 4;
        if (s < groups) {
            const int x = head + 4 * s;
            const uint32_t* p = (const uint32_t*)(row + 3 * x);
            const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
            Cols c[4];
            c[0] = pixel_cols(w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255, s_sdiv, s_hdiv, s_col);
            c[1] = pixel_cols(w0 >> 24, w1 & 255, (w1 >> 8) & 255, s_sdiv, s_hdiv, s_col);
            c[2] = pixel_cols((w1 >> 16) & 255, w1 >> 24, w2 & 255, s_sdiv, s_hdiv, s_col);
            c[3] = pixel_cols((w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24, s_sdiv, s_hdiv, s_col);
            for (int m = 0; m < n; m++) {
                uint32_t mk;
                __builtin_memcpy(&mk, mrow + m * mplane + x, 4);   // four mask bytes, any alignment
                if (mk == 0) continue;
                int* hm = s_hist + m * kBins;
                // neighbouring pixels mostly share their bins: one add per run of equal columns among the group's masked pixels (measured against one add per
                // pixel and bin, DESIGN.md 7.16: 3.2 times faster on a frame of one colour, 7 to 17 % slower on noise)
                int pv = -1, ps = -1, ph = -1, nv = 0, ns = 0, nh = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (!((mk >> (8 * k)) & 255)) continue;
                    if (c[k].v == pv) nv++; else { if (pv >= 0) atomicAdd(hm + pv, nv); pv = c[k].v; nv = 1; }
                    if (c[k].s == ps) ns++; else { if (ps >= 0) atomicAdd(hm + ps, ns); ps = c[k].s; ns = 1; }
                    if (c[k].h == ph) nh++; else { if (ph >= 0) atomicAdd(hm + ph, nh); ph = c[k].h; nh = 1; }
                }
                if (pv >= 0) atomicAdd(hm + pv, nv);
                if (ps >= 0) atomicAdd(hm + ps, ns);
                if (ph >= 0) atomicAdd(hm + ph, nh);
            }
        } else if (s == groups) {
            const int tail0 = head + 4 * groups;
            for (int q = 0; q < head + (W - tail0); q++) {
                const int x = q < head ? q : tail0 + (q - head);
                const Cols c = pixel_cols(row[3 * x], row[3 * x + 1], row[3 * x + 2], s_sdiv, s_hdiv, s_col);
                for (int m = 0; m < n; m++)
                    if (mrow[m * mplane + x]) count_pixel(s_hist + m * kBins, c);
            }
        }
    }
    __syncthreads();
    int32_t* out = a.ws + ((size_t)f * a.bands + band) * a.max_det * kBins;
    for (int t = tid; t < n * kBins; t += kThreads) out[t] = s_hist[t];
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// One workgroup per frame, one wavefront per mask: the partial counts of the bands summed in band order, in integers; cv::normalize(NORM_L1)
__global__ __launch_bounds__(kThreads) void k_hsv_combine(HistArgs a) {
    const int f = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const oslam_objmatch_frame_t F = a.frames[f];
    if (!(frame_fits(F, a.max_det) && frame_lies_inside(F, a.n_masks_total))) return;
    for (int m = wave; m < F.n_masks; m += kThreads / 64) {
        int c0 = 0, c1 = 0;
        for (int band = 0; band < a.bands; band++) {
            const int32_t* p = a.ws + (((size_t)f * a.bands + band) * a.max_det + m) * kBins;
            c0 += p[lane];
            if (lane + 64 < kBins) c1 += p[lane + 64];
        }
        const double norm = (double)wave_sum(c0 + c1);   // three times the mask's pixel count
        const double scale = norm > DBL_EPSILON ? 1.0 / norm : 0.0;
        const size_t o = (size_t)(F.mask_off + m) * kBins;
        a.counts[o + lane] = c0;
        a.hist[o + lane] = (float)c0 * (float)scale;
        if (lane + 64 < kBins) { a.counts[o + lane + 64] = c1; a.hist[o + lane + 64] = (float)c1 * (float)scale; }
    }
}

// ------------------------------------------------------------------ the matchers ------------------------------------------------------------------

// ObjectMatcher::CalCosineSimilarity (:877-889), operator by operator: xy in float, xx and yy through pow(float, 2), which is a double
__device__ __forceinline__ float cosine(const float* __restrict__ h1, const float* __restrict__ h2) {
    float xy = 0.0f, xx = 0.0f, yy = 0.0f;
    for (int k = 0; k < kBins; k++) {
        const float x = h1[k], y = h2[k];
        xy += x * y;
        xx = (float)((double)xx + (double)x * (double)x);
        yy = (float)((double)yy + (double)y * (double)y);
    }
    return xy / (sqrtf(xx) * sqrtf(yy));
}

// The best (value, index) over the lanes of a wavefront whose idx >= 0, in every lane: the largest (want_max) or smallest value, and among equal values
// the largest (tie_hi) or smallest index.  Values are not NaN where idx >= 0.  All 64 lanes are active.
__device__ __forceinline__ void wave_best(float& v, int& idx, bool want_max, bool tie_hi) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(idx, off);
        const bool take = oi >= 0 && (idx < 0 || (want_max ? ov > v : ov < v) || (ov == v && (tie_hi ? oi > idx : oi < idx)));
        if (take) { v = ov; idx = oi; }
    }
}

struct PairArgs {
    const oslam_objmatch_pair_problem_t* problems;
    oslam_objmatch_det_rows_t pre, cur;
    oslam_objmatch_params_t prm;
    int n_scores, max_det;
    float *sim, *iou;
    int32_t *n_assigned, *status;
};

__global__ __launch_bounds__(kThreads) void k_match_two_frame(PairArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const oslam_objmatch_pair_problem_t P = a.problems[b];
    const bool inside = P.n_pre >= 0 && P.n_cur >= 0 && P.n_pre <= a.max_det && P.n_cur <= a.max_det && P.off_pre >= 0 && P.off_cur >= 0 && P.off_pre <= a.pre.n_rows - P.n_pre &&
                        P.off_cur <= a.cur.n_rows - P.n_cur && P.off_score >= 0 && P.off_score <= a.n_scores && P.n_pre * P.n_cur <= a.n_scores - P.off_score;
    if (!inside) {   // a refusal: the status and nothing else
        if (tid == 0) a.status[b] = OSLAM_OBJMATCH_REFUSED_RECORD;
        return;
    }
    const int nPre = P.n_pre, nCur = P.n_cur;
    __shared__ float s_hist[kMaxDet * kBins];
    __shared__ int s_label[kMaxDet], s_claim0[kMaxDet];
    for (int t = tid; t < nCur * kBins; t += kThreads) s_hist[t] = a.cur.hist[(size_t)P.off_cur * kBins + t];
    if (tid < nCur) { s_label[tid] = a.cur.label[P.off_cur + tid]; s_claim0[tid] = a.cur.obj3d[P.off_cur + tid]; }
    __syncthreads();
    float* sim = a.sim + P.off_score;
    float* iou = a.iou + P.off_score;

    // ---- phase 1: the scores of every pair that the labels and the claims the call began with allow (:98-147) ----
    for (int p = tid; p < nPre * nCur; p += kThreads) {
        const int i = p / nCur, j = p % nCur, ri = P.off_pre + i;
        float s = NAN, u = NAN;
        if (a.pre.obj3d[ri] >= 0 && s_claim0[j] < 0 && s_label[j] == a.pre.label[ri]) {
            s = cosine(a.pre.hist + (size_t)ri * kBins, s_hist + j * kBins);
            const float* pb = a.pre.box + 4 * (size_t)ri;
            const float* cb = a.cur.box + 4 * (size_t)(P.off_cur + j);
            const float preArea = pb[2] * pb[3], curArea = cb[2] * cb[3];
            const float p0 = pb[0], p1 = pb[1], p2 = pb[0] + pb[2], p3 = pb[1] + pb[3];
            const float c0 = cb[0], c1 = cb[1], c2 = cb[0] + cb[2], c3 = cb[1] + cb[3];
            const float x1 = c0 < p0 ? p0 : c0, x2 = p2 < c2 ? p2 : c2;   // std::max(Cur, Pre), std::min(Cur, Pre)
            const float y1 = c1 < p1 ? p1 : c1, y2 = p3 < c3 ? p3 : c3;
            u = 0.0f;   // (what :138 leaves unset reads as 0)
            if (!(x1 >= x2 || y1 >= y2)) {
                const float inter = (x2 - x1) * (y2 - y1);
                u = inter / (preArea + curArea - inter);
            }
        }
        sim[p] = s; iou[p] = u;
    }
    __syncthreads();

    // ---- phase 2: the loop over the previous frame's objects with its claims (:59-439), one wavefront, lane j = detection j ----
    if (tid < 64) {
        const int lane = tid;
        int claim = lane < nCur ? s_claim0[lane] : 0;
        const int label = lane < nCur ? s_label[lane] : 0;
        int assigned = 0;
        for (int i = 0; i < nPre; i++) {
            const int id = a.pre.obj3d[P.off_pre + i];
            if (id < 0) continue;
            const bool cand = lane < nCur && claim < 0 && label == a.pre.label[P.off_pre + i];
            float s = NAN, u = NAN;
            if (cand) { s = sim[i * nCur + lane]; u = iou[i * nCur + lane]; }
            else if (lane < nCur) { sim[i * nCur + lane] = NAN; iou[i * nCur + lane] = NAN; }   // claimed inside this loop
            float best = s;
            int idx = (cand && s == s) ? lane : -1;
            wave_best(best, idx, true, true);
            const float maxSim = idx >= 0 ? best : 0.0f;
            const float wIou = __shfl(u, idx >= 0 ? idx : 0);
            if (idx >= 0 && (double)maxSim > a.prm.min_similarity && (double)wIou > a.prm.min_iou) {   // :430
                if (lane == idx) claim = id;
                assigned++;
            }
        }
        if (lane < nCur) a.cur.obj3d[P.off_cur + lane] = claim;
        if (lane == 0) { a.n_assigned[b] = assigned; a.status[b] = OSLAM_OBJMATCH_DONE; }
    }
}

struct MapArgs {
    const oslam_objmatch_map_problem_t* problems;
    oslam_objmatch_det_rows_t cur;
    oslam_objmatch_obj_rows_t obj;
    oslam_objmatch_params_t prm;
    int n_scores, max_det, max_obj;
    float *sim, *mean, *mind;
    int32_t *n_by_sim, *n_by_dist, *status;
};

__global__ __launch_bounds__(kThreads) void k_match_map_to_frame(MapArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const oslam_objmatch_map_problem_t P = a.problems[b];
    const bool inside = P.n_cur >= 0 && P.n_obj >= 0 && P.n_cur <= a.max_det && P.n_obj <= a.max_obj && P.off_cur >= 0 && P.off_obj >= 0 && P.off_cur <= a.cur.n_rows - P.n_cur &&
                        P.off_obj <= a.obj.n_rows - P.n_obj && P.off_score >= 0 && P.off_score <= a.n_scores && (long long)P.n_obj * P.n_cur <= (long long)(a.n_scores - P.off_score);
    if (!inside) {
        if (tid == 0) a.status[b] = OSLAM_OBJMATCH_REFUSED_RECORD;
        return;
    }
    const int nCur = P.n_cur, nObj = P.n_obj;
    // the preconditions: every range inside its flat array, every object observed, every detection with keypoints
    __shared__ int s_bad;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    int bad = 0;
    for (int j = tid; j < nCur; j += kThreads) {
        const int kn = a.cur.kp_n[P.off_cur + j], ko = a.cur.kp_off[P.off_cur + j];
        if (kn < 1) bad |= 4;
        else if (ko < 0 || ko > a.cur.n_kps - kn) bad |= 1;
    }
    for (int i = tid; i < nObj; i += kThreads) {
        const int on = a.obj.obs_n[P.off_obj + i], oo = a.obj.obs_off[P.off_obj + i];
        if (on < 1) bad |= 2;
        else if (oo < 0 || oo > a.obj.n_obs - on) bad |= 1;
    }
    if (bad) atomicOr(&s_bad, bad);
    __syncthreads();
    bad = s_bad;
    if (bad) {
        if (tid == 0) a.status[b] = (bad & 1) ? OSLAM_OBJMATCH_REFUSED_RECORD : ((bad & 2) ? OSLAM_OBJMATCH_REFUSED_NO_OBSERVATION : OSLAM_OBJMATCH_REFUSED_NO_KEYPOINT);
        return;
    }

    __shared__ float s_hist[kMaxDet * kBins];
    __shared__ float s_ctr[kMaxDet][3];
    __shared__ int s_label[kMaxDet], s_claim0[kMaxDet];
    for (int t = tid; t < nCur * kBins; t += kThreads) s_hist[t] = a.cur.hist[(size_t)P.off_cur * kBins + t];
    if (tid < nCur) {
        s_label[tid] = a.cur.label[P.off_cur + tid];
        s_claim0[tid] = a.cur.obj3d[P.off_cur + tid];
        // the centre of the detection's unprojected keypoints (:567-573, Frame::UnprojectStereo src/Frame.cc:906-920), in keypoint order
        const int kn = a.cur.kp_n[P.off_cur + tid];
        const float* kp = a.cur.kps + 3 * (size_t)a.cur.kp_off[P.off_cur + tid];
        const float invfx = 1.0f / P.fx, invfy = 1.0f / P.fy;
        float sx = 0.0f, sy = 0.0f, sz = 0.0f;
        for (int q = 0; q < kn; q++) {
            const float u = kp[3 * q], v = kp[3 * q + 1], z = kp[3 * q + 2];
            const float x = (u - P.cx) * z * invfx, y = (v - P.cy) * z * invfy;
            sx = sx + (P.Rwc[0] * x + P.Rwc[1] * y + P.Rwc[2] * z + P.Ow[0]);
            sy = sy + (P.Rwc[3] * x + P.Rwc[4] * y + P.Rwc[5] * z + P.Ow[1]);
            sz = sz + (P.Rwc[6] * x + P.Rwc[7] * y + P.Rwc[8] * z + P.Ow[2]);
        }
        const float inv = (float)(1.0 / (double)kn);
        s_ctr[tid][0] = sx * inv; s_ctr[tid][1] = sy * inv; s_ctr[tid][2] = sz * inv;
    }
    __syncthreads();
    float* sim = a.sim + P.off_score;
    float* mean = a.mean + P.off_score;
    float* mind = a.mind + P.off_score;

    // ---- phase 1: eight lanes per (object, detection) pair.  The similarity is a maximum over the observations (:519-542): each lane takes every eighth
    //      one; the distances are sums in observation order (:577-591): lane 0 of the eight walks them. ----
    const int grp = tid >> 3, t8 = tid & 7;
    for (int p = grp; p < nObj * nCur; p += kThreads / 8) {
        const int i = p / nCur, j = p % nCur, ri = P.off_obj + i;
        const int id = a.obj.obj3d_id[ri];
        bool skip = id < 0 || s_claim0[j] >= 0 || s_label[j] != a.obj.label[ri];
        for (int k = 0; k < nCur && !skip; k++) skip = s_claim0[k] == id;   // the snapshot of :451-459
        if (skip) {
            if (t8 == 0) { sim[p] = NAN; mean[p] = NAN; mind[p] = NAN; }
            continue;
        }
        const int on = a.obj.obs_n[ri], oo = a.obj.obs_off[ri];
        float best = 0.0f;
        for (int o = t8; o < on; o += 8) {
            const float s = cosine(a.obj.obs_hist + (size_t)(oo + o) * kBins, s_hist + j * kBins);
            if (s > best) best = s;
        }
#pragma unroll
        for (int off = 1; off <= 4; off <<= 1) {
            const float ob = __shfl_xor(best, off);
            if (ob > best) best = ob;
        }
        if (t8 == 0) {
            const float cx = s_ctr[j][0], cy = s_ctr[j][1], cz = s_ctr[j][2];
            float sum = 0.0f, mn = FLT_MAX;
            for (int o = 0; o < on; o++) {
                const float* oc = a.obj.obs_center + 3 * (size_t)(oo + o);
                const float dx = oc[0] - cx, dy = oc[1] - cy, dz = oc[2] - cz;
                const float d = (float)sqrt((double)dx * (double)dx + (double)dy * (double)dy + (double)dz * (double)dz);
                sum = sum + d;
                if (d < mn) mn = d;
            }
            sim[p] = best; mean[p] = sum / (float)on; mind[p] = mn;
        }
    }
    __syncthreads();

    // ---- phase 2: the loop over the map's objects with its claims (:465-799), one wavefront, lane j = detection j ----
    if (tid < 64) {
        const int lane = tid;
        int claim = lane < nCur ? s_claim0[lane] : 0;
        const int claim0 = claim, label = lane < nCur ? s_label[lane] : 0;
        int bySim = 0, byDist = 0;
        for (int i = 0; i < nObj; i++) {
            const int ri = P.off_obj + i, id = a.obj.obj3d_id[ri];
            if (id < 0 || __ballot(lane < nCur && claim0 == id)) continue;
            const bool cand = lane < nCur && claim < 0 && label == a.obj.label[ri];
            float s = NAN, dm = NAN, dn = NAN;
            if (cand) { s = sim[i * nCur + lane]; dm = mean[i * nCur + lane]; dn = mind[i * nCur + lane]; }
            else if (lane < nCur) { sim[i * nCur + lane] = NAN; mean[i * nCur + lane] = NAN; mind[i * nCur + lane] = NAN; }
            float bestS = s, bestD = dn;
            int idx = (cand && s == s) ? lane : -1, idx2 = (cand && dn == dn) ? lane : -1;
            wave_best(bestS, idx, true, true);     // std::sort, back(): the largest index among equals (:637-648)
            wave_best(bestD, idx2, false, false);  // std::sort, front(): the smallest index among equals (:657-668)
            const float maxSim = idx >= 0 ? bestS : 0.0f, minMin = idx2 >= 0 ? bestD : 0.0f;
            const float wMean = __shfl(dm, idx >= 0 ? idx : 0);
            if (idx >= 0 && (double)maxSim > a.prm.min_similarity && (double)wMean < a.prm.max_mean_dist) {   // :783
                if (lane == idx) claim = id;
                bySim++;
            }
            if (idx2 >= 0 && (double)minMin < a.prm.max_min_dist) {   // :789
                if (lane == idx2) claim = id;
                byDist++;
            }
        }
        if (lane < nCur) a.cur.obj3d[P.off_cur + lane] = claim;
        if (lane == 0) { a.n_by_sim[b] = bySim; a.n_by_dist[b] = byDist; a.status[b] = OSLAM_OBJMATCH_DONE; }
    }
}

// ------------------------------------------------------------------ host ------------------------------------------------------------------

int cv_round(double v) { return (int)std::nearbyint(v); }   // saturate_cast<int>(double): to nearest, ties to even (the default rounding mode)

void fill_tables(HsvTables& t) {
    t.sdiv[0] = t.hdiv[0] = 0;
    for (int i = 1; i < 256; i++) {
        t.sdiv[i] = cv_round((255 << kHsvShift) / (1.0 * i));
        t.hdiv[i] = cv_round((180 << kHsvShift) / (6.0 * i));
    }
    const double low[3] = {0.0, 0.0, 0.0}, high[3] = {180.0, 256.0, 256.0};   // hRanges, sRanges, vRanges (include/Frame.h:123-125)
    const int size[3] = {30, 32, 32}, first[3] = {64, 32, 0};                 // HSVhistSize (:127); the columns after the hconcat calls (:403-410)
    for (int c = 0; c < 3; c++) {
        const double sa = size[c] / (high[c] - low[c]), sb = -sa * low[c];
        for (int j = 0; j < 256; j++) {
            const int idx = (int)std::floor(j * sa + sb);
            t.col[c][j] = (int16_t)(idx >= 0 && idx < size[c] ? first[c] + idx : -1);
        }
    }
}

int check_params(const char* fn, const oslam_objmatch_params_t* p) {
    if (!p) { set_error("%s: params is NULL", fn); return OSLAM_E_INVALID; }
    if (std::isnan(p->min_similarity) || std::isnan(p->min_iou) || std::isnan(p->max_mean_dist) || std::isnan(p->max_min_dist)) { set_error("%s: a threshold is NaN", fn); return OSLAM_E_INVALID; }
    return OSLAM_OK;
}

int check_hsv(const char* fn, const oslam_objmatch* h, int n_frames, int W, int H, int stride, int mstride, int n_masks_total) {
    if (!h) { set_error("%s: handle is NULL", fn); return OSLAM_E_INVALID; }
    if (n_frames < 0 || n_masks_total < 0) { set_error("%s: %d frames, %d masks: none may be negative", fn, n_frames, n_masks_total); return OSLAM_E_CAPACITY; }
    if (n_frames > h->max_frames) { set_error("%s: %d frames exceed the handle's %d", fn, n_frames, h->max_frames); return OSLAM_E_CAPACITY; }
    if (W > h->max_w || H > h->max_h) { set_error("%s: %d x %d exceeds the handle's %d x %d", fn, W, H, h->max_w, h->max_h); return OSLAM_E_CAPACITY; }
    if ((long long)n_masks_total > (long long)h->max_frames * h->max_det) { set_error("%s: %d masks exceed the handle's %d frames of %d", fn, n_masks_total, h->max_frames, h->max_det); return OSLAM_E_CAPACITY; }
    if (W < 1 || H < 1 || stride < 3 * W || mstride < W) { set_error("%s: %d x %d with strides %d and %d", fn, W, H, stride, mstride); return OSLAM_E_INVALID; }
    return OSLAM_OK;
}

int launch_hsv(const char* fn, oslam_objmatch* h, int n_frames, int W, int H, int stride, int mstride, const uint8_t* d_images, const oslam_objmatch_frame_t* d_frames,
               int n_masks_total, const uint8_t* d_masks, int32_t* d_counts, float* d_hist, hipStream_t stream) {
    OSLAM_CHECK(check_hsv(fn, h, n_frames, W, H, stride, mstride, n_masks_total));
    if (n_frames == 0) return OSLAM_OK;
    if (!d_images || !d_frames || (n_masks_total > 0 && (!d_masks || !d_counts || !d_hist))) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    HistArgs a;
    a.img = d_images; a.masks = d_masks; a.frames = d_frames; a.tab = h->tables.as<HsvTables>(); a.ws = h->ws.as<int32_t>(); a.counts = d_counts; a.hist = d_hist;
    a.W = W; a.H = H; a.stride = stride; a.mstride = mstride; a.n_masks_total = n_masks_total; a.max_det = h->max_det; a.bands = div_up(H, kBandRows);
    if (h->timing) OSLAM_HIP_CHECK(hipEventRecord(h->ev[0], stream));
    hipLaunchKernelGGL(k_hsv_hist, dim3(a.bands, n_frames), dim3(kThreads), 0, stream, a);
    if (h->timing) OSLAM_HIP_CHECK(hipEventRecord(h->ev[1], stream));
    hipLaunchKernelGGL(k_hsv_combine, dim3(n_frames), dim3(kThreads), 0, stream, a);
    if (h->timing) OSLAM_HIP_CHECK(hipEventRecord(h->ev[2], stream));
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

// what the handle bounds of a matcher call: checked before anything is launched
int check_match(const char* fn, const oslam_objmatch* h, int n_problems, const oslam_objmatch_det_rows_t* cur, int other_rows, int other_cap, int n_obs, int n_scores,
                const oslam_objmatch_params_t* prm) {
    if (!h || !cur) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_CHECK(check_params(fn, prm));
    if (n_problems < 0 || cur->n_rows < 0 || cur->n_kps < 0 || other_rows < 0 || n_obs < 0 || n_scores < 0) { set_error("%s: a negative count", fn); return OSLAM_E_CAPACITY; }
    if (n_problems > h->max_frames) { set_error("%s: %d problems exceed the handle's %d", fn, n_problems, h->max_frames); return OSLAM_E_CAPACITY; }
    const long long det_cap = (long long)h->max_frames * h->max_det;
    if (cur->n_rows > det_cap) { set_error("%s: %d detection rows exceed the handle's %lld", fn, cur->n_rows, det_cap); return OSLAM_E_CAPACITY; }
    if (other_rows > (long long)h->max_frames * other_cap) { set_error("%s: %d object rows exceed the handle's %lld", fn, other_rows, (long long)h->max_frames * other_cap); return OSLAM_E_CAPACITY; }
    if (n_obs > h->max_obs) { set_error("%s: %d observations exceed the handle's max_observations_total %d", fn, n_obs, h->max_obs); return OSLAM_E_CAPACITY; }
    if (cur->n_kps > h->max_kps) { set_error("%s: %d keypoints exceed the handle's max_keypoints_total %d", fn, cur->n_kps, h->max_kps); return OSLAM_E_CAPACITY; }
    return OSLAM_OK;
}

int launch_two_frame(const char* fn, oslam_objmatch* h, int n_problems, const oslam_objmatch_pair_problem_t* d_problems, const oslam_objmatch_det_rows_t* pre,
                     const oslam_objmatch_det_rows_t* cur, const oslam_objmatch_params_t* prm, int n_scores, float* d_sim, float* d_iou, int32_t* d_n_assigned, int32_t* d_status,
                     hipStream_t stream) {
    if (!h || !pre) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_CHECK(check_match(fn, h, n_problems, cur, pre->n_rows, h->max_det, 0, n_scores, prm));
    if (n_problems == 0) return OSLAM_OK;
    if (!d_problems || !d_n_assigned || !d_status || (n_scores > 0 && (!d_sim || !d_iou)) || (pre->n_rows > 0 && (!pre->label || !pre->hist || !pre->box || !pre->obj3d)) ||
        (cur->n_rows > 0 && (!cur->label || !cur->hist || !cur->box || !cur->obj3d))) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    PairArgs a;
    a.problems = d_problems; a.pre = *pre; a.cur = *cur; a.prm = *prm; a.n_scores = n_scores; a.max_det = h->max_det;
    a.sim = d_sim; a.iou = d_iou; a.n_assigned = d_n_assigned; a.status = d_status;
    if (h->timing) OSLAM_HIP_CHECK(hipEventRecord(h->ev[0], stream));
    hipLaunchKernelGGL(k_match_two_frame, dim3(n_problems), dim3(kThreads), 0, stream, a);
    if (h->timing) { OSLAM_HIP_CHECK(hipEventRecord(h->ev[1], stream)); OSLAM_HIP_CHECK(hipEventRecord(h->ev[2], stream)); }
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int launch_map(const char* fn, oslam_objmatch* h, int n_problems, const oslam_objmatch_map_problem_t* d_problems, const oslam_objmatch_det_rows_t* cur,
               const oslam_objmatch_obj_rows_t* obj, const oslam_objmatch_params_t* prm, int n_scores, float* d_sim, float* d_mean, float* d_min, int32_t* d_by_sim,
               int32_t* d_by_dist, int32_t* d_status, hipStream_t stream) {
    if (!h || !obj) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_CHECK(check_match(fn, h, n_problems, cur, obj->n_rows, h->max_obj, obj->n_obs, n_scores, prm));
    if (n_problems == 0) return OSLAM_OK;
    if (!d_problems || !d_by_sim || !d_by_dist || !d_status || (n_scores > 0 && (!d_sim || !d_mean || !d_min)) ||
        (cur->n_rows > 0 && (!cur->label || !cur->hist || !cur->obj3d || !cur->kp_off || !cur->kp_n)) || (cur->n_kps > 0 && !cur->kps) ||
        (obj->n_rows > 0 && (!obj->obj3d_id || !obj->label || !obj->obs_off || !obj->obs_n)) || (obj->n_obs > 0 && (!obj->obs_center || !obj->obs_hist))) {
        set_error("%s: NULL argument", fn);
        return OSLAM_E_INVALID;
    }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    MapArgs a;
    a.problems = d_problems; a.cur = *cur; a.obj = *obj; a.prm = *prm; a.n_scores = n_scores; a.max_det = h->max_det; a.max_obj = h->max_obj;
    a.sim = d_sim; a.mean = d_mean; a.mind = d_min; a.n_by_sim = d_by_sim; a.n_by_dist = d_by_dist; a.status = d_status;
    if (h->timing) OSLAM_HIP_CHECK(hipEventRecord(h->ev[0], stream));
    hipLaunchKernelGGL(k_match_map_to_frame, dim3(n_problems), dim3(kThreads), 0, stream, a);
    if (h->timing) { OSLAM_HIP_CHECK(hipEventRecord(h->ev[1], stream)); OSLAM_HIP_CHECK(hipEventRecord(h->ev[2], stream)); }
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

}  // namespace

extern "C" {

void oslam_objmatch_destroy(oslam_objmatch_t* h) {
    if (!h) return;
    delete h;
}

int oslam_objmatch_create(oslam_objmatch_t** out, int max_frames, int max_width, int max_height, int max_detections, int max_objects, int max_observations_total,
                          int max_keypoints_total) {
    if (!out) { set_error("oslam_objmatch_create: out is NULL"); return OSLAM_E_INVALID; }
    *out = nullptr;
    if (max_frames < 1 || max_width < 1 || max_height < 1 || max_objects < 1 || max_observations_total < 1 || max_keypoints_total < 1 || max_detections < 8 ||
        max_detections > kMaxDet || (long long)max_width * max_height > (1ll << 29)) {
        set_error("oslam_objmatch_create: bad argument (max_detections is 8 .. %d, max_width * max_height at most 2^29)", kMaxDet);
        return OSLAM_E_INVALID;
    }
    if (oslam_device_count() <= 0) return oslam::no_device("oslam_objmatch_create");
    oslam_objmatch* h = new oslam_objmatch;
    h->max_frames = max_frames; h->max_w = max_width; h->max_h = max_height; h->max_det = max_detections; h->max_obj = max_objects;
    h->max_obs = max_observations_total; h->max_kps = max_keypoints_total; h->bands_max = div_up(max_height, kBandRows);
    HsvTables t;
    fill_tables(t);
    int rc = hipGetDevice(&h->device) == hipSuccess ? OSLAM_OK : OSLAM_E_HIP;
    if (rc != OSLAM_OK) set_error("oslam_objmatch_create: hipGetDevice failed");
    if (rc == OSLAM_OK) rc = h->tables.alloc(sizeof(HsvTables));
    if (rc == OSLAM_OK) rc = h->ws.alloc((size_t)max_frames * h->bands_max * max_detections * kBins * sizeof(int32_t));
    if (rc == OSLAM_OK && hipMemcpy(h->tables.ptr(), &t, sizeof t, hipMemcpyHostToDevice) != hipSuccess) { set_error("oslam_objmatch_create: hipMemcpy failed"); rc = OSLAM_E_HIP; }
    if (rc != OSLAM_OK) { delete h; return rc; }
    *out = h;
    return OSLAM_OK;
}

int oslam_objmatch_set_timing(oslam_objmatch_t* h, int on) {
    if (!h) { set_error("oslam_objmatch_set_timing: handle is NULL"); return OSLAM_E_INVALID; }
    if (on)
        for (hipEvent_t& e : h->ev) if (!e) OSLAM_HIP_CHECK(hipEventCreate(&e));
    h->timing = on != 0;
    return OSLAM_OK;
}

int oslam_objmatch_last_kernel_ms(oslam_objmatch_t* h, float ms[2]) {
    if (!h || !ms || !h->timing) { set_error("oslam_objmatch_last_kernel_ms: timing is not on"); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipEventSynchronize(h->ev[2]));
    OSLAM_HIP_CHECK(hipEventElapsedTime(&ms[0], h->ev[0], h->ev[1]));
    OSLAM_HIP_CHECK(hipEventElapsedTime(&ms[1], h->ev[1], h->ev[2]));
    return OSLAM_OK;
}

int oslam_objmatch_hsv_histograms_device(oslam_objmatch_t* h, int n_frames, int width, int height, int stride, int mask_stride, const uint8_t* d_images,
                                         const oslam_objmatch_frame_t* d_frames, int n_masks_total, const uint8_t* d_masks, int32_t* d_counts, float* d_hist, void* stream) {
    return launch_hsv("oslam_objmatch_hsv_histograms_device", h, n_frames, width, height, stride, mask_stride, d_images, d_frames, n_masks_total, d_masks, d_counts, d_hist,
                      (hipStream_t)stream);
}

int oslam_objmatch_hsv_histograms(oslam_objmatch_t* h, int n_frames, int width, int height, int stride, int mask_stride, const uint8_t* images, const oslam_objmatch_frame_t* frames,
                                  int n_masks_total, const uint8_t* masks, int32_t* counts, float* hist) {
    const char* fn = "oslam_objmatch_hsv_histograms";
    OSLAM_CHECK(check_hsv(fn, h, n_frames, width, height, stride, mask_stride, n_masks_total));
    if (n_frames == 0) return OSLAM_OK;
    if (!images || !frames || (n_masks_total > 0 && (!masks || !counts || !hist))) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    for (int f = 0; f < n_frames; f++) {
        if (!frame_fits(frames[f], h->max_det)) { set_error("%s: frame %d has %d masks (at most %d, not negative)", fn, f, frames[f].n_masks, h->max_det); return OSLAM_E_CAPACITY; }
        if (!frame_lies_inside(frames[f], n_masks_total)) { set_error("%s: frame %d (masks %d + %d) lies outside the %d masks", fn, f, frames[f].mask_off, frames[f].n_masks, n_masks_total); return OSLAM_E_INVALID; }
    }
    std::lock_guard<std::mutex> lock(h->mu);
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t nf = (size_t)n_frames, nm = (size_t)n_masks_total;
    oslam::StageLayout lay;   // inputs, then what is read and written: one upload, one download
    const auto fFr = lay.add<oslam_objmatch_frame_t>(nf);
    const auto fImg = lay.add<uint8_t>(nf * height * stride), fMask = lay.add<uint8_t>(nm * height * mask_stride);
    const auto fCnt = lay.add<int32_t>(nm * kBins);
    const auto fHist = lay.add<float>(nm * kBins);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fFr, ph, frames); put(fImg, ph, images); put(fMask, ph, masks);
    put(fCnt, ph, (const int32_t*)counts); put(fHist, ph, (const float*)hist);   // rows no frame owns come back as they were
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, nullptr));
    OSLAM_CHECK(launch_hsv(fn, h, n_frames, width, height, stride, mask_stride, at(fImg, pd), at(fFr, pd), n_masks_total, at(fMask, pd), at(fCnt, pd), at(fHist, pd), nullptr));
    if (lay.total() > fCnt.off) OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fCnt.off, pd + fCnt.off, lay.total() - fCnt.off, hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(fCnt, ph, counts); get(fHist, ph, hist);
    return OSLAM_OK;
}

int oslam_objmatch_match_two_frame_device(oslam_objmatch_t* h, int n_problems, const oslam_objmatch_pair_problem_t* d_problems, const oslam_objmatch_det_rows_t* pre,
                                          const oslam_objmatch_det_rows_t* cur, const oslam_objmatch_params_t* params, int n_scores, float* d_similarity, float* d_iou,
                                          int32_t* d_n_assigned, int32_t* d_status, void* stream) {
    return launch_two_frame("oslam_objmatch_match_two_frame_device", h, n_problems, d_problems, pre, cur, params, n_scores, d_similarity, d_iou, d_n_assigned, d_status,
                            (hipStream_t)stream);
}

int oslam_objmatch_match_two_frame(oslam_objmatch_t* h, int n_problems, const oslam_objmatch_pair_problem_t* problems, const oslam_objmatch_det_rows_t* pre,
                                   const oslam_objmatch_det_rows_t* cur, const oslam_objmatch_params_t* params, int n_scores, float* similarity, float* iou, int32_t* n_assigned,
                                   int32_t* status) {
    const char* fn = "oslam_objmatch_match_two_frame";
    if (!h || !pre) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_CHECK(check_match(fn, h, n_problems, cur, pre->n_rows, h->max_det, 0, n_scores, params));
    if (n_problems == 0) return OSLAM_OK;
    if (!problems || !n_assigned || !status || (n_scores > 0 && (!similarity || !iou)) || (pre->n_rows > 0 && (!pre->label || !pre->hist || !pre->box || !pre->obj3d)) ||
        (cur->n_rows > 0 && (!cur->label || !cur->hist || !cur->box || !cur->obj3d))) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    std::lock_guard<std::mutex> lock(h->mu);
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t np = (size_t)n_problems, rp = (size_t)pre->n_rows, rc = (size_t)cur->n_rows, ns = (size_t)n_scores;
    oslam::StageLayout lay;
    const auto fProb = lay.add<oslam_objmatch_pair_problem_t>(np);
    const auto fPL = lay.add<int32_t>(rp), fPO = lay.add<int32_t>(rp);
    const auto fPH = lay.add<float>(rp * kBins), fPB = lay.add<float>(rp * 4);
    const auto fCL = lay.add<int32_t>(rc);
    const auto fCH = lay.add<float>(rc * kBins), fCB = lay.add<float>(rc * 4);
    const auto fCO = lay.add<int32_t>(rc);   // from here on: read and written
    const auto fSim = lay.add<float>(ns), fIou = lay.add<float>(ns);
    const auto fNas = lay.add<int32_t>(np), fSt = lay.add<int32_t>(np);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fProb, ph, problems); put(fPL, ph, pre->label); put(fPO, ph, (const int32_t*)pre->obj3d); put(fPH, ph, pre->hist); put(fPB, ph, pre->box);
    put(fCL, ph, cur->label); put(fCH, ph, cur->hist); put(fCB, ph, cur->box); put(fCO, ph, (const int32_t*)cur->obj3d);
    put(fSim, ph, (const float*)similarity); put(fIou, ph, (const float*)iou); put(fNas, ph, (const int32_t*)n_assigned); put(fSt, ph, (const int32_t*)status);
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, nullptr));
    oslam_objmatch_det_rows_t dp = {}, dc = {};
    dp.n_rows = pre->n_rows; dp.label = at(fPL, pd); dp.hist = at(fPH, pd); dp.box = at(fPB, pd); dp.obj3d = at(fPO, pd);
    dc.n_rows = cur->n_rows; dc.label = at(fCL, pd); dc.hist = at(fCH, pd); dc.box = at(fCB, pd); dc.obj3d = at(fCO, pd);
    OSLAM_CHECK(launch_two_frame(fn, h, n_problems, at(fProb, pd), &dp, &dc, params, n_scores, at(fSim, pd), at(fIou, pd), at(fNas, pd), at(fSt, pd), nullptr));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fCO.off, pd + fCO.off, lay.total() - fCO.off, hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(fCO, ph, cur->obj3d); get(fSim, ph, similarity); get(fIou, ph, iou); get(fNas, ph, n_assigned); get(fSt, ph, status);
    return OSLAM_OK;
}

int oslam_objmatch_match_map_to_frame_device(oslam_objmatch_t* h, int n_problems, const oslam_objmatch_map_problem_t* d_problems, const oslam_objmatch_det_rows_t* cur,
                                             const oslam_objmatch_obj_rows_t* objects, const oslam_objmatch_params_t* params, int n_scores, float* d_similarity, float* d_mean_dist,
                                             float* d_min_dist, int32_t* d_n_by_similarity, int32_t* d_n_by_distance, int32_t* d_status, void* stream) {
    return launch_map("oslam_objmatch_match_map_to_frame_device", h, n_problems, d_problems, cur, objects, params, n_scores, d_similarity, d_mean_dist, d_min_dist,
                      d_n_by_similarity, d_n_by_distance, d_status, (hipStream_t)stream);
}

int oslam_objmatch_match_map_to_frame(oslam_objmatch_t* h, int n_problems, const oslam_objmatch_map_problem_t* problems, const oslam_objmatch_det_rows_t* cur,
                                      const oslam_objmatch_obj_rows_t* obj, const oslam_objmatch_params_t* params, int n_scores, float* similarity, float* mean_dist, float* min_dist,
                                      int32_t* n_by_similarity, int32_t* n_by_distance, int32_t* status) {
    const char* fn = "oslam_objmatch_match_map_to_frame";
    if (!h || !obj) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_CHECK(check_match(fn, h, n_problems, cur, obj->n_rows, h->max_obj, obj->n_obs, n_scores, params));
    if (n_problems == 0) return OSLAM_OK;
    if (!problems || !n_by_similarity || !n_by_distance || !status || (n_scores > 0 && (!similarity || !mean_dist || !min_dist)) ||
        (cur->n_rows > 0 && (!cur->label || !cur->hist || !cur->obj3d || !cur->kp_off || !cur->kp_n)) || (cur->n_kps > 0 && !cur->kps) ||
        (obj->n_rows > 0 && (!obj->obj3d_id || !obj->label || !obj->obs_off || !obj->obs_n)) || (obj->n_obs > 0 && (!obj->obs_center || !obj->obs_hist))) {
        set_error("%s: NULL argument", fn);
        return OSLAM_E_INVALID;
    }
    std::lock_guard<std::mutex> lock(h->mu);
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t np = (size_t)n_problems, rc = (size_t)cur->n_rows, nk = (size_t)cur->n_kps, ro = (size_t)obj->n_rows, no = (size_t)obj->n_obs, ns = (size_t)n_scores;
    oslam::StageLayout lay;
    const auto fProb = lay.add<oslam_objmatch_map_problem_t>(np);
    const auto fCL = lay.add<int32_t>(rc), fKO = lay.add<int32_t>(rc), fKN = lay.add<int32_t>(rc);
    const auto fCH = lay.add<float>(rc * kBins), fKp = lay.add<float>(nk * 3);
    const auto fOI = lay.add<int32_t>(ro), fOL = lay.add<int32_t>(ro), fOO = lay.add<int32_t>(ro), fON = lay.add<int32_t>(ro);
    const auto fOC = lay.add<float>(no * 3), fOH = lay.add<float>(no * kBins);
    const auto fCO = lay.add<int32_t>(rc);   // from here on: read and written
    const auto fSim = lay.add<float>(ns), fMean = lay.add<float>(ns), fMin = lay.add<float>(ns);
    const auto fBS = lay.add<int32_t>(np), fBD = lay.add<int32_t>(np), fSt = lay.add<int32_t>(np);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fProb, ph, problems); put(fCL, ph, cur->label); put(fKO, ph, cur->kp_off); put(fKN, ph, cur->kp_n); put(fCH, ph, cur->hist); put(fKp, ph, cur->kps);
    put(fOI, ph, obj->obj3d_id); put(fOL, ph, obj->label); put(fOO, ph, obj->obs_off); put(fON, ph, obj->obs_n); put(fOC, ph, obj->obs_center); put(fOH, ph, obj->obs_hist);
    put(fCO, ph, (const int32_t*)cur->obj3d); put(fSim, ph, (const float*)similarity); put(fMean, ph, (const float*)mean_dist); put(fMin, ph, (const float*)min_dist);
    put(fBS, ph, (const int32_t*)n_by_similarity); put(fBD, ph, (const int32_t*)n_by_distance); put(fSt, ph, (const int32_t*)status);
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, nullptr));
    oslam_objmatch_det_rows_t dc = {};
    dc.n_rows = cur->n_rows; dc.label = at(fCL, pd); dc.hist = at(fCH, pd); dc.obj3d = at(fCO, pd); dc.kp_off = at(fKO, pd); dc.kp_n = at(fKN, pd); dc.n_kps = cur->n_kps; dc.kps = at(fKp, pd);
    oslam_objmatch_obj_rows_t dobj = {};
    dobj.n_rows = obj->n_rows; dobj.obj3d_id = at(fOI, pd); dobj.label = at(fOL, pd); dobj.obs_off = at(fOO, pd); dobj.obs_n = at(fON, pd); dobj.n_obs = obj->n_obs;
    dobj.obs_center = at(fOC, pd); dobj.obs_hist = at(fOH, pd);
    OSLAM_CHECK(launch_map(fn, h, n_problems, at(fProb, pd), &dc, &dobj, params, n_scores, at(fSim, pd), at(fMean, pd), at(fMin, pd), at(fBS, pd), at(fBD, pd), at(fSt, pd), nullptr));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fCO.off, pd + fCO.off, lay.total() - fCO.off, hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(fCO, ph, cur->obj3d); get(fSim, ph, similarity); get(fMean, ph, mean_dist); get(fMin, ph, min_dist); get(fBS, ph, n_by_similarity); get(fBD, ph, n_by_distance);
    get(fSt, ph, status);
    return OSLAM_OK;
}

}  // extern "C"
