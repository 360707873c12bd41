// sim3_match.hip — ORBmatcher::SearchBySim3 (reference src/ORBmatcher.cc:1102-1326) for batches of independent keyframe pairs on gfx950
// (include/oslam_hip.h, "SearchBySim3").  One launch, one workgroup per pair: the workgroup stages KF2 in LDS (keypoint xy, octave, descriptors and
// the 64 x 48 cell table: window_search.h, which also has the level, the window walk and the Hamming minimum), its threads stride over KF1's map points
// (:1148-1225), then it stages KF1 in the same LDS and strides over KF2's map points (:1228-1305); vnMatch1 and vnMatch2 stay in LDS and the agreement
// (:1308-1323) follows after a barrier.
// No inter-workgroup synchronisation and no atomics on global memory: the result does not depend on the order the hardware runs anything in.
// The roundings are those the header lists.  Product code; never includes oracle/.
#include <climits>
#include <cmath>
#include <mutex>

#include "common.h"
#include "stage_layout.h"
#include "window_search.h"

using oslam::set_error;
using namespace oslam::kf_stage;   // the staged keyframe, the window search and gemm_row

struct oslam_sim3_match {
    int device = 0, max_pairs = 0, max_kps = 0;
    size_t lds = 0;
    oslam::StagePair io;   // staging of the host-pointer entry point: inputs | outputs
    std::mutex mu;
};

namespace {

constexpr int kThHigh = 100;                    // ORBmatcher::TH_HIGH, src/ORBmatcher.cc:36
constexpr int kSkip = -2;                       // vbAlreadyMatched, kept in the vnMatch arrays (never equal to a keypoint index)

struct Sim3MatchArgs {
    const oslam_sim3_pair_t* pairs;
    int n_pairs, n_rows, n_out, ncap;
    oslam_sim3_match_rows_t rows;
    const int32_t* matched_in;
    int32_t* match12; int32_t* n_found;
    WindowCam cam;
};

__device__ __forceinline__ bool finite_all(const float* v, int n) {
    bool ok = true;
    for (int i = 0; i < n; i++) ok = ok && isfinite(v[i]);
    return ok;
}

// The target keyframe (rows off .. off + N - 1) into LDS
__device__ __forceinline__ void stage_rows(const Sim3MatchArgs& a, const Lds& s, int off, int N, int* s_wtot) {
    stage_target(s, a.rows.keysUn + off, a.rows.desc + (size_t)off * 32, N, a.cam, s_wtot);
}

// One direction (:1148-1225 / :1228-1305): the map points of the source keyframe (rows off .. off + N - 1, pose Tsw) through (sR, t) into the staged target.
// m_src[i] is kSkip for an already matched point and receives bestIdx.
__device__ void search_direction(const Sim3MatchArgs& a, const Lds& s, const float* s_scale, int off, int N, const float* Tsw, const float* sR, const float* t,
                                 float th, int* m_src) {
    float Rs[9], ts[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int k = 0; k < 3; k++) Rs[3 * r + k] = Tsw[4 * r + k];
        ts[r] = Tsw[4 * r + 3];
    }
    for (int i = threadIdx.x; i < N; i += kThreads) {
        const size_t o = (size_t)off + i;
        if (!a.rows.has_mp[o] || m_src[i] == kSkip) continue;
        const float X[3] = {a.rows.Xw[3 * o], a.rows.Xw[3 * o + 1], a.rows.Xw[3 * o + 2]};
        const float Ps[3] = {gemm_row(Rs, X, ts[0]), gemm_row(Rs + 3, X, ts[1]), gemm_row(Rs + 6, X, ts[2])};
        const float Pt[3] = {gemm_row(sR, Ps, t[0]), gemm_row(sR + 3, Ps, t[1]), gemm_row(sR + 6, Ps, t[2])};
        if (Pt[2] < 0.0f) continue;
        const float invz = (float)(1.0 / (double)Pt[2]);
        const float x = Pt[0] * invz, y = Pt[1] * invz;
        const float u = a.cam.fx * x + a.cam.cx, v = a.cam.fy * y + a.cam.cy;
        if (!(u >= a.cam.minX && u < a.cam.maxX && v >= a.cam.minY && v < a.cam.maxY)) continue;   // KeyFrame::IsInImage (src/KeyFrame.cc:610)
        const float mfMax = a.rows.maxDistance[o];
        const float maxDistance = 1.2f * mfMax, minDistance = 0.8f * a.rows.minDistance[o];
        const float dist3D = (float)sqrt(((double)Pt[0] * (double)Pt[0] + (double)Pt[1] * (double)Pt[1]) + (double)Pt[2] * (double)Pt[2]);   // cv::norm
        if (dist3D < minDistance || dist3D > maxDistance) continue;
        const int level = predict_level(mfMax, dist3D, a.cam);
        const Nearest best = nearest_in_window<-1, 0>(s, a.cam, u, v, th * s_scale[level], level, a.rows.mp_desc + o * 32);
        if (best.dist <= kThHigh) m_src[i] = best.idx;
    }
}

__global__ __launch_bounds__(kThreads) void k_search_by_sim3(Sim3MatchArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const oslam_sim3_pair_t& P = a.pairs[b];
    const int n1 = P.n1, off1 = P.off1, n2 = P.n2, off2 = P.off2, out_off = P.out_off;
    // a record that does not fit the handle or the arrays: -2, nothing else is written (the host-pointer entry point refuses the call instead)
    if (n1 < 0 || n2 < 0 || n1 > a.ncap || n2 > a.ncap || off1 < 0 || off2 < 0 || out_off < 0 || off1 > a.n_rows - n1 || off2 > a.n_rows - n2 || out_off > a.n_out - n1) {
        if (tid == 0) a.n_found[b] = -2;
        return;
    }
    int32_t* match12 = a.match12 + out_off;
    const float s12 = P.s12;
    if (!(isfinite(s12) && s12 > 0.0f && finite_all(P.R12, 9) && finite_all(P.t12, 3) && finite_all(P.T1w, 16) && finite_all(P.T2w, 16))) {
        for (int i = tid; i < n1; i += kThreads) match12[i] = -1;
        if (tid == 0) a.n_found[b] = -1;
        return;
    }

    extern __shared__ __align__(16) uint8_t smem[];
    const Lds s = carve(smem, a.ncap);
    int* const m1 = s.v0;   // [ncap] vnMatch1 (kSkip: vbAlreadyMatched1)
    int* const m2 = s.v1;   // [ncap] vnMatch2 (kSkip: vbAlreadyMatched2)
    __shared__ int s_wtot[kThreads / 64];
    __shared__ float s_scale[OSLAM_MAX_LEVELS];
    __shared__ int s_nfound;

    // sR12 = s12 * R12, sR21 = (1.0 / s12) * R12^T: one rounding of the double product; t21 = -sR21 * t12: a gemm with alpha = -1 (:1119-1121)
    float sR12[9], sR21[9], t21[3];
    const double inv = 1.0 / (double)s12;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            sR12[3 * i + j] = (float)((double)s12 * (double)P.R12[3 * i + j]);
            sR21[3 * i + j] = (float)(inv * (double)P.R12[3 * j + i]);
        }
#pragma unroll
    for (int i = 0; i < 3; i++) t21[i] = -(sR21[3 * i] * P.t12[0] + sR21[3 * i + 1] * P.t12[1] + sR21[3 * i + 2] * P.t12[2]);

    // vbAlreadyMatched1 / 2 (:1129-1142), vnMatch1 / 2 (:1144-1145)
    if (tid < OSLAM_MAX_LEVELS) s_scale[tid] = a.cam.scale[tid];
    if (tid == 0) s_nfound = 0;
    for (int i = tid; i < n2; i += kThreads) m2[i] = -1;
    __syncthreads();
    for (int i = tid; i < n1; i += kThreads) {
        const int idx2 = a.matched_in ? a.matched_in[out_off + i] : -1;
        m1[i] = idx2 != -1 ? kSkip : -1;
        if (idx2 >= 0 && idx2 < n2) m2[idx2] = kSkip;   // (-2, other negative values and >= n2: matched, but not a keypoint of KF2)
    }
    // (stage_target begins with a barrier)
    stage_rows(a, s, off2, n2, s_wtot);
    search_direction(a, s, s_scale, off1, n1, P.T1w, sR21, t21, P.th, m1);
    stage_rows(a, s, off1, n1, s_wtot);
    search_direction(a, s, s_scale, off2, n2, P.T2w, sR12, P.t12, P.th, m2);
    __syncthreads();
    // agreement (:1308-1323)
    int found = 0;
    for (int i1 = tid; i1 < n1; i1 += kThreads) {
        const int idx2 = m1[i1];
        const bool ok = idx2 >= 0 && m2[idx2] == i1;
        match12[i1] = ok ? idx2 : -1;
        found += ok ? 1 : 0;
    }
    if (found) atomicAdd(&s_nfound, found);
    __syncthreads();
    if (tid == 0) a.n_found[b] = s_nfound;
}

int check_call(const char* fn, const oslam_sim3_match* h, int n_pairs, const oslam_sim3_match_rows_t* rows, int n_out, const oslam_camera_t* cam, const float* bounds,
               const float* scaleFactors, int nlevels, float logScaleFactor) {
    if (!h || !rows || !cam || !bounds || !scaleFactors) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    if (n_pairs < 0 || rows->n_rows < 0 || n_out < 0) { set_error("%s: %d pairs, %d rows, %d output rows: none may be negative", fn, n_pairs, rows->n_rows, n_out); return OSLAM_E_CAPACITY; }
    if (n_pairs > h->max_pairs) { set_error("%s: %d pairs exceed the handle's %d", fn, n_pairs, h->max_pairs); return OSLAM_E_CAPACITY; }
    OSLAM_CHECK(check_window(fn, bounds, nlevels, logScaleFactor));
    if (rows->n_rows > 0 && (!rows->keysUn || !rows->desc || !rows->has_mp || !rows->Xw || !rows->mp_desc || !rows->maxDistance || !rows->minDistance)) {
        set_error("%s: a per-keypoint array is NULL", fn);
        return OSLAM_E_INVALID;
    }
    return OSLAM_OK;
}

}  // namespace

extern "C" {

void oslam_sim3_match_destroy(oslam_sim3_match_t* h) {
    if (!h) return;
    delete h;
}

int oslam_sim3_match_create(oslam_sim3_match_t** out, int max_pairs, int max_keypoints, int device) {
    if (!out) { set_error("oslam_sim3_match_create: out is NULL"); return OSLAM_E_INVALID; }
    *out = nullptr;
    if (max_pairs < 1 || max_keypoints < 1) { set_error("oslam_sim3_match_create: bad argument"); return OSLAM_E_INVALID; }
    OSLAM_CHECK(check_max_keypoints("oslam_sim3_match_create", max_keypoints, "one keyframe's", "both match vectors"));
    const int ndev = oslam_device_count();
    if (ndev <= 0) return oslam::no_device("oslam_sim3_match_create");
    if (device < 0 || device >= ndev) { set_error("oslam_sim3_match_create: device out of range"); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(device));
    oslam_sim3_match* h = new oslam_sim3_match;
    h->device = device; h->max_pairs = max_pairs; h->max_kps = max_keypoints; h->lds = lds_bytes(max_keypoints);
    const int rc = allow_full_lds("oslam_sim3_match_create", {(const void*)k_search_by_sim3});
    if (rc != OSLAM_OK) { delete h; return rc; }
    *out = h;
    return OSLAM_OK;
}

int oslam_match_search_by_sim3_batch_device(oslam_sim3_match_t* h, int n_pairs, const oslam_sim3_pair_t* d_pairs, const oslam_sim3_match_rows_t* rows, int n_out,
                                            const int32_t* d_matched_in, const oslam_camera_t* cam, const float bounds[4], const float* scaleFactors, int nlevels,
                                            float logScaleFactor, int32_t* d_match12, int32_t* d_n_found, void* stream) {
    const char* fn = "oslam_match_search_by_sim3_batch_device";
    OSLAM_CHECK(check_call(fn, h, n_pairs, rows, n_out, cam, bounds, scaleFactors, nlevels, logScaleFactor));
    if (n_pairs == 0) return OSLAM_OK;
    if (!d_pairs || !d_n_found || (n_out > 0 && !d_match12)) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    Sim3MatchArgs a;
    a.pairs = d_pairs; a.n_pairs = n_pairs; a.n_rows = rows->n_rows; a.n_out = n_out; a.ncap = h->max_kps;
    a.rows = *rows; a.matched_in = d_matched_in; a.match12 = d_match12; a.n_found = d_n_found;
    fill_window_cam(a.cam, cam, bounds, scaleFactors, nlevels, logScaleFactor);
    hipLaunchKernelGGL(k_search_by_sim3, dim3(n_pairs), dim3(kThreads), h->lds, (hipStream_t)stream, a);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int oslam_match_search_by_sim3_batch(oslam_sim3_match_t* h, int n_pairs, const oslam_sim3_pair_t* pairs, const oslam_sim3_match_rows_t* rows, int n_out,
                                     const int32_t* matched_in, const oslam_camera_t* cam, const float bounds[4], const float* scaleFactors, int nlevels,
                                     float logScaleFactor, int32_t* match12, int32_t* n_found) {
    const char* fn = "oslam_match_search_by_sim3_batch";
    OSLAM_CHECK(check_call(fn, h, n_pairs, rows, n_out, cam, bounds, scaleFactors, nlevels, logScaleFactor));
    if (n_pairs == 0) return OSLAM_OK;
    if (!pairs || !n_found || (n_out > 0 && !match12)) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    const int nr = rows->n_rows;
    for (int b = 0; b < n_pairs; b++) {
        const oslam_sim3_pair_t& P = pairs[b];
        if (P.n1 < 0 || P.n2 < 0 || P.n1 > h->max_kps || P.n2 > h->max_kps) {
            set_error("%s: pair %d has %d / %d keypoints, outside [0, %d]", fn, b, P.n1, P.n2, h->max_kps);
            return OSLAM_E_CAPACITY;
        }
        if (P.off1 < 0 || P.off2 < 0 || P.out_off < 0 || P.off1 > nr - P.n1 || P.off2 > nr - P.n2 || P.out_off > n_out - P.n1) {
            set_error("%s: pair %d (off1 %d, off2 %d, out_off %d) lies outside the %d rows / %d output rows", fn, b, P.off1, P.off2, P.out_off, nr, n_out);
            return OSLAM_E_INVALID;
        }
    }
    std::lock_guard<std::mutex> lock(h->mu);
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t np = (size_t)n_pairs, R = (size_t)nr, NO = (size_t)n_out;
    oslam::StageLayout lay;   // one block, inputs then outputs: one upload, one download
    const auto fPair = lay.add<oslam_sim3_pair_t>(np);
    const auto fKeys = lay.add<oslam_keypoint_t>(R);
    const auto fDesc = lay.add<uint8_t>(R * 32), fHas = lay.add<uint8_t>(R);
    const auto fXw = lay.add<float>(R * 3);
    const auto fMpd = lay.add<uint8_t>(R * 32);
    const auto fMax = lay.add<float>(R), fMin = lay.add<float>(R);
    const auto fIn = lay.add<int32_t>(NO, matched_in != nullptr);
    const auto fOut = lay.add<int32_t>(NO), fNf = lay.add<int32_t>(np);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fPair, ph, pairs); put(fKeys, ph, rows->keysUn); put(fDesc, ph, rows->desc); put(fHas, ph, rows->has_mp); put(fXw, ph, rows->Xw); put(fMpd, ph, rows->mp_desc);
    put(fMax, ph, rows->maxDistance); put(fMin, ph, rows->minDistance); put(fIn, ph, matched_in);
    // the caller's output rows travel too: rows no pair owns, and those of a pair the kernel leaves alone, come back as they were
    put(fOut, ph, match12); put(fNf, ph, n_found);
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, nullptr));
    oslam_sim3_match_rows_t d;
    d.n_rows = nr; d.keysUn = at(fKeys, pd); d.desc = at(fDesc, pd); d.has_mp = at(fHas, pd); d.Xw = at(fXw, pd); d.mp_desc = at(fMpd, pd);
    d.maxDistance = at(fMax, pd); d.minDistance = at(fMin, pd);
    OSLAM_CHECK(oslam_match_search_by_sim3_batch_device(h, n_pairs, at(fPair, pd), &d, n_out, at(fIn, pd), cam, bounds, scaleFactors, nlevels, logScaleFactor, at(fOut, pd),
                                                        at(fNf, pd), nullptr));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fOut.off, pd + fOut.off, lay.total() - fOut.off, hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(fOut, ph, match12); get(fNf, ph, n_found);
    return OSLAM_OK;
}

}  // extern "C"
