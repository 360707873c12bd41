// initializer.hip — Initializer::Initialize (src/Initializer.cc:44-121: H / F RANSAC, model selection, ReconstructH / ReconstructF) for batches of
// independent problems on gfx950 (include/oslam_hip.h, "Initializer").  Two launches per call: k_init_hypotheses — one workgroup per problem: validation,
// match compaction and Normalize once, then every (iteration, model) hypothesis by a group of 16 lanes — and k_init_reconstruct — one workgroup per
// problem: best iterations, RH, the motion hypotheses, CheckRT per inlier match, the decision.  The null-vector solves are fp64; the
// checks keep the reference's float arithmetic.  Product code; never includes oracle/.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <mutex>

#include "common.h"
#include "lane_ops.h"
#include "ransac_draw.h"
#include "small_svd.h"
#include "stage_layout.h"

using oslam::set_error;

struct oslam_init {
    int max_problems = 0, max_keys = 0, max_iterations = 0;
    // work arena: [problem][iteration][2][9] float, [problem][iteration][2] float, [problem][iteration][2] int32, [problem] int32,
    // and by compacted match: float4 (u1, v1, u2, v2), key-1 index, inlier byte of the chosen model, cosParallax
    oslam::DeviceBuffer hyp, score, count, nmatch, mxy, midx, inl, cosp;
    oslam::StagePair up, down;   // staging of the host-pointer entry point
    std::mutex mu;
    bool timing = false;         // oslam_init_set_timing: events before, between and after the two launches
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    ~oslam_init() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

namespace {

constexpr int kG = 16;           // lanes per hypothesis
constexpr int kBlock = 256;      // both kernels: four wavefronts
constexpr int kItsPerRound = 8;  // wavefronts 0, 1 take the homographies of eight iterations, wavefronts 2, 3 their fundamental matrices
constexpr int kNullSweeps = 12;  // one-sided Jacobi on the 16 x 9 system: fixed, so that NaN inputs cannot spin and every lane exchange is in uniform control flow
constexpr float kNoCos = 2.0f;   // cosParallax slot of a match that CheckRT did not count

struct InitArgs {
    const oslam_init_problem_t* problems;
    const float* k1; const int32_t* m12; const float* k2;
    int nk1, nk2;         // entries of the packed key arrays
    int it_stride;        // = params.max_iterations: row length of samples, of the dumps and of the arena
    oslam_init_params_t prm;
    const int32_t* samples;
    float* hyp; float* score; int32_t* count; int32_t* nmatch; float4* mxy; int32_t* midx; uint8_t* inl; float* cosp;   // arena
    float* R21; float* t21; float* P3D; uint8_t* tri; int32_t* status; float* scores;
    float* iter_scores; float* hypotheses; int32_t* iter_inliers; uint8_t* match_inliers;
};

__host__ __device__ inline bool problem_valid(const oslam_init_problem_t& pr, int nk1, int nk2) {
    return pr.n1 >= 0 && pr.off1 >= 0 && pr.n1 <= nk1 && pr.off1 <= nk1 - pr.n1 && pr.n2 >= 0 && pr.off2 >= 0 && pr.n2 <= nk2 && pr.off2 <= nk2 - pr.n2;
}

// ---- 3 x 3 helpers: products accumulate in fp64 and round once to the CV_32F the reference stores (cv::gemm of floats has a double accumulator) ----
__device__ inline void mul33(const float* A, const float* B, float* C) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[3 * i + j] = (float)((double)A[3 * i] * (double)B[j] + (double)A[3 * i + 1] * (double)B[3 + j] + (double)A[3 * i + 2] * (double)B[6 + j]);
}
// The inverse by cofactors in fp64, every quotient rounded to float: inv[i][j] = cofactor[j][i] / det.
__device__ inline void inv33(const float* M, float* out) {
    const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7], i = M[8];
    const double c00 = e * i - f * h, c01 = f * g - d * i, c02 = d * h - e * g;
    const double c10 = c * h - b * i, c11 = a * i - c * g, c12 = b * g - a * h;
    const double c20 = b * f - c * e, c21 = c * d - a * f, c22 = a * e - b * d;
    const double det = a * c00 + b * c01 + c * c02;
    out[0] = (float)(c00 / det); out[1] = (float)(c10 / det); out[2] = (float)(c20 / det);
    out[3] = (float)(c01 / det); out[4] = (float)(c11 / det); out[5] = (float)(c21 / det);
    out[6] = (float)(c02 / det); out[7] = (float)(c12 / det); out[8] = (float)(c22 / det);
}

// ---- the two checks for one match, in the reference's float arithmetic (the library is compiled without contraction) ----
// CheckHomography (:337-385): the two score terms (0 where the chi-square is above th) and the inlier bit.
__device__ __forceinline__ bool check_h(const float* H21, const float* H12, const float4 p, float invSigmaSquare, float& s1, float& s2) {
    const float th = 5.991f;
    const float u1 = p.x, v1 = p.y, u2 = p.z, v2 = p.w;
    bool bIn = true;
    const float w2in1inv = (float)(1.0 / (double)(H12[6] * u2 + H12[7] * v2 + H12[8]));
    const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
    const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) { bIn = false; s1 = 0.f; } else s1 = th - chiSquare1;
    const float w1in2inv = (float)(1.0 / (double)(H21[6] * u1 + H21[7] * v1 + H21[8]));
    const float u1in2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w1in2inv;
    const float v1in2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) { bIn = false; s2 = 0.f; } else s2 = th - chiSquare2;
    return bIn;
}
// CheckFundamental (:413-465)
__device__ __forceinline__ bool check_f(const float* F, const float4 p, float invSigmaSquare, float& s1, float& s2) {
    const float th = 3.841f, thScore = 5.991f;
    const float u1 = p.x, v1 = p.y, u2 = p.z, v2 = p.w;
    bool bIn = true;
    const float a2 = F[0] * u1 + F[1] * v1 + F[2];
    const float b2 = F[3] * u1 + F[4] * v1 + F[5];
    const float c2 = F[6] * u1 + F[7] * v1 + F[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) { bIn = false; s1 = 0.f; } else s1 = thScore - chiSquare1;
    const float a1 = F[0] * u2 + F[3] * v2 + F[6];
    const float b1 = F[1] * u2 + F[4] * v2 + F[7];
    const float c1 = F[2] * u2 + F[5] * v2 + F[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) { bIn = false; s2 = 0.f; } else s2 = thScore - chiSquare2;
    return bIn;
}
__device__ __forceinline__ float inv_sigma_square(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }

// ---- sums over the workgroup in a fixed order: thread t's partial, then a binary tree over LDS ----
__device__ inline void block_sum2(double& a, double& b, double (*red)[kBlock]) {
    const int t = threadIdx.x;
    red[0][t] = a; red[1][t] = b;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (t < s) { red[0][t] += red[0][t + s]; red[1][t] += red[1][t + s]; }
        __syncthreads();
    }
    a = red[0][0]; b = red[1][0];
    __syncthreads();
}
__device__ inline int block_sum_i32(int v, int* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const int r = red[0];
    __syncthreads();
    return r;
}

// The right singular vector of the smallest singular value of a 16 x 9 system by one-sided Jacobi rotations of its columns: lane c of the group holds
// row c of the system in B and, for c < 9, row c of V.  Every lane returns the vector (unit norm, its component of largest magnitude positive, the first
// of equals).  All lanes of the wavefront call it together.
__device__ inline void null9(double (&B)[9], int c, double (&nv)[9]) {
    double V[9];
#pragma unroll
    for (int j = 0; j < 9; j++) V[j] = c == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kNullSweeps; sweep++) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
#pragma unroll
            for (int j = i + 1; j < 9; j++) {
                const double a = oslam::row16_sum(B[i] * B[i]), b = oslam::row16_sum(B[j] * B[j]), g = oslam::row16_sum(B[i] * B[j]);
                if (fabs(g) > DBL_EPSILON * sqrt(a * b)) {   // (the same in all lanes of the group; only register arithmetic inside)
                    const double zeta = (b - a) / (2.0 * g);
                    const double t = (zeta < 0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                    const double bi = B[i], bj = B[j];
                    B[i] = cs * bi - sn * bj; B[j] = sn * bi + cs * bj;
                    const double vi = V[i], vj = V[j];
                    V[i] = cs * vi - sn * vj; V[j] = sn * vi + cs * vj;
                }
            }
        }
    }
    double best = oslam::row16_sum(B[0] * B[0]);
    double mine = V[0];
#pragma unroll
    for (int j = 1; j < 9; j++) {
        const double n = oslam::row16_sum(B[j] * B[j]);
        if (n < best) { best = n; mine = V[j]; }
    }
    const int base = (threadIdx.x & 63) & ~(kG - 1);
    double lead = 0.0;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        nv[k] = __shfl(mine, base + k);
        if (fabs(nv[k]) > fabs(lead)) lead = nv[k];
    }
    if (lead < 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) nv[k] = -nv[k];
    }
}

// One workgroup per problem.  Preparation once: validation (normalisation 5), the matches compacted in key-1 order, Normalize of both key sets; then
// rounds of eight iterations: wavefronts 0 and 1 compute their homographies, wavefronts 2 and 3 their fundamental matrices, 16 lanes per hypothesis.
__global__ __launch_bounds__(kBlock) void k_init_hypotheses(InitArgs a) {
    __shared__ double s_red[2][kBlock];
    __shared__ int s_wcnt[kBlock / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const oslam_init_problem_t pr = a.problems[b];
    if (!problem_valid(pr, a.nk1, a.nk2)) return;
    const float* k1 = a.k1 + 2 * (size_t)pr.off1;
    const float* k2 = a.k2 + 2 * (size_t)pr.off2;
    const int32_t* m12 = a.m12 + pr.off1;
    {
        int bad = (isfinite(pr.fx) && isfinite(pr.fy) && isfinite(pr.cx) && isfinite(pr.cy) && isfinite(pr.sigma)) ? 0 : 1;
        for (int i = tid; i < pr.n1; i += kBlock) bad |= (isfinite(k1[2 * i]) && isfinite(k1[2 * i + 1]) && m12[i] < pr.n2) ? 0 : 1;
        for (int i = tid; i < pr.n2; i += kBlock) bad |= (isfinite(k2[2 * i]) && isfinite(k2[2 * i + 1])) ? 0 : 1;
        if (__syncthreads_or(bad)) { if (tid == 0) a.nmatch[b] = -1; return; }
    }
    // mvMatches12 (:54-63): a prefix scan over the key-1 order, 256 entries at a time
    float4* mxy = a.mxy + pr.off1;
    int32_t* midx = a.midx + pr.off1;
    int N = 0;
    for (int base = 0; base < pr.n1; base += kBlock) {
        const int i = base + tid;
        const int m = i < pr.n1 ? m12[i] : -1;
        const unsigned long long bal = __ballot(m >= 0);
        const int lane = tid & 63, w = tid >> 6;
        if (lane == 0) s_wcnt[w] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kBlock / 64; k++) { before += k < w ? s_wcnt[k] : 0; total += s_wcnt[k]; }
        if (m >= 0) {
            const int at = N + before + __popcll(bal & ((1ull << lane) - 1ull));
            mxy[at] = make_float4(k1[2 * i], k1[2 * i + 1], k2[2 * m], k2[2 * m + 1]);
            midx[at] = i;
        }
        N += total;
        __syncthreads();
    }
    if (tid == 0) a.nmatch[b] = N;
    if (N < 8) return;   // normalisation 2
    // Normalize (:749-795) of ALL keys of each frame: every term in float, the sums in fp64 (normalisation 3)
    float mean[2][2], sc[2][2];
#pragma unroll
    for (int f = 0; f < 2; f++) {
        const float* k = f == 0 ? k1 : k2;
        const int n = f == 0 ? pr.n1 : pr.n2;
        double sx = 0.0, sy = 0.0;
        for (int i = tid; i < n; i += kBlock) { sx += (double)k[2 * i]; sy += (double)k[2 * i + 1]; }
        block_sum2(sx, sy, s_red);
        const float meanX = (float)sx / n, meanY = (float)sy / n;
        double dx = 0.0, dy = 0.0;
        for (int i = tid; i < n; i += kBlock) { dx += (double)fabsf(k[2 * i] - meanX); dy += (double)fabsf(k[2 * i + 1] - meanY); }
        block_sum2(dx, dy, s_red);
        const float meanDevX = (float)dx / n, meanDevY = (float)dy / n;
        mean[f][0] = meanX; mean[f][1] = meanY;
        sc[f][0] = (float)(1.0 / (double)meanDevX); sc[f][1] = (float)(1.0 / (double)meanDevY);
    }
    const float T1[9] = {sc[0][0], 0.f, -mean[0][0] * sc[0][0], 0.f, sc[0][1], -mean[0][1] * sc[0][1], 0.f, 0.f, 1.f};
    const float T2[9] = {sc[1][0], 0.f, -mean[1][0] * sc[1][0], 0.f, sc[1][1], -mean[1][1] * sc[1][1], 0.f, 0.f, 1.f};
    const float T2t[9] = {T2[0], 0.f, 0.f, 0.f, T2[4], 0.f, T2[2], T2[5], 1.f};
    float T2inv[9];
    inv33(T2, T2inv);
    const float invSigmaSquare = inv_sigma_square(pr.sigma);

    const int w = tid >> 6, model = w >> 1, gi = ((w & 1) << 2) | ((tid & 63) >> 4), c = tid & (kG - 1);
    const int its = a.prm.max_iterations;
    for (int first = 0; first < its; first += kItsPerRound) {
        const bool live = first + gi < its;
        const int it = live ? first + gi : its - 1;   // a spare group repeats the last iteration and writes nothing
        int idx[8];
        bool ok = true;
        if (a.samples) {
            const int32_t* s = a.samples + ((size_t)b * a.it_stride + it) * 8;
#pragma unroll
            for (int k = 0; k < 8; k++) { idx[k] = s[k]; ok = ok && idx[k] >= 0 && idx[k] < N; }
#pragma unroll
            for (int k = 0; k < 8; k++)
#pragma unroll
                for (int j = k + 1; j < 8; j++) ok = ok && idx[k] != idx[j];
        } else {
            oslam::ransac_draw<8>(pr.seed, it, N, idx);
        }
        // lane c holds row c of the system: for H rows 2 j and 2 j + 1 of point j (:239-257), for F row j of point j in lanes 0..7 and zero rows above (:281-289)
        const int j = model == 0 ? c >> 1 : c & 7;
        int mine = idx[0];
#pragma unroll
        for (int k = 1; k < 8; k++) if (j == k) mine = idx[k];
        if (!ok) mine = j;
        const float4 p = mxy[mine];
        const float u1 = (p.x - mean[0][0]) * sc[0][0], v1 = (p.y - mean[0][1]) * sc[0][1];   // vPn1, vPn2 (:771-787)
        const float u2 = (p.z - mean[1][0]) * sc[1][0], v2 = (p.w - mean[1][1]) * sc[1][1];
        double B[9];
        if (model == 0) {
            if ((c & 1) == 0) { B[0] = 0.0; B[1] = 0.0; B[2] = 0.0; B[3] = -u1; B[4] = -v1; B[5] = -1.0; B[6] = v2 * u1; B[7] = v2 * v1; B[8] = v2; }
            else { B[0] = u1; B[1] = v1; B[2] = 1.0; B[3] = 0.0; B[4] = 0.0; B[5] = 0.0; B[6] = -u2 * u1; B[7] = -u2 * v1; B[8] = -u2; }
        } else if (c < 8) {
            B[0] = u2 * u1; B[1] = u2 * v1; B[2] = u2; B[3] = v2 * u1; B[4] = v2 * v1; B[5] = v2; B[6] = u1; B[7] = v1; B[8] = 1.0;
        } else {
#pragma unroll
            for (int k = 0; k < 9; k++) B[k] = 0.0;
        }
        double nv[9];
        null9(B, c, nv);
        float M[9];   // H21i or F21i
        float H12[9];
        if (model == 0) {
            float Hn[9], t[9];
#pragma unroll
            for (int k = 0; k < 9; k++) Hn[k] = (float)nv[k];
            mul33(T2inv, Hn, t);
            mul33(t, T1, M);      // H21i = T2inv * Hn * T1 (:160)
            inv33(M, H12);        // H12i = H21i.inv() (:161)
        } else {
            double Fp[3][3], U[3][3], sv[3], V[3][3];
#pragma unroll
            for (int k = 0; k < 9; k++) Fp[k / 3][k % 3] = (double)(float)nv[k];   // Fpre is CV_32F
            oslam::svd3(Fp, U, sv, V);
            const int z = (sv[0] <= sv[1] && sv[0] <= sv[2]) ? 0 : (sv[1] <= sv[2] ? 1 : 2);   // w.at<float>(2) = 0 (:300)
            float Fn[9], t[9];
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    double e = 0.0;
#pragma unroll
                    for (int k = 0; k < 3; k++) e += k == z ? 0.0 : U[r][k] * sv[k] * V[q][k];
                    Fn[3 * r + q] = (float)e;
                }
            mul33(T2t, Fn, t);
            mul33(t, T1, M);      // F21i = T2t * Fn * T1 (:212)
        }
        // CheckHomography / CheckFundamental over all N matches: lane c takes matches c, c + 16, .. in order; the score is an fp64 sum rounded once
        double sum = 0.0;
        int cnt = 0;
        for (int i = c; i < N; i += kG) {
            float s1, s2;
            const bool in = model == 0 ? check_h(M, H12, mxy[i], invSigmaSquare, s1, s2) : check_f(M, mxy[i], invSigmaSquare, s1, s2);
            sum += (double)s1; sum += (double)s2;
            cnt += in ? 1 : 0;
        }
        float score = (float)oslam::row16_sum(sum);
        cnt = oslam::row16_sum_i32(cnt);
        if (!ok) { score = 0.f; cnt = 0; }
        if (live && c == 0) {
            const size_t o = ((size_t)b * a.it_stride + it) * 2 + model;
            a.score[o] = score; a.count[o] = cnt;
#pragma unroll
            for (int k = 0; k < 9; k++) a.hyp[o * 9 + k] = M[k];
            if (a.iter_scores) a.iter_scores[o] = score;
            if (a.iter_inliers) a.iter_inliers[o] = cnt;
            if (a.hypotheses) {
#pragma unroll
                for (int k = 0; k < 9; k++) a.hypotheses[o * 9 + k] = ok ? M[k] : __int_as_float(0x7fc00000);
            }
        }
    }
}

// ---- reconstruction ----
struct Motion { float R[9]; float t[3]; };

// What CheckRT derives from a motion (:814-826): P2 = K [R | t] and O2 = -R^T t.
struct RtCam { float fx, fy, cx, cy, th2; float R[9], t[3], P2[12], O2[3]; };
__device__ inline void rt_cam(const oslam_init_problem_t& pr, const Motion& m, RtCam& C) {
    C.fx = pr.fx; C.fy = pr.fy; C.cx = pr.cx; C.cy = pr.cy;
    C.th2 = (float)(4.0 * (double)(pr.sigma * pr.sigma));
#pragma unroll
    for (int k = 0; k < 9; k++) C.R[k] = m.R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) C.t[k] = m.t[k];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float r0 = k < 3 ? m.R[k] : m.t[0], r1 = k < 3 ? m.R[3 + k] : m.t[1], r2 = k < 3 ? m.R[6 + k] : m.t[2];
        C.P2[k] = (float)((double)pr.fx * (double)r0 + (double)pr.cx * (double)r2);
        C.P2[4 + k] = (float)((double)pr.fy * (double)r1 + (double)pr.cy * (double)r2);
        C.P2[8 + k] = r2;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) C.O2[k] = -(float)((double)m.R[k] * (double)m.t[0] + (double)m.R[3 + k] * (double)m.t[1] + (double)m.R[6 + k] * (double)m.t[2]);
}
// The body of CheckRT's loop for one inlier match (:835-893): whether it counts for nGood; then cosParallax and the point are valid.
__device__ inline bool check_rt_point(const RtCam& C, const float4 p, float& cosParallax, float (&X)[3]) {
    const float u1 = p.x, v1 = p.y, u2 = p.z, v2 = p.w;
    float A[16];   // Triangulate (:734-747); a row is x * P.row(2) - P.row(0), one rounding
    A[0] = -C.fx; A[1] = 0.f; A[2] = u1 - C.cx; A[3] = 0.f;
    A[4] = 0.f; A[5] = -C.fy; A[6] = v1 - C.cy; A[7] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        A[8 + k] = (float)((double)C.P2[8 + k] * (double)u2 - (double)C.P2[k]);
        A[12 + k] = (float)((double)C.P2[8 + k] * (double)v2 - (double)C.P2[4 + k]);
    }
    float v[4];
    oslam::svd4_last_row(A, v);
    const double invw = 1.0 / (double)v[3];
#pragma unroll
    for (int k = 0; k < 3; k++) X[k] = (float)((double)v[k] * invw);
    if (!isfinite(X[0]) || !isfinite(X[1]) || !isfinite(X[2])) return false;
    const float n2[3] = {X[0] - C.O2[0], X[1] - C.O2[1], X[2] - C.O2[2]};
    const float dist1 = (float)sqrt((double)X[0] * X[0] + (double)X[1] * X[1] + (double)X[2] * X[2]);
    const float dist2 = (float)sqrt((double)n2[0] * n2[0] + (double)n2[1] * n2[1] + (double)n2[2] * n2[2]);
    cosParallax = (float)(((double)X[0] * n2[0] + (double)X[1] * n2[1] + (double)X[2] * n2[2]) / (double)(dist1 * dist2));
    const bool low = (double)cosParallax < 0.99998;
    if (X[2] <= 0 && low) return false;
    float Y[3];   // p3dC2 = R * p3dC1 + t
#pragma unroll
    for (int k = 0; k < 3; k++) Y[k] = (float)((double)C.R[3 * k] * X[0] + (double)C.R[3 * k + 1] * X[1] + (double)C.R[3 * k + 2] * X[2] + (double)C.t[k]);
    if (Y[2] <= 0 && low) return false;
    const float invZ1 = (float)(1.0 / (double)X[2]);
    const float im1x = C.fx * X[0] * invZ1 + C.cx, im1y = C.fy * X[1] * invZ1 + C.cy;
    const float squareError1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);
    if (squareError1 > C.th2) return false;
    const float invZ2 = (float)(1.0 / (double)Y[2]);
    const float im2x = C.fx * Y[0] * invZ2 + C.cx, im2y = C.fy * Y[1] * invZ2 + C.cy;
    const float squareError2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);
    if (squareError2 > C.th2) return false;
    return true;
}

// column order of a 3 x 3 SVD by descending singular value, ties by index (cvSVD's order)
__device__ inline void order3(const double w[3], int ord[3]) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < 3; j++) rank += (w[j] > w[i] || (w[j] == w[i] && j < i)) ? 1 : 0;
#pragma unroll
        for (int r = 0; r < 3; r++) if (rank == r) ord[r] = i;
    }
}
__device__ inline double lead3(const double x[3]) {   // the component of largest magnitude, the first of equals
    const double a0 = fabs(x[0]), a1 = fabs(x[1]), a2 = fabs(x[2]);
    return (a0 >= a1 && a0 >= a2) ? x[0] : (a1 >= a2 ? x[1] : x[2]);
}

// DecomposeE (:909-929) and the four motions of ReconstructF (:479-497).  E has two equal singular values and a zero one: u.col(2) and vt.row(2) are taken
// as the cross products of the other two, which leaves both determinants at +1.  Normalisation 4: t has its component of largest magnitude positive and
// R1 is the rotation of larger trace.
__device__ inline int motions_f(const oslam_init_problem_t& pr, const float* F21, Motion* out) {
    const float K[9] = {pr.fx, 0.f, pr.cx, 0.f, pr.fy, pr.cy, 0.f, 0.f, 1.f};
    const float Kt[9] = {pr.fx, 0.f, 0.f, 0.f, pr.fy, 0.f, pr.cx, pr.cy, 1.f};
    float tmp[9], E[9];
    mul33(Kt, F21, tmp);
    mul33(tmp, K, E);
    double Ed[3][3], U[3][3], w[3], V[3][3];
#pragma unroll
    for (int k = 0; k < 9; k++) Ed[k / 3][k % 3] = E[k];
    oslam::svd3(Ed, U, w, V);
    int o[3];
    order3(w, o);
    double u[3][3], v[3][3];   // u[k] = k-th left vector, v[k] = k-th right vector
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 2; k++) {
            u[k][r] = o[k] == 0 ? U[r][0] : o[k] == 1 ? U[r][1] : U[r][2];
            v[k][r] = o[k] == 0 ? V[r][0] : o[k] == 1 ? V[r][1] : V[r][2];
        }
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1]; u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2]; u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    v[2][0] = v[0][1] * v[1][2] - v[0][2] * v[1][1]; v[2][1] = v[0][2] * v[1][0] - v[0][0] * v[1][2]; v[2][2] = v[0][0] * v[1][1] - v[0][1] * v[1][0];
    double t[3] = {u[2][0], u[2][1], u[2][2]};
    const double nt = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    const double sg = lead3(t) < 0 ? -1.0 : 1.0;
    // R1 = u W vt = u1 v0^T - u0 v1^T + u2 v2^T, R2 = u W^T vt = -u1 v0^T + u0 v1^T + u2 v2^T
    double R1[9], R2[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const double x = u[1][r] * v[0][q] - u[0][r] * v[1][q], y = u[2][r] * v[2][q];
            R1[3 * r + q] = x + y; R2[3 * r + q] = -x + y;
        }
    const bool swap = R2[0] + R2[4] + R2[8] > R1[0] + R1[4] + R1[8];
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const bool second = ((m & 1) != 0) != swap;
#pragma unroll
        for (int k = 0; k < 9; k++) out[m].R[k] = (float)(second ? R2[k] : R1[k]);
#pragma unroll
        for (int k = 0; k < 3; k++) out[m].t[k] = (float)((m < 2 ? sg : -sg) * t[k] / nt);
    }
    return 4;
}

// The eight motions of ReconstructH (:584-686), or 0 when the singular values are too close (:597-600).  Normalisation 4: every left singular vector has
// its component of largest magnitude positive, its right vector follows.
__device__ inline int motions_h(const oslam_init_problem_t& pr, const float* H21, Motion* out) {
    const float K[9] = {pr.fx, 0.f, pr.cx, 0.f, pr.fy, pr.cy, 0.f, 0.f, 1.f};
    float invK[9], tmp[9], A[9];
    inv33(K, invK);
    mul33(invK, H21, tmp);
    mul33(tmp, K, A);
    double Ad[3][3], U0[3][3], w0[3], V0[3][3];
#pragma unroll
    for (int k = 0; k < 9; k++) Ad[k / 3][k % 3] = A[k];
    oslam::svd3(Ad, U0, w0, V0);
    int o[3];
    order3(w0, o);
    double U[3][3], V[3][3], w[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double uc[3], vc[3];
#pragma unroll
        for (int r = 0; r < 3; r++) { uc[r] = o[k] == 0 ? U0[r][0] : o[k] == 1 ? U0[r][1] : U0[r][2]; vc[r] = o[k] == 0 ? V0[r][0] : o[k] == 1 ? V0[r][1] : V0[r][2]; }
        w[k] = o[k] == 0 ? w0[0] : o[k] == 1 ? w0[1] : w0[2];
        const double sg = lead3(uc) < 0 ? -1.0 : 1.0;
#pragma unroll
        for (int r = 0; r < 3; r++) { U[r][k] = sg * uc[r]; V[r][k] = sg * vc[r]; }
    }
    auto det = [](const double M[3][3]) {
        return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
    };
    const float s = (float)(det(U) * det(V));
    const float d1 = (float)w[0], d2 = (float)w[1], d3 = (float)w[2];
    if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return 0;
    float Uf[9], Vt[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) { Uf[3 * r + q] = (float)U[r][q]; Vt[3 * r + q] = (float)V[q][r]; }
    const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float x1[4] = {aux1, aux1, -aux1, -aux1};
    const float x3[4] = {aux3, -aux3, aux3, -aux3};
    const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const int i = m & 3;
        float Rp[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, tp[3];
        if (m < 4) {   // case d' = d2
            Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta;
            tp[0] = x1[i] * (d1 - d3); tp[1] = 0.f * (d1 - d3); tp[2] = -x3[i] * (d1 - d3);
        } else {       // case d' = -d2
            Rp[0] = cphi; Rp[2] = sphi[i]; Rp[4] = -1.f; Rp[6] = sphi[i]; Rp[8] = -cphi;
            tp[0] = x1[i] * (d1 + d3); tp[1] = 0.f * (d1 + d3); tp[2] = x3[i] * (d1 + d3);
        }
        float t1[9], t2[9];
        mul33(Uf, Rp, t1);
        mul33(t1, Vt, t2);
#pragma unroll
        for (int k = 0; k < 9; k++) out[m].R[k] = s * t2[k];
        float t[3];
#pragma unroll
        for (int r = 0; r < 3; r++) t[r] = (float)((double)Uf[3 * r] * (double)tp[0] + (double)Uf[3 * r + 1] * (double)tp[1] + (double)Uf[3 * r + 2] * (double)tp[2]);
        const double nt = sqrt((double)t[0] * t[0] + (double)t[1] * t[1] + (double)t[2] * t[2]);
#pragma unroll
        for (int r = 0; r < 3; r++) out[m].t[r] = (float)((double)t[r] / nt);
    }
    return 8;
}

// One workgroup per problem: the best iterations, the model, the motions, CheckRT of every motion, the decision, the outputs.
__global__ __launch_bounds__(kBlock) void k_init_reconstruct(InitArgs a) {
    __shared__ int s_red[kBlock];
    __shared__ float s_bs[kBlock];
    __shared__ Motion s_mot[8];
    __shared__ int s_nm, s_win, s_ret;
    __shared__ float s_cos;
    __shared__ int s_ng[8];
    __shared__ float s_par[8];
    const int b = blockIdx.x, tid = threadIdx.x;
    const oslam_init_problem_t pr = a.problems[b];
    int32_t* st = a.status + 8 * (size_t)b;
    float* sco = a.scores + 4 * (size_t)b;
    if (!problem_valid(pr, a.nk1, a.nk2)) { if (tid == 0) { st[0] = -1; st[1] = 0; st[2] = 0; st[3] = 0; st[4] = -1; st[5] = -1; st[6] = -1; st[7] = 0; } return; }
    const int N = a.nmatch[b];
    if (N < 8) {   // normalisations 2 and 5
        if (tid == 0) { st[0] = 0; st[1] = 0; st[2] = N < 0 ? 0 : N; st[3] = 0; st[4] = -1; st[5] = -1; st[6] = -1; st[7] = 0; sco[0] = 0.f; sco[1] = 0.f; sco[2] = 0.f; sco[3] = 0.f; }
        return;
    }
    const int its = a.prm.max_iterations;
    const size_t o = (size_t)b * a.it_stride * 2;
    // the first iteration of strictly highest score per model (:165, :216), from score = 0
    int bestIt[2];
    float bestS[2];
    for (int model = 0; model < 2; model++) {
        float bs = 0.f;
        int bi = -1;
        for (int it = tid; it < its; it += kBlock) { const float s = a.score[o + 2 * (size_t)it + model]; if (s > bs) { bs = s; bi = it; } }
        s_bs[tid] = bs; s_red[tid] = bi;
        __syncthreads();
        for (int s = kBlock / 2; s > 0; s >>= 1) {
            if (tid < s) {
                const float os = s_bs[tid + s];
                const int oi = s_red[tid + s];
                if (oi >= 0 && (os > s_bs[tid] || (os == s_bs[tid] && (s_red[tid] < 0 || oi < s_red[tid])))) { s_bs[tid] = os; s_red[tid] = oi; }
            }
            __syncthreads();
        }
        bestS[model] = s_bs[0]; bestIt[model] = s_red[0];
        __syncthreads();
    }
    const float SH = bestS[0], SF = bestS[1];
    const float RH = SH / (SH + SF);
    const bool useH = (double)RH > 0.40;   // anything else, NaN included, takes ReconstructF (:115-118)
    const int chosen = useH ? bestIt[0] : bestIt[1];
    float H21[9], H12[9], F21[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        H21[k] = bestIt[0] >= 0 ? a.hyp[(o + 2 * (size_t)bestIt[0]) * 9 + k] : 0.f;
        F21[k] = bestIt[1] >= 0 ? a.hyp[(o + 2 * (size_t)bestIt[1] + 1) * 9 + k] : 0.f;
    }
    inv33(H21, H12);
    const float invSigmaSquare = inv_sigma_square(pr.sigma);
    const float4* mxy = a.mxy + pr.off1;
    const int32_t* midx = a.midx + pr.off1;
    uint8_t* inl = a.inl + pr.off1;
    float* cosp = a.cosp + pr.off1;
    // vbMatchesInliersH / F of the best iterations; the chosen model's go to the arena by compacted match
    if (a.match_inliers) {
        for (int i = tid; i < pr.n1; i += kBlock) { a.match_inliers[2 * ((size_t)pr.off1 + i)] = 0; a.match_inliers[2 * ((size_t)pr.off1 + i) + 1] = 0; }
        __syncthreads();
    }
    int nin = 0;
    for (int i = tid; i < N; i += kBlock) {
        float s1, s2;
        const bool inH = bestIt[0] >= 0 && check_h(H21, H12, mxy[i], invSigmaSquare, s1, s2);
        const bool inF = bestIt[1] >= 0 && check_f(F21, mxy[i], invSigmaSquare, s1, s2);
        const bool in = useH ? inH : inF;
        inl[i] = in ? 1 : 0;
        nin += in ? 1 : 0;
        if (a.match_inliers) { a.match_inliers[2 * ((size_t)pr.off1 + midx[i])] = inH ? 1 : 0; a.match_inliers[2 * ((size_t)pr.off1 + midx[i]) + 1] = inF ? 1 : 0; }
    }
    nin = block_sum_i32(nin, s_red);   // N of ReconstructF / ReconstructH (:473-476, :575-578)
    if (tid == 0) {
        s_nm = chosen < 0 ? 0 : (useH ? motions_h(pr, H21, s_mot) : motions_f(pr, F21, s_mot));
        s_win = -1; s_ret = 0;
    }
    __syncthreads();
    const int nm = s_nm;
    for (int m = 0; m < nm; m++) {
        RtCam C;
        rt_cam(pr, s_mot[m], C);
        int good = 0;
        for (int i = tid; i < N; i += kBlock) {
            float cp = kNoCos, X[3];
            if (inl[i] && check_rt_point(C, mxy[i], cp, X)) good++; else cp = kNoCos;
            cosp[i] = cp;
        }
        const int ngm = block_sum_i32(good, s_red);   // (its barriers also publish cosp)
        float parm = 0.f;
        if (ngm > 0) {
            // sort, then element min(50, size - 1) (:898-901): the one with that many counted values before it, ties by match index
            const int want = ngm - 1 < 50 ? ngm - 1 : 50;
            if (tid == 0) s_cos = 1.f;
            __syncthreads();
            for (int i = tid; i < N; i += kBlock) {
                const float ci = cosp[i];
                if (!(ci < 1.5f)) continue;
                int rank = 0;
                for (int j = 0; j < N; j++) { const float cj = cosp[j]; rank += (cj < 1.5f && (cj < ci || (cj == ci && j < i))) ? 1 : 0; }
                if (rank == want) s_cos = ci;
            }
            __syncthreads();
            parm = (float)(acos((double)s_cos) * 180.0 / 3.1415926535897932384626433832795);
        }
        if (tid == 0) { s_ng[m] = ngm; s_par[m] = parm; }
        __syncthreads();
    }
    if (tid == 0) {
        const int* nGood = s_ng;
        const float* parallax = s_par;
        int win = -1, ret = 0, sel = 0, ng = 0;
        float par = 0.f;
        if (nm == 4) {   // ReconstructF (:499-569)
            int maxGood = 0;
            for (int m = 0; m < 4; m++) maxGood = nGood[m] > maxGood ? nGood[m] : maxGood;
            const int nMinGood = (int)(0.9 * nin) > a.prm.min_triangulated ? (int)(0.9 * nin) : a.prm.min_triangulated;
            for (int m = 0; m < 4; m++) sel += (double)nGood[m] > 0.7 * maxGood ? 1 : 0;
            ng = maxGood;
            for (int m = 3; m >= 0; m--) if (nGood[m] == maxGood) win = m;   // the first of the == cascade
            par = parallax[win];
            ret = !(maxGood < nMinGood || sel > 1) && par > a.prm.min_parallax;
        } else if (nm == 8) {   // ReconstructH (:689-731)
            int bestGood = 0, secondBestGood = 0;
            float bestParallax = -1.f;
            for (int m = 0; m < 8; m++) {
                if (nGood[m] > bestGood) { secondBestGood = bestGood; bestGood = nGood[m]; win = m; bestParallax = parallax[m]; }
                else if (nGood[m] > secondBestGood) secondBestGood = nGood[m];
            }
            sel = secondBestGood; ng = bestGood; par = bestParallax;
            ret = (double)secondBestGood < 0.75 * bestGood && bestParallax >= a.prm.min_parallax && bestGood > a.prm.min_triangulated && (double)bestGood > 0.9 * nin;
        }
        s_win = win; s_ret = ret;
        st[0] = ret; st[1] = useH ? 1 : 2; st[2] = N; st[3] = ng; st[4] = win; st[5] = bestIt[0]; st[6] = bestIt[1]; st[7] = sel;
        sco[0] = SH; sco[1] = SF; sco[2] = RH; sco[3] = par;
    }
    __syncthreads();
    if (!s_ret) return;   // the caller's R21, t21, P3D and triangulated stay
    const int win = s_win;
    float* P3D = a.P3D + 3 * (size_t)pr.off1;
    uint8_t* tri = a.tri + pr.off1;
    for (int i = tid; i < pr.n1; i += kBlock) { P3D[3 * i] = 0.f; P3D[3 * i + 1] = 0.f; P3D[3 * i + 2] = 0.f; tri[i] = 0; }   // vP3D.resize, vbGood(size, false) (:808-809)
    __syncthreads();
    RtCam C;
    rt_cam(pr, s_mot[win], C);
    for (int i = tid; i < N; i += kBlock) {
        float cp, X[3];
        if (!inl[i] || !check_rt_point(C, mxy[i], cp, X)) continue;
        const int k = midx[i];
        P3D[3 * k] = X[0]; P3D[3 * k + 1] = X[1]; P3D[3 * k + 2] = X[2];   // (:889)
        if ((double)cp < 0.99998) tri[k] = 1;                                // (:892-893)
    }
    if (tid < 9) a.R21[9 * (size_t)b + tid] = s_mot[win].R[tid];
    if (tid < 3) a.t21[3 * (size_t)b + tid] = s_mot[win].t[tid];
}

int check_call(const char* fn, const oslam_init* h, int n_problems, int nk1, int nk2, const oslam_init_params_t* p) {
    if (!p) { set_error("%s: params is NULL", fn); return OSLAM_E_INVALID; }
    if (p->max_iterations < 1 || !(p->min_parallax >= 0.f) || p->min_triangulated < 0) { set_error("%s: bad parameter block", fn); return OSLAM_E_INVALID; }
    if (p->max_iterations > h->max_iterations || n_problems > h->max_problems || nk1 > h->max_keys || nk2 > h->max_keys) {
        set_error("%s: %d problems / %d + %d keys / %d iterations exceed the handle's %d / %d / %d", fn, n_problems, nk1, nk2, p->max_iterations, h->max_problems, h->max_keys,
                  h->max_iterations);
        return OSLAM_E_CAPACITY;
    }
    return OSLAM_OK;
}

}  // namespace

extern "C" {

int oslam_init_draw(uint32_t seed, int iteration, int N, int32_t idx[8]) {
    if (!idx || N < 8 || iteration < 0) { set_error("oslam_init_draw: bad argument"); return OSLAM_E_INVALID; }
    int v[8];
    oslam::ransac_draw<8>(seed, iteration, N, v);
    for (int k = 0; k < 8; k++) idx[k] = v[k];
    return OSLAM_OK;
}

void oslam_init_destroy(oslam_init_t* h) {
    if (!h) return;
    delete h;
}

int oslam_init_create(oslam_init_t** out, int max_problems, int max_keys_total, int max_iterations) {
    if (!out) { set_error("oslam_init_create: out is NULL"); return OSLAM_E_INVALID; }
    *out = nullptr;
    if (max_problems < 1 || max_keys_total < 1 || max_iterations < 1) { set_error("oslam_init_create: bad argument"); return OSLAM_E_INVALID; }
    if (oslam_device_count() <= 0) return oslam::no_device("oslam_init_create");
    oslam_init* h = new oslam_init;
    h->max_problems = max_problems; h->max_keys = max_keys_total; h->max_iterations = max_iterations;
    const size_t hyp = (size_t)max_problems * max_iterations * 2, nk = (size_t)max_keys_total;
    int rc;
    if ((rc = h->hyp.alloc(hyp * 9 * sizeof(float))) || (rc = h->score.alloc(hyp * sizeof(float))) || (rc = h->count.alloc(hyp * sizeof(int32_t))) ||
        (rc = h->nmatch.alloc((size_t)max_problems * sizeof(int32_t))) || (rc = h->mxy.alloc(nk * sizeof(float4))) || (rc = h->midx.alloc(nk * sizeof(int32_t))) ||
        (rc = h->inl.alloc(nk)) || (rc = h->cosp.alloc(nk * sizeof(float)))) {
        delete h;
        return rc;
    }
    *out = h;
    return OSLAM_OK;
}

int oslam_init_set_timing(oslam_init_t* h, int on) {
    if (!h) { set_error("oslam_init_set_timing: handle is NULL"); return OSLAM_E_INVALID; }
    if (on)
        for (hipEvent_t& e : h->ev) if (!e) OSLAM_HIP_CHECK(hipEventCreate(&e));
    h->timing = on != 0;
    return OSLAM_OK;
}

int oslam_init_last_kernel_ms(oslam_init_t* h, float ms[2]) {
    if (!h || !ms || !h->timing) { set_error("oslam_init_last_kernel_ms: timing is not on"); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipEventSynchronize(h->ev[2]));
    OSLAM_HIP_CHECK(hipEventElapsedTime(&ms[0], h->ev[0], h->ev[1]));
    OSLAM_HIP_CHECK(hipEventElapsedTime(&ms[1], h->ev[1], h->ev[2]));
    return OSLAM_OK;
}

int oslam_init_initialize_batch_device(oslam_init_t* h, int n_problems, const oslam_init_problem_t* d_problems, int n_keys1, const float* d_keys1, const int32_t* d_matches12,
                                       int n_keys2, const float* d_keys2, const oslam_init_params_t* params, const int32_t* d_samples, float* d_R21, float* d_t21, float* d_P3D,
                                       uint8_t* d_triangulated, int32_t* d_status, float* d_scores, float* d_iter_scores, float* d_hypotheses, int32_t* d_iter_inliers,
                                       uint8_t* d_match_inliers, void* stream) {
    if (!h || n_problems < 0 || n_keys1 < 0 || n_keys2 < 0 || (n_problems > 0 && (!d_problems || !d_R21 || !d_t21 || !d_status || !d_scores)) ||
        (n_keys1 > 0 && (!d_keys1 || !d_matches12 || !d_P3D || !d_triangulated)) || (n_keys2 > 0 && !d_keys2)) {
        set_error("oslam_init_initialize_batch_device: bad argument");
        return OSLAM_E_INVALID;
    }
    OSLAM_CHECK(check_call("oslam_init_initialize_batch_device", h, n_problems, n_keys1, n_keys2, params));
    if (n_problems == 0) return OSLAM_OK;
    InitArgs a;
    a.problems = d_problems; a.k1 = d_keys1; a.m12 = d_matches12; a.k2 = d_keys2; a.nk1 = n_keys1; a.nk2 = n_keys2; a.it_stride = params->max_iterations; a.prm = *params;
    a.samples = d_samples;
    a.hyp = h->hyp.as<float>(); a.score = h->score.as<float>(); a.count = h->count.as<int32_t>(); a.nmatch = h->nmatch.as<int32_t>(); a.mxy = h->mxy.as<float4>();
    a.midx = h->midx.as<int32_t>(); a.inl = h->inl.as<uint8_t>(); a.cosp = h->cosp.as<float>();
    a.R21 = d_R21; a.t21 = d_t21; a.P3D = d_P3D; a.tri = d_triangulated; a.status = d_status; a.scores = d_scores;
    a.iter_scores = d_iter_scores; a.hypotheses = d_hypotheses; a.iter_inliers = d_iter_inliers; a.match_inliers = d_match_inliers;
    if (h->timing) OSLAM_HIP_CHECK(hipEventRecord(h->ev[0], (hipStream_t)stream));
    hipLaunchKernelGGL(k_init_hypotheses, dim3(n_problems), dim3(kBlock), 0, (hipStream_t)stream, a);
    if (h->timing) OSLAM_HIP_CHECK(hipEventRecord(h->ev[1], (hipStream_t)stream));
    hipLaunchKernelGGL(k_init_reconstruct, dim3(n_problems), dim3(kBlock), 0, (hipStream_t)stream, a);
    if (h->timing) OSLAM_HIP_CHECK(hipEventRecord(h->ev[2], (hipStream_t)stream));
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int oslam_init_initialize_batch(oslam_init_t* h, int n_problems, const oslam_init_problem_t* problems, int n_keys1, const float* keys1, const int32_t* matches12, int n_keys2,
                                const float* keys2, const oslam_init_params_t* params, const int32_t* samples, float* R21, float* t21, float* P3D, uint8_t* triangulated,
                                int32_t* status, float* scores, float* iter_scores, float* hypotheses, int32_t* iter_inliers, uint8_t* match_inliers) {
    if (!h || n_problems < 0 || n_keys1 < 0 || n_keys2 < 0 || (n_problems > 0 && (!problems || !R21 || !t21 || !status || !scores)) ||
        (n_keys1 > 0 && (!keys1 || !matches12 || !P3D || !triangulated)) || (n_keys2 > 0 && !keys2)) {
        set_error("oslam_init_initialize_batch: bad argument");
        return OSLAM_E_INVALID;
    }
    OSLAM_CHECK(check_call("oslam_init_initialize_batch", h, n_problems, n_keys1, n_keys2, params));
    for (int b = 0; b < n_problems; b++)
        if (!problem_valid(problems[b], n_keys1, n_keys2)) {
            set_error("oslam_init_initialize_batch: problem %d (keys 1 %d + %d, keys 2 %d + %d) lies outside the %d / %d keys", b, problems[b].off1, problems[b].n1, problems[b].off2,
                      problems[b].n2, n_keys1, n_keys2);
            return OSLAM_E_INVALID;
        }
    if (n_problems == 0) return OSLAM_OK;
    std::lock_guard<std::mutex> lock(h->mu);
    const size_t np = (size_t)n_problems, n1 = (size_t)n_keys1, n2 = (size_t)n_keys2, its = (size_t)params->max_iterations;
    oslam::StageLayout up, down;   // one upload, one download
    const auto uProb = up.add<oslam_init_problem_t>(np);
    const auto uK1 = up.add<float>(n1 * 2), uK2 = up.add<float>(n2 * 2);
    const auto uM = up.add<int32_t>(n1);
    const auto uSam = up.add<int32_t>(np * its * 8, samples != nullptr);
    const auto dSt = down.add<int32_t>(np * 8);
    const auto dSc = down.add<float>(np * 4);
    const auto dR = down.add<float>(np * 9), dT = down.add<float>(np * 3);
    const auto dP = down.add<float>(n1 * 3);
    const auto dTri = down.add<uint8_t>(n1);
    const auto dIS = down.add<float>(np * its * 2, iter_scores != nullptr);
    const auto dHy = down.add<float>(np * its * 18, hypotheses != nullptr);
    const auto dII = down.add<int32_t>(np * its * 2, iter_inliers != nullptr);
    const auto dMI = down.add<uint8_t>(n1 * 2, match_inliers != nullptr);
    OSLAM_CHECK(h->up.grow(up.total(), 4096));
    OSLAM_CHECK(h->down.grow(down.total(), 4096));
    uint8_t *uh = h->up.h.bytes(), *ud = h->up.d.bytes(), *dh = h->down.h.bytes(), *dd = h->down.d.bytes();
    put(uProb, uh, problems); put(uK1, uh, keys1); put(uK2, uh, keys2); put(uM, uh, matches12); put(uSam, uh, samples);
    OSLAM_HIP_CHECK(hipMemcpyAsync(ud, uh, up.total(), hipMemcpyHostToDevice, nullptr));
    // dumps of what is not run: NaN scores and matrices, -1 counts, no inliers
    if (iter_scores) OSLAM_HIP_CHECK(hipMemsetAsync(at(dIS, dd), 0xff, dIS.bytes, nullptr));
    if (hypotheses) OSLAM_HIP_CHECK(hipMemsetAsync(at(dHy, dd), 0xff, dHy.bytes, nullptr));
    if (iter_inliers) OSLAM_HIP_CHECK(hipMemsetAsync(at(dII, dd), 0xff, dII.bytes, nullptr));
    if (match_inliers && dMI.bytes) OSLAM_HIP_CHECK(hipMemsetAsync(at(dMI, dd), 0, dMI.bytes, nullptr));
    if (dSc.bytes) OSLAM_HIP_CHECK(hipMemsetAsync(at(dSc, dd), 0, dSc.bytes, nullptr));
    OSLAM_CHECK(oslam_init_initialize_batch_device(h, n_problems, at(uProb, ud), n_keys1, at(uK1, ud), at(uM, ud), n_keys2, at(uK2, ud), params, at(uSam, ud), at(dR, dd), at(dT, dd),
                                                   at(dP, dd), at(dTri, dd), at(dSt, dd), at(dSc, dd), at(dIS, dd), at(dHy, dd), at(dII, dd), at(dMI, dd), nullptr));
    OSLAM_HIP_CHECK(hipMemcpyAsync(dh, dd, down.total(), hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(dSt, dh, status); get(dSc, dh, scores); get(dIS, dh, iter_scores); get(dHy, dh, hypotheses); get(dII, dh, iter_inliers); get(dMI, dh, match_inliers);
    for (int b = 0; b < n_problems; b++) {   // a problem that does not return keeps the caller's R21, t21, P3D and triangulated
        if (status[8 * b] != 1) continue;
        memcpy(R21 + 9 * (size_t)b, at(dR, dh) + 9 * (size_t)b, 9 * sizeof(float));
        memcpy(t21 + 3 * (size_t)b, at(dT, dh) + 3 * (size_t)b, 3 * sizeof(float));
        memcpy(P3D + 3 * (size_t)problems[b].off1, at(dP, dh) + 3 * (size_t)problems[b].off1, 3 * sizeof(float) * (size_t)problems[b].n1);
        memcpy(triangulated + problems[b].off1, at(dTri, dh) + problems[b].off1, (size_t)problems[b].n1);
    }
    return OSLAM_OK;
}

}  // extern "C"
