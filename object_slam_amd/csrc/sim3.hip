// sim3.hip — Sim3Solver (src/Sim3Solver.cc: Horn's closed form inside RANSAC) for batches of independent problems on gfx950 (include/oslam_hip.h,
// "Sim3 solver").  Two launches per call: k_sim3_hypotheses computes every (problem, iteration of the chunk) hypothesis — 16 lanes each, four per
// wavefront: Horn once, then the lanes stride over the correspondences — and k_sim3_select replays iterate()'s control flow over the counts, 16 lanes
// per problem, and updates the state records.  Horn is fp64 from the float inputs, rounded to float where the reference stores
// CV_32F; T12, T21 and the projections are float.  Product code; never includes oracle/.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <mutex>

#include "common.h"
#include "lane_ops.h"
#include "ransac_draw.h"
#include "stage_layout.h"

using oslam::set_error;

struct oslam_sim3 {
    int max_problems = 0, max_corr = 0, max_iterations = 0;
    oslam::DeviceBuffer hyp, counts;   // work arena: [problem][iteration][13] float, [problem][iteration] int32
    oslam::StagePair io;               // staging of the host-pointer entry point: inputs | states | outputs
    std::mutex mu;
};

namespace {

constexpr int kG = 16;             // lanes per hypothesis / per problem of the select kernel
constexpr int kPerBlock = 4;       // one wavefront
constexpr int kJacobiSweeps = 10;  // cyclic Jacobi on the 4 x 4 matrix N: fixed, so that NaN inputs cannot spin

struct Sim3Ransac { int iterations; int no_more; };

// SetRansacParameters (src/Sim3Solver.cc:114-138) with its mixed arithmetic; the same text runs on the host and in the kernels.
__host__ __device__ inline Sim3Ransac ransac_adjust(int N, double probability, int minInliers, int maxIterations) {
    Sim3Ransac r;
    r.no_more = (N < minInliers || N < 3) ? 1 : 0;   // iterate() returns before its loop (:146-150); N < 3: normalisation 4
    r.iterations = 0;
    if (r.no_more) return r;
    int nIterations;
    if (minInliers == N) nIterations = 1;
    else {
        const float epsilon = (float)minInliers / N;
        const double d = ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3.0)));
        nIterations = d >= (double)maxIterations ? maxIterations : d >= 1.0 ? (int)d : 1;   // (NaN and -inf: max(1, .) of the reference)
    }
    if (nIterations > maxIterations) nIterations = maxIterations;
    r.iterations = nIterations < 1 ? 1 : nIterations;
    return r;
}

struct Sim3Hyp { float R[9], t[3], s; };      // mR12i, mt12i, ms12i
struct Sim3T { float a12[12], a21[12]; };     // the first three rows of mT12i and mT21i

// Symmetric 4 x 4 eigen-decomposition by cyclic Jacobi in registers: A's diagonal becomes the eigenvalues, V's columns the eigenvectors.
__device__ inline void jacobi4(double (&A)[4][4], double (&V)[4][4]) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
#pragma unroll
        for (int pr = 0; pr < 6; pr++) {
            const int p = pr < 3 ? 0 : pr < 5 ? 1 : 2, q = pr < 3 ? pr + 1 : pr < 5 ? pr - 1 : 3;
            const double apq = A[p][q];
            if (apq != 0.0) {
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta < 0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
                }
                A[p][q] = 0.0; A[q][p] = 0.0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
                }
            }
        }
    }
}

// ComputeSim3 (:226-316) on the correspondences idx[0..2].
__device__ inline Sim3Hyp compute_sim3(const float* X1, const float* X2, const int idx[3], bool fix_scale) {
    double P1[3][3], P2[3][3], O1[3], O2[3];   // [point][coordinate]
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int c = 0; c < 3; c++) { P1[k][c] = X1[3 * (size_t)idx[k] + c]; P2[k][c] = X2[3 * (size_t)idx[k] + c]; }
    // Step 1: centroids and relative coordinates
#pragma unroll
    for (int c = 0; c < 3; c++) {
        O1[c] = (P1[0][c] + P1[1][c] + P1[2][c]) / 3.0;
        O2[c] = (P2[0][c] + P2[1][c] + P2[2][c]) / 3.0;
#pragma unroll
        for (int k = 0; k < 3; k++) { P1[k][c] -= O1[c]; P2[k][c] -= O2[c]; }
    }
    // Step 2: M = Pr2 * Pr1^T
    double M[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[i][j] = P2[0][i] * P1[0][j] + P2[1][i] * P1[1][j] + P2[2][i] * P1[2][j];
    // Step 3: N
    double N[4][4], V[4][4];
    N[0][0] = M[0][0] + M[1][1] + M[2][2];
    N[0][1] = M[1][2] - M[2][1];
    N[0][2] = M[2][0] - M[0][2];
    N[0][3] = M[0][1] - M[1][0];
    N[1][1] = M[0][0] - M[1][1] - M[2][2];
    N[1][2] = M[0][1] + M[1][0];
    N[1][3] = M[2][0] + M[0][2];
    N[2][2] = -M[0][0] + M[1][1] - M[2][2];
    N[2][3] = M[1][2] + M[2][1];
    N[3][3] = -M[0][0] - M[1][1] + M[2][2];
#pragma unroll
    for (int i = 1; i < 4; i++)
#pragma unroll
        for (int j = 0; j < i; j++) N[i][j] = N[j][i];
    // Step 4: the eigenvector of the largest eigenvalue (the first of equals) is the quaternion
    jacobi4(N, V);
    double ev = N[0][0], q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int j = 1; j < 4; j++)
        if (N[j][j] > ev) { ev = N[j][j]; q[0] = V[0][j]; q[1] = V[1][j]; q[2] = V[2][j]; q[3] = V[3][j]; }
    const double nrm = sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double ang = atan2(nrm, q[0]);
    double r[3] = {2 * ang * q[1] / nrm, 2 * ang * q[2] / nrm, 2 * ang * q[3] / nrm};   // angle-axis: the quaternion's angle is the half
    // cv::Rodrigues
    Sim3Hyp H;
    const double theta = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (theta < DBL_EPSILON) {
#pragma unroll
        for (int i = 0; i < 9; i++) H.R[i] = (i % 4 == 0) ? 1.f : 0.f;
    } else {
        const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, itheta = 1.0 / theta;
        r[0] *= itheta; r[1] *= itheta; r[2] *= itheta;
        const double rx[9] = {0, -r[2], r[1], r[2], 0, -r[0], -r[1], r[0], 0};
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) H.R[3 * i + j] = (float)(((i == j ? c : 0.0) + c1 * r[i] * r[j]) + s * rx[3 * i + j]);
    }
    double Rd[9];
#pragma unroll
    for (int i = 0; i < 9; i++) Rd[i] = H.R[i];
    // Steps 5, 6: rotate set 2, scale
    if (!fix_scale) {
        double nom = 0.0, den = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double p3 = Rd[3 * i] * P2[k][0] + Rd[3 * i + 1] * P2[k][1] + Rd[3 * i + 2] * P2[k][2];
                nom += P1[k][i] * p3;
                den += p3 * p3;
            }
        H.s = (float)(nom / den);
    } else {
        H.s = 1.0f;
    }
    // Step 7: t = O1 - s R O2
    const double sd = H.s;
#pragma unroll
    for (int i = 0; i < 3; i++) H.t[i] = (float)(O1[i] - (((sd * Rd[3 * i]) * O2[0] + (sd * Rd[3 * i + 1]) * O2[1]) + (sd * Rd[3 * i + 2]) * O2[2]));
    return H;
}

__device__ __forceinline__ bool hyp_finite(const Sim3Hyp& H) {
    bool ok = isfinite(H.s);
#pragma unroll
    for (int i = 0; i < 9; i++) ok = ok && isfinite(H.R[i]);
#pragma unroll
    for (int i = 0; i < 3; i++) ok = ok && isfinite(H.t[i]);
    return ok;
}

// Step 8 (:318-336) in float: T12 = [sR | t], T21 = [(1 / s) R^T | -(1 / s) R^T t].
__device__ inline Sim3T make_T(const Sim3Hyp& H) {
    Sim3T T;
    const float inv = (float)(1.0 / (double)H.s);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) { T.a12[4 * i + j] = H.s * H.R[3 * i + j]; T.a21[4 * i + j] = inv * H.R[3 * j + i]; }
        T.a12[4 * i + 3] = H.t[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) T.a21[4 * i + 3] = -((T.a21[4 * i] * H.t[0] + T.a21[4 * i + 1] * H.t[1]) + T.a21[4 * i + 2] * H.t[2]);
    return T;
}

struct Sim3ProblemDev { const float* x1; const float* x2; const float* s1; const float* s2; int N; float K1[4], K2[4]; };

// FromCameraToImage (:405-423)
__device__ __forceinline__ void to_image(const float K[4], float X, float Y, float Z, float& u, float& v) {
    const float invz = 1.0f / Z;
    const float x = X * invz, y = Y * invz;
    u = K[0] * x + K[2]; v = K[1] * y + K[3];
}
// Project (:382-403): a = the first three rows of Tcw
__device__ __forceinline__ void project(const float a[12], const float K[4], float X, float Y, float Z, float& u, float& v) {
    const float xc = ((a[0] * X + a[1] * Y) + a[2] * Z) + a[3];
    const float yc = ((a[4] * X + a[5] * Y) + a[6] * Z) + a[7];
    const float zc = ((a[8] * X + a[9] * Y) + a[10] * Z) + a[11];
    to_image(K, xc, yc, zc, u, v);
}
// mvnMaxError (:87-88): the double product truncated to size_t, compared as float (:356)
__device__ __forceinline__ float max_error(float sigma2) { return sigma2 > 0.f ? (float)floor(9.210 * (double)sigma2) : 0.f; }

// CheckInliers (:340-364) of correspondence i
__device__ __forceinline__ bool is_inlier(const Sim3ProblemDev& Q, const Sim3T& T, int i) {
    const float X1 = Q.x1[3 * (size_t)i], Y1 = Q.x1[3 * (size_t)i + 1], Z1 = Q.x1[3 * (size_t)i + 2];
    const float X2 = Q.x2[3 * (size_t)i], Y2 = Q.x2[3 * (size_t)i + 1], Z2 = Q.x2[3 * (size_t)i + 2];
    float u11, v11, u22, v22, u21, v21, u12, v12;
    to_image(Q.K1, X1, Y1, Z1, u11, v11);            // mvP1im1
    to_image(Q.K2, X2, Y2, Z2, u22, v22);            // mvP2im2
    project(T.a12, Q.K1, X2, Y2, Z2, u21, v21);      // vP2im1
    project(T.a21, Q.K2, X1, Y1, Z1, u12, v12);      // vP1im2
    const float d1x = u11 - u21, d1y = v11 - v21, d2x = u12 - u22, d2y = v12 - v22;
    const float err1 = d1x * d1x + d1y * d1y, err2 = d2x * d2x + d2y * d2y;
    return err1 < max_error(Q.s1[i]) && err2 < max_error(Q.s2[i]);
}

struct Sim3Args {
    const oslam_sim3_problem_t* problems;
    oslam_sim3_state_t* states;
    const float* x1; const float* x2; const float* s1; const float* s2;
    int n_problems;
    int n_corr;           // entries of the packed arrays
    int it_stride;        // = params.max_iterations: row length of samples, iter_inliers, hypotheses and the arena
    int chunk;            // iterations of this call per problem, at most it_stride
    oslam_sim3_params_t prm;
    const int32_t* samples;
    float* hyp; int32_t* counts;   // arena
    float* T12; uint8_t* inliers; int32_t* status; int32_t* iter_inliers; float* hypotheses;
};

__device__ __forceinline__ bool problem_valid(const oslam_sim3_problem_t& pr, int n_corr) {
    return pr.count >= 0 && pr.offset >= 0 && pr.count <= n_corr && pr.offset <= n_corr - pr.count;
}
__device__ __forceinline__ Sim3ProblemDev problem_dev(const Sim3Args& a, const oslam_sim3_problem_t& pr) {
    Sim3ProblemDev Q;
    Q.x1 = a.x1 + 3 * (size_t)pr.offset; Q.x2 = a.x2 + 3 * (size_t)pr.offset; Q.s1 = a.s1 + pr.offset; Q.s2 = a.s2 + pr.offset;
    Q.N = pr.count;
    Q.K1[0] = pr.fx1; Q.K1[1] = pr.fy1; Q.K1[2] = pr.cx1; Q.K1[3] = pr.cy1;
    Q.K2[0] = pr.fx2; Q.K2[1] = pr.fy2; Q.K2[2] = pr.cx2; Q.K2[3] = pr.cy2;
    return Q;
}

// One hypothesis per group of 16 lanes: group (problem b, k) evaluates iteration iterations_done + k of problem b.  64 threads; groups beyond a
// problem's range leave at once (no workgroup synchronisation in this kernel: the exchanges of the count stay inside a row of 16 lanes).
// A hypothesis that is not finite, or whose explicit sample is not three distinct indices of the problem, is stored with the count -1.
__global__ __launch_bounds__(kG* kPerBlock) void k_sim3_hypotheses(Sim3Args a) {
    const long long gid = (long long)blockIdx.x * kPerBlock + threadIdx.x / kG;
    const int c = threadIdx.x % kG;
    if (gid >= (long long)a.n_problems * a.chunk) return;
    const int b = (int)(gid / a.chunk), k = (int)(gid % a.chunk);
    const oslam_sim3_problem_t pr = a.problems[b];
    if (!problem_valid(pr, a.n_corr)) return;
    const int it0 = a.states[b].iterations_done;
    const Sim3Ransac ra = ransac_adjust(pr.count, a.prm.probability, a.prm.min_inliers, a.prm.max_iterations);
    if (ra.no_more || it0 < 0 || it0 >= ra.iterations || k >= ra.iterations - it0) return;   // (ra.iterations <= it_stride)
    const int it = it0 + k;
    int idx[3];
    bool ok = true;
    if (a.samples) {
        const int32_t* s = a.samples + ((size_t)b * a.it_stride + it) * 3;
#pragma unroll
        for (int j = 0; j < 3; j++) { idx[j] = s[j]; ok = ok && idx[j] >= 0 && idx[j] < pr.count; }
        ok = ok && idx[0] != idx[1] && idx[0] != idx[2] && idx[1] != idx[2];
        if (!ok) { idx[0] = 0; idx[1] = 1; idx[2] = 2; }   // (count >= 3)
    } else {
        oslam::ransac_draw<3>(pr.seed, it, pr.count, idx);
    }
    const Sim3ProblemDev Q = problem_dev(a, pr);
    const Sim3Hyp H = compute_sim3(Q.x1, Q.x2, idx, pr.fix_scale != 0);
    ok = ok && hyp_finite(H);
    const Sim3T T = make_T(H);
    int cnt = 0;
    for (int i = c; i < Q.N; i += kG) cnt += is_inlier(Q, T, i) ? 1 : 0;
    cnt = oslam::row16_sum_i32(cnt);
    if (c == 0) {
        const size_t o = (size_t)b * a.it_stride + it;
        a.counts[o] = ok ? cnt : -1;
        float* ho = a.hyp + o * 13;
#pragma unroll
        for (int i = 0; i < 9; i++) ho[i] = H.R[i];
#pragma unroll
        for (int i = 0; i < 3; i++) ho[9 + i] = H.t[i];
        ho[12] = H.s;
    }
}

__device__ __forceinline__ Sim3Hyp hyp_load(const float* ho) {
    Sim3Hyp H;
#pragma unroll
    for (int i = 0; i < 9; i++) H.R[i] = ho[i];
#pragma unroll
    for (int i = 0; i < 3; i++) H.t[i] = ho[9 + i];
    H.s = ho[12];
    return H;
}

// iterate() (:140-207) over the counts of the chunk, 16 lanes per problem, four problems per workgroup.
__global__ __launch_bounds__(kG* kPerBlock) void k_sim3_select(Sim3Args a) {
    const int b = blockIdx.x * kPerBlock + threadIdx.x / kG, c = threadIdx.x % kG;
    if (b >= a.n_problems) return;
    const oslam_sim3_problem_t pr = a.problems[b];
    int32_t* st = a.status + 4 * (size_t)b;
    oslam_sim3_state_t* S = a.states + b;
    const int it0 = S->iterations_done;
    if (!problem_valid(pr, a.n_corr) || it0 < 0) { if (c == 0) { st[0] = -1; st[1] = 0; st[2] = 0; st[3] = 0; } return; }
    const Sim3Ransac ra = ransac_adjust(pr.count, a.prm.probability, a.prm.min_inliers, a.prm.max_iterations);
    if (ra.no_more) { if (c == 0) { st[0] = 0; st[1] = 0; st[2] = 0; st[3] = 1; } return; }
    const Sim3ProblemDev Q = problem_dev(a, pr);
    {   // input validation: a problem with a number that is not finite has no Sim3 (its hypotheses are not looked at)
        int bad = (isfinite(pr.fx1) && isfinite(pr.fy1) && isfinite(pr.cx1) && isfinite(pr.cy1) && isfinite(pr.fx2) && isfinite(pr.fy2) && isfinite(pr.cx2) && isfinite(pr.cy2)) ? 0 : 1;
        for (int i = c; i < Q.N; i += kG) {
            bool fin = isfinite(Q.s1[i]) && isfinite(Q.s2[i]);
#pragma unroll
            for (int j = 0; j < 3; j++) fin = fin && isfinite(Q.x1[3 * (size_t)i + j]) && isfinite(Q.x2[3 * (size_t)i + j]);
            bad |= fin ? 0 : 1;
        }
        if (oslam::row16_sum_i32(bad) != 0) { if (c == 0) { st[0] = 0; st[1] = 0; st[2] = 0; st[3] = 1; } return; }
    }
    const size_t o = (size_t)b * a.it_stride;
    const int end = it0 >= ra.iterations ? it0 : it0 + min(a.chunk, ra.iterations - it0);
    int best = S->best_inliers, best_it = -1, ret = -1, ret_cnt = 0;
    for (int it = it0; it < end; it++) {   // (uniform over the group: every lane reads the same counts)
        const int cnt = a.counts[o + it];
        if (cnt < 0 || cnt < best) continue;
        best = cnt; best_it = it;
        if (cnt > a.prm.min_inliers) { ret = it; ret_cnt = cnt; break; }
    }
    const int ran = (ret >= 0 ? ret + 1 : end) - it0;
    if (a.iter_inliers)
        for (int it = it0 + c; it < it0 + ran; it += kG) a.iter_inliers[o + it] = max(a.counts[o + it], 0);
    if (a.hypotheses)
        for (int e = c; e < ran * 13; e += kG) a.hypotheses[(o + it0) * 13 + e] = a.hyp[(o + it0) * 13 + e];
    if (ret >= 0) {   // the flags of the returning hypothesis, recomputed from what the arena holds
        const Sim3Hyp H = hyp_load(a.hyp + (o + ret) * 13);
        const Sim3T T = make_T(H);
        uint8_t* flags = a.inliers + pr.offset;
        for (int i = c; i < Q.N; i += kG) flags[i] = is_inlier(Q, T, i) ? 1 : 0;
        if (c == 0) {
            float* T12 = a.T12 + 16 * (size_t)b;
#pragma unroll
            for (int i = 0; i < 12; i++) T12[i] = T.a12[i];
            T12[12] = 0.f; T12[13] = 0.f; T12[14] = 0.f; T12[15] = 1.f;
        }
    }
    if (c == 0) {
        S->iterations_done = it0 + ran;
        if (best_it >= 0) {
            S->best_inliers = best; S->best_iteration = best_it;
            const float* ho = a.hyp + (o + best_it) * 13;
#pragma unroll
            for (int i = 0; i < 9; i++) S->R[i] = ho[i];
#pragma unroll
            for (int i = 0; i < 3; i++) S->t[i] = ho[9 + i];
            S->s = ho[12];
        }
        st[0] = ret >= 0 ? 1 : 0; st[1] = ret_cnt; st[2] = ran;
        st[3] = (ret < 0 && it0 + ran >= ra.iterations) ? 1 : 0;   // bNoMore stays false on a return, even on the last iteration
    }
}

int check_call(const char* fn, const oslam_sim3_t* h, const oslam_sim3_params_t* p, int n_problems, int n_corr, int n_iterations) {
    if (!p) { set_error("%s: params is NULL", fn); return OSLAM_E_INVALID; }
    if (p->min_inliers < 0 || n_iterations < 0) { set_error("%s: min_inliers = %d, n_iterations = %d: neither may be negative", fn, p->min_inliers, n_iterations); return OSLAM_E_INVALID; }
    if (p->max_iterations < 1 || !(p->probability > 0.0 && p->probability < 1.0)) { set_error("%s: bad parameter block", fn); return OSLAM_E_INVALID; }
    if (p->max_iterations > h->max_iterations) {
        set_error("%s: max_iterations = %d exceeds the handle's %d", fn, p->max_iterations, h->max_iterations);
        return OSLAM_E_CAPACITY;
    }
    if (n_problems > h->max_problems || n_corr > h->max_corr) {
        set_error("%s: %d problems / %d correspondences exceed the handle's %d / %d", fn, n_problems, n_corr, h->max_problems, h->max_corr);
        return OSLAM_E_CAPACITY;
    }
    return OSLAM_OK;
}

}  // namespace

extern "C" {

int oslam_sim3_ransac_params(int N, double probability, int min_inliers, int max_iterations, oslam_sim3_ransac_t* out) {
    if (!out || N < 0 || max_iterations < 1) { set_error("oslam_sim3_ransac_params: bad argument"); return OSLAM_E_INVALID; }
    const Sim3Ransac r = ransac_adjust(N, probability, min_inliers, max_iterations);
    out->iterations = r.iterations; out->no_more = r.no_more;
    return OSLAM_OK;
}

int oslam_sim3_draw(uint32_t seed, int iteration, int N, int32_t idx[3]) {
    if (!idx || N < 3 || iteration < 0) { set_error("oslam_sim3_draw: bad argument"); return OSLAM_E_INVALID; }
    int v[3];
    oslam::ransac_draw<3>(seed, iteration, N, v);
    for (int k = 0; k < 3; k++) idx[k] = v[k];
    return OSLAM_OK;
}

void oslam_sim3_destroy(oslam_sim3_t* h) {
    if (!h) return;
    delete h;
}

int oslam_sim3_create(oslam_sim3_t** out, int max_problems, int max_correspondences_total, int max_iterations) {
    if (!out) { set_error("oslam_sim3_create: out is NULL"); return OSLAM_E_INVALID; }
    *out = nullptr;
    if (max_problems < 1 || max_correspondences_total < 1 || max_iterations < 1 || (long long)max_problems * max_iterations > (1ll << 30)) {
        set_error("oslam_sim3_create: bad argument");
        return OSLAM_E_INVALID;
    }
    if (oslam_device_count() <= 0) return oslam::no_device("oslam_sim3_create");
    oslam_sim3* h = new oslam_sim3;
    h->max_problems = max_problems; h->max_corr = max_correspondences_total; h->max_iterations = max_iterations;
    const size_t hyp = (size_t)max_problems * max_iterations;
    int rc;
    if ((rc = h->hyp.alloc(hyp * 13 * sizeof(float))) || (rc = h->counts.alloc(hyp * sizeof(int32_t)))) {
        delete h;
        return rc;
    }
    *out = h;
    return OSLAM_OK;
}

int oslam_sim3_iterate_batch_device(oslam_sim3_t* h, int n_problems, const oslam_sim3_problem_t* d_problems, oslam_sim3_state_t* d_states, int n_corr, const float* d_X3Dc1,
                                    const float* d_X3Dc2, const float* d_sigma2_1, const float* d_sigma2_2, const oslam_sim3_params_t* params, int n_iterations,
                                    const int32_t* d_samples, float* d_T12, uint8_t* d_inliers, int32_t* d_status, int32_t* d_iter_inliers, float* d_hypotheses,
                                    void* stream) {
    if (!h || n_problems < 0 || n_corr < 0 || !d_status || (n_problems > 0 && (!d_problems || !d_states || !d_T12)) ||
        (n_corr > 0 && (!d_X3Dc1 || !d_X3Dc2 || !d_sigma2_1 || !d_sigma2_2 || !d_inliers))) {
        set_error("oslam_sim3_iterate_batch_device: bad argument");
        return OSLAM_E_INVALID;
    }
    OSLAM_CHECK(check_call("oslam_sim3_iterate_batch_device", h, params, n_problems, n_corr, n_iterations));
    if (n_problems == 0) return OSLAM_OK;
    Sim3Args a;
    a.problems = d_problems; a.states = d_states; a.x1 = d_X3Dc1; a.x2 = d_X3Dc2; a.s1 = d_sigma2_1; a.s2 = d_sigma2_2;
    a.n_problems = n_problems; a.n_corr = n_corr; a.it_stride = params->max_iterations; a.chunk = std::min(n_iterations, params->max_iterations); a.prm = *params;
    a.samples = d_samples; a.hyp = h->hyp.as<float>(); a.counts = h->counts.as<int32_t>();
    a.T12 = d_T12; a.inliers = d_inliers; a.status = d_status; a.iter_inliers = d_iter_inliers; a.hypotheses = d_hypotheses;
    if (a.chunk > 0) {
        const long long groups = (long long)n_problems * a.chunk;   // (at most 2^30: oslam_sim3_create)
        hipLaunchKernelGGL(k_sim3_hypotheses, dim3((unsigned)((groups + kPerBlock - 1) / kPerBlock)), dim3(kG * kPerBlock), 0, (hipStream_t)stream, a);
    }
    hipLaunchKernelGGL(k_sim3_select, dim3(oslam::div_up(n_problems, kPerBlock)), dim3(kG * kPerBlock), 0, (hipStream_t)stream, a);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int oslam_sim3_iterate_batch(oslam_sim3_t* h, int n_problems, const oslam_sim3_problem_t* problems, oslam_sim3_state_t* states, int n_corr, const float* X3Dc1,
                             const float* X3Dc2, const float* sigma2_1, const float* sigma2_2, const oslam_sim3_params_t* params, int n_iterations, const int32_t* samples,
                             float* T12, uint8_t* inliers, int32_t* status, int32_t* iter_inliers, float* hypotheses) {
    if (!h || n_problems < 0 || n_corr < 0 || (n_problems > 0 && (!problems || !states || !T12 || !status)) ||
        (n_corr > 0 && (!X3Dc1 || !X3Dc2 || !sigma2_1 || !sigma2_2 || !inliers))) {
        set_error("oslam_sim3_iterate_batch: bad argument");
        return OSLAM_E_INVALID;
    }
    OSLAM_CHECK(check_call("oslam_sim3_iterate_batch", h, params, n_problems, n_corr, n_iterations));
    for (int b = 0; b < n_problems; b++) {
        const oslam_sim3_problem_t& pr = problems[b];
        if (pr.count < 0 || pr.offset < 0 || pr.count > n_corr || pr.offset > n_corr - pr.count) {
            set_error("oslam_sim3_iterate_batch: problem %d (offset %d, count %d) lies outside the %d correspondences", b, pr.offset, pr.count, n_corr);
            return OSLAM_E_INVALID;
        }
        if (states[b].iterations_done < 0) { set_error("oslam_sim3_iterate_batch: state %d has iterations_done = %d", b, states[b].iterations_done); return OSLAM_E_INVALID; }
    }
    if (n_problems == 0) return OSLAM_OK;
    std::lock_guard<std::mutex> lock(h->mu);
    const size_t np = (size_t)n_problems, nc = (size_t)n_corr, its = (size_t)params->max_iterations;
    // one block.  One upload of everything up to and including the states, one download of everything from the states on.
    oslam::StageLayout lay;
    const auto fProb = lay.add<oslam_sim3_problem_t>(np);
    const auto fX1 = lay.add<float>(nc * 3), fX2 = lay.add<float>(nc * 3), fS1 = lay.add<float>(nc), fS2 = lay.add<float>(nc);
    const auto fSam = lay.add<int32_t>(np * its * 3, samples != nullptr);
    const auto fState = lay.add<oslam_sim3_state_t>(np);
    const auto fSt = lay.add<int32_t>(np * 4);
    const auto fT = lay.add<float>(np * 16);
    const auto fIn = lay.add<uint8_t>(nc);
    const auto fIt = lay.add<int32_t>(np * its, iter_inliers != nullptr);
    const auto fHy = lay.add<float>(np * its * 13, hypotheses != nullptr);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fProb, ph, problems); put(fX1, ph, X3Dc1); put(fX2, ph, X3Dc2); put(fS1, ph, sigma2_1); put(fS2, ph, sigma2_2); put(fSam, ph, samples); put(fState, ph, states);
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, fSt.off, hipMemcpyHostToDevice, nullptr));
    OSLAM_CHECK(oslam_sim3_iterate_batch_device(h, n_problems, at(fProb, pd), at(fState, pd), n_corr, at(fX1, pd), at(fX2, pd), at(fS1, pd), at(fS2, pd), params, n_iterations,
                                                at(fSam, pd), at(fT, pd), at(fIn, pd), at(fSt, pd), at(fIt, pd), at(fHy, pd), nullptr));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fState.off, pd + fState.off, lay.total() - fState.off, hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(fSt, ph, status);
    for (int b = 0; b < n_problems; b++) {
        const size_t row = (size_t)b * its + states[b].iterations_done, ran = (size_t)std::max(status[4 * b + 2], 0);   // (the caller's record still holds the state before the call)
        if (iter_inliers && ran) memcpy(iter_inliers + row, at(fIt, ph) + row, ran * sizeof(int32_t));
        if (hypotheses && ran) memcpy(hypotheses + row * 13, at(fHy, ph) + row * 13, ran * 13 * sizeof(float));
        if (status[4 * b] <= 0) continue;   // a problem without a Sim3 keeps the caller's T12 and inlier bytes
        memcpy(T12 + 16 * (size_t)b, at(fT, ph) + 16 * (size_t)b, 16 * sizeof(float));
        memcpy(inliers + problems[b].offset, at(fIn, ph) + problems[b].offset, (size_t)problems[b].count);
    }
    get(fState, ph, states);
    return OSLAM_OK;
}

}  // extern "C"
