// pnp.hip — PnPsolver (src/PnPsolver.cc: EPnP inside RANSAC) for batches of independent problems on gfx950 (include/oslam_hip.h, "PnP solver").
// Two launches per call: k_pnp_hypotheses computes every (problem, iteration) hypothesis — 16 lanes each, four per wavefront — and k_pnp_select replays
// iterate()'s control flow over the counts, one 16-lane workgroup per problem.  All EPnP arithmetic is fp64; CheckInliers keeps the
// reference's float / double mix.  Product code; never includes oracle/.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <mutex>
#include <vector>

#include "common.h"
#include "lane_ops.h"
#include "ransac_draw.h"   // the counter-based generator and the draw rule, shared with sim3.hip
#include "small_svd.h"     // svd3, shared with initializer.hip
#include "stage_layout.h"

using oslam::set_error;
using oslam::svd3;

struct oslam_pnp {
    int max_problems = 0, max_corr = 0, max_iterations = 0, max_sets = 0;
    oslam::DeviceBuffer pose, counts, sel;   // work arena: [problem][iteration][12] fp64, [problem][iteration] int32, [correspondence] int32
    oslam::StagePair up, down;               // staging of the host-pointer entry points
    std::mutex mu;
};

namespace {

constexpr int kG = 16;             // lanes per hypothesis / per EPnP
constexpr int kHypPerBlock = 4;    // one wavefront
constexpr int kJacobiSweeps = 10;  // cyclic Jacobi on the 12 x 12 MtM: fixed, so that NaN inputs cannot spin and every lane exchange is in uniform control flow

struct RansacAdj { int min_inliers; float epsilon; int iterations; int no_more; };

// SetRansacParameters (src/PnPsolver.cc:121-157) with its mixed arithmetic; the same text runs on the host and in the kernels.
__host__ __device__ inline RansacAdj ransac_adjust(int N, double probability, int minInliers, int maxIterations, int minSet, float epsilon) {
    RansacAdj r;
    int nMinInliers = (int)((float)N * epsilon);   // int nMinInliers = N*mRansacEpsilon
    if (nMinInliers < minInliers) nMinInliers = minInliers;
    if (nMinInliers < minSet) nMinInliers = minSet;
    r.min_inliers = nMinInliers;
    r.no_more = N < nMinInliers;
    if (N > 0 && epsilon < (float)nMinInliers / N) epsilon = (float)nMinInliers / N;
    r.epsilon = epsilon;
    if (r.no_more) { r.iterations = 0; return r; }   // iterate() returns before its loop (:173-177)
    int nIterations;
    if (nMinInliers == N) nIterations = 1;
    else {
        const double d = ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3.0)));
        nIterations = d < (double)maxIterations ? (int)d : maxIterations;   // (also NaN: the comparison is false)
    }
    if (nIterations > maxIterations) nIterations = maxIterations;
    r.iterations = nIterations < 1 ? 1 : nIterations;
    return r;
}

struct PnpPts {
    const float* p3;    // [..][3], the problem's first correspondence
    const float* p2;    // [..][2]
    const int* sel;     // correspondence of EPnP point i, or NULL = i
    int n;
    double fu, fv, uc, vc;
};
struct Pt { double X, Y, Z, u, v; };
__device__ __forceinline__ Pt pt_load(const PnpPts& P, int i) {
    const int j = P.sel ? P.sel[i] : i;
    Pt p;
    p.X = P.p3[3 * j]; p.Y = P.p3[3 * j + 1]; p.Z = P.p3[3 * j + 2];
    p.u = P.p2[2 * j]; p.v = P.p2[2 * j + 1];
    return p;
}

// qr_solve (:860-950) for 6 rows: Householder QR, b <- Qt b, back substitution.  A singular column leaves X at zero (the reference returns with X unset).
template <int NC>
__device__ inline void qr_solve6(double (&A)[6 * NC], double (&b)[6], double (&X)[NC]) {
    constexpr int nr = 6, nc = NC;
    double A1[NC], A2[NC];
#pragma unroll
    for (int k = 0; k < nc; k++) X[k] = 0.0;
    bool singular = false;
#pragma unroll
    for (int k = 0; k < nc; k++) {
        double eta = fabs(A[k * nc + k]);
#pragma unroll
        for (int i = k + 1; i < nr; i++) { const double elt = fabs(A[(i - 1) * nc + k]); if (eta < elt) eta = elt; }   // (:881-885 reads before it steps: rows k .. nr - 2)
        if (eta == 0) { singular = true; A1[k] = A2[k] = 0.0; }
        if (!singular) {
            double sum = 0.0;
            const double inv_eta = 1. / eta;
#pragma unroll
            for (int i = k; i < nr; i++) { A[i * nc + k] *= inv_eta; sum += A[i * nc + k] * A[i * nc + k]; }
            double sigma = sqrt(sum);
            if (A[k * nc + k] < 0) sigma = -sigma;
            A[k * nc + k] += sigma;
            A1[k] = sigma * A[k * nc + k];
            A2[k] = -eta * sigma;
#pragma unroll
            for (int j = k + 1; j < nc; j++) {
                double s2 = 0;
#pragma unroll
                for (int i = k; i < nr; i++) s2 += A[i * nc + k] * A[i * nc + j];
                const double tau = s2 / A1[k];
#pragma unroll
                for (int i = k; i < nr; i++) A[i * nc + j] -= tau * A[i * nc + k];
            }
        }
    }
    if (singular) return;
#pragma unroll
    for (int j = 0; j < nc; j++) {
        double tau = 0;
#pragma unroll
        for (int i = j; i < nr; i++) tau += A[i * nc + j] * b[i];
        tau /= A1[j];
#pragma unroll
        for (int i = j; i < nr; i++) b[i] -= tau * A[i * nc + j];
    }
    X[nc - 1] = b[nc - 1] / A2[nc - 1];
#pragma unroll
    for (int i = nc - 2; i >= 0; i--) {
        double sum = 0;
#pragma unroll
        for (int j = i + 1; j < nc; j++) sum += A[i * nc + j] * X[j];
        X[i] = (b[i] - sum) / A2[i];
    }
}

// What EPnP keeps per group in LDS: the 12 x 12 image of MtM (diagonal = eigenvalues after the sweeps), the eigenvectors (columns), the rotations of a round.
struct PnpLds { double A[144]; double V[144]; double cs[12]; double L[60]; double rho[6]; };

struct Epnp {   // state shared by the steps below (registers, the same in every lane of the group)
    double cws0[3];        // centroid = control point 0
    double ci[3][3];       // CC^-1: row j = PCA axis j / k_j
    double cw[3][3];       // control points 1..3 minus control point 0
    int vidx[4];           // eigenvector (column of V) of the smallest, second smallest, .. eigenvalue = ut rows 11, 10, 9, 8
};

__device__ __forceinline__ void alphas_of(const Epnp& E, const Pt& p, double a[4]) {
    const double dx = p.X - E.cws0[0], dy = p.Y - E.cws0[1], dz = p.Z - E.cws0[2];
#pragma unroll
    for (int j = 0; j < 3; j++) a[1 + j] = E.ci[j][0] * dx + E.ci[j][1] * dy + E.ci[j][2] * dz;
    a[0] = 1.0 - a[1] - a[2] - a[3];
}

// 12 x 12 symmetric eigen-decomposition in LDS by cyclic Jacobi with the round-robin ordering: 11 rounds of six disjoint rotations per sweep.  A round =
// lanes 0..5 compute (c, s) of their pair from the current image; then the 21 pairs of rotation pairs (a <= b) each transform one 2 x 2 block of J^T A J and
// its mirror, and lanes 0..11 rotate their row of V.  Called by all 16 lanes of every group of the workgroup, in uniform control flow.
__device__ inline void jacobi12(PnpLds& S, int c) {
    for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
        for (int r = 0; r < 11; r++) {
            if (c < 6) {
                int p = c == 0 ? r : (r + c) % 11, q = c == 0 ? 11 : (r + 11 - c) % 11;
                if (p > q) { const int t = p; p = q; q = t; }
                const double app = S.A[p * 12 + p], aqq = S.A[q * 12 + q], apq = S.A[p * 12 + q];
                double cc = 1.0, ss = 0.0;
                if (apq != 0.0) {
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double t = (theta < 0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    cc = 1.0 / sqrt(t * t + 1.0); ss = t * cc;
                }
                S.cs[2 * c] = cc; S.cs[2 * c + 1] = ss;
            }
            __syncthreads();
            for (int e = c; e < 21; e += kG) {
                int a = 0, rem = e;   // e -> (a, b), a <= b < 6, row-major over the upper triangle
                while (rem >= 6 - a) { rem -= 6 - a; a++; }
                const int b = a + rem;
                int pa = a == 0 ? r : (r + a) % 11, qa = a == 0 ? 11 : (r + 11 - a) % 11;
                if (pa > qa) { const int t = pa; pa = qa; qa = t; }
                int pb = b == 0 ? r : (r + b) % 11, qb = b == 0 ? 11 : (r + 11 - b) % 11;
                if (pb > qb) { const int t = pb; pb = qb; qb = t; }
                const double ca = S.cs[2 * a], sa = S.cs[2 * a + 1], cb = S.cs[2 * b], sb = S.cs[2 * b + 1];
                const double b00 = S.A[pa * 12 + pb], b01 = S.A[pa * 12 + qb], b10 = S.A[qa * 12 + pb], b11 = S.A[qa * 12 + qb];
                const double t00 = ca * b00 - sa * b10, t01 = ca * b01 - sa * b11, t10 = sa * b00 + ca * b10, t11 = sa * b01 + ca * b11;
                double n00 = t00 * cb - t01 * sb, n01 = t00 * sb + t01 * cb, n10 = t10 * cb - t11 * sb, n11 = t10 * sb + t11 * cb;
                if (a == b) { n01 = 0.0; n10 = 0.0; }
                S.A[pa * 12 + pb] = n00; S.A[pa * 12 + qb] = n01; S.A[qa * 12 + pb] = n10; S.A[qa * 12 + qb] = n11;
                if (a != b) { S.A[pb * 12 + pa] = n00; S.A[qb * 12 + pa] = n01; S.A[pb * 12 + qa] = n10; S.A[qb * 12 + qa] = n11; }
            }
            if (c < 12) {
                for (int k = 0; k < 6; k++) {
                    int p = k == 0 ? r : (r + k) % 11, q = k == 0 ? 11 : (r + 11 - k) % 11;
                    if (p > q) { const int t = p; p = q; q = t; }
                    const double cc = S.cs[2 * k], ss = S.cs[2 * k + 1];
                    const double vp = S.V[c * 12 + p], vq = S.V[c * 12 + q];
                    S.V[c * 12 + p] = cc * vp - ss * vq; S.V[c * 12 + q] = ss * vp + cc * vq;
                }
            }
            __syncthreads();
        }
    }
}

// compute_R_and_t (:651-662) for one beta set: control points in the camera frame, solve_for_sign, estimate_R_and_t, reprojection_error.  The sums over
// the points go over the group's lanes: lane c adds points c, c + 16, .. in order, then the xor butterfly of row16_sum — an order fixed by n alone.
__device__ inline double compute_R_and_t(const PnpPts& P, const Epnp& E, const PnpLds& S, const double betas[4], int c, double R[3][3], double t[3]) {
    double ccs[4][3];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int k = 0; k < 3; k++) ccs[j][k] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 3; k++) ccs[j][k] += betas[i] * S.V[(3 * j + k) * 12 + E.vidx[i]];
    {   // solve_for_sign: pcs[2], the depth of the first point
        double a[4];
        alphas_of(E, pt_load(P, 0), a);
        const double z0 = a[0] * ccs[0][2] + a[1] * ccs[1][2] + a[2] * ccs[2][2] + a[3] * ccs[3][2];
        if (z0 < 0.0) {
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int k = 0; k < 3; k++) ccs[j][k] = -ccs[j][k];
        }
    }
    const double n = (double)P.n;
    double pc0[3] = {0, 0, 0};
    for (int i = c; i < P.n; i += kG) {
        double a[4];
        alphas_of(E, pt_load(P, i), a);
#pragma unroll
        for (int j = 0; j < 3; j++) pc0[j] += a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j];
    }
#pragma unroll
    for (int j = 0; j < 3; j++) pc0[j] = oslam::row16_sum(pc0[j]) / n;
    const double* pw0 = E.cws0;   // (the same sum as the centroid of choose_control_points)
    double abt[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int i = c; i < P.n; i += kG) {
        const Pt p = pt_load(P, i);
        double a[4];
        alphas_of(E, p, a);
        const double pw[3] = {p.X, p.Y, p.Z};
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double pcj = a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j];
#pragma unroll
            for (int k = 0; k < 3; k++) abt[j][k] += (pcj - pc0[j]) * (pw[k] - pw0[k]);
        }
    }
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int k = 0; k < 3; k++) abt[j][k] = oslam::row16_sum(abt[j][k]);
    double U[3][3], w[3], V[3][3];
    svd3(abt, U, w, V);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[i][j] = U[i][0] * V[j][0] + U[i][1] * V[j][1] + U[i][2] * V[j][2];
    const double det = R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] - R[0][2] * R[1][1] * R[2][0] -
                       R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1];
    if (det < 0) { R[2][0] = -R[2][0]; R[2][1] = -R[2][1]; R[2][2] = -R[2][2]; }
#pragma unroll
    for (int j = 0; j < 3; j++) t[j] = pc0[j] - (R[j][0] * pw0[0] + R[j][1] * pw0[1] + R[j][2] * pw0[2]);
    double sum2 = 0.0;
    for (int i = c; i < P.n; i += kG) {
        const Pt p = pt_load(P, i);
        const double Xc = R[0][0] * p.X + R[0][1] * p.Y + R[0][2] * p.Z + t[0];
        const double Yc = R[1][0] * p.X + R[1][1] * p.Y + R[1][2] * p.Z + t[1];
        const double inv_Zc = 1.0 / (R[2][0] * p.X + R[2][1] * p.Y + R[2][2] * p.Z + t[2]);
        const double ue = P.uc + P.fu * Xc * inv_Zc, ve = P.vc + P.fv * Yc * inv_Zc;
        sum2 += sqrt((p.u - ue) * (p.u - ue) + (p.v - ve) * (p.v - ve));
    }
    return oslam::row16_sum(sum2) / n;
}

__device__ inline void gauss_newton(const double* L, const double* rho, double betas[4]) {
    for (int it = 0; it < 5; it++) {
        double A[24], b[6], x[4];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const double* rowL = &L[i * 10];
            A[i * 4 + 0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
            A[i * 4 + 1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
            A[i * 4 + 2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
            A[i * 4 + 3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
            b[i] = rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] + rowL[3] * betas[0] * betas[2] +
                             rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] + rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] +
                             rowL[8] * betas[2] * betas[3] + rowL[9] * betas[3] * betas[3]);
        }
        qr_solve6<4>(A, b, x);
#pragma unroll
        for (int i = 0; i < 4; i++) betas[i] += x[i];
    }
}

// compute_pose (:477-525) over the points of P by one group of 16 lanes (c = lane of the group); every lane returns the same R, t and error.
// All groups of the workgroup call it together with the same P.n (it synchronises the workgroup).
__device__ inline double epnp_group(const PnpPts& P, PnpLds& S, int c, double R[3][3], double t[3]) {
    Epnp E;
    const double n = (double)P.n;
    // ---- choose_control_points (:375-409) ----
    double s3[3] = {0, 0, 0};
    for (int i = c; i < P.n; i += kG) { const Pt p = pt_load(P, i); s3[0] += p.X; s3[1] += p.Y; s3[2] += p.Z; }
#pragma unroll
    for (int j = 0; j < 3; j++) E.cws0[j] = oslam::row16_sum(s3[j]) / n;
    double C6[6] = {0, 0, 0, 0, 0, 0};   // PW0^T PW0, upper triangle
    for (int i = c; i < P.n; i += kG) {
        const Pt p = pt_load(P, i);
        const double dx = p.X - E.cws0[0], dy = p.Y - E.cws0[1], dz = p.Z - E.cws0[2];
        C6[0] += dx * dx; C6[1] += dx * dy; C6[2] += dx * dz; C6[3] += dy * dy; C6[4] += dy * dz; C6[5] += dz * dz;
    }
#pragma unroll
    for (int j = 0; j < 6; j++) C6[j] = oslam::row16_sum(C6[j]);
    {
        const double Cm[3][3] = {{C6[0], C6[1], C6[2]}, {C6[1], C6[3], C6[4]}, {C6[2], C6[4], C6[5]}};
        double U[3][3], w[3], V[3][3];
        svd3(Cm, U, w, V);
        // descending singular values, ties by index (cvSVD's order)
        int ord[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            int rank = 0;
#pragma unroll
            for (int j = 0; j < 3; j++) rank += (w[j] > w[i] || (w[j] == w[i] && j < i)) ? 1 : 0;
            ord[i] = rank;
        }
        double kk[3] = {0, 0, 0}, ax[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int r = 0; r < 3; r++)
                if (ord[i] == r) { kk[r] = sqrt(w[i] / n); ax[r][0] = U[0][i]; ax[r][1] = U[1][i]; ax[r][2] = U[2][i]; }
        // the sign of an axis is the SVD's choice in the reference (and moves a noisy solution at the 1e-3 level): here its largest component is positive
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const double a0 = fabs(ax[r][0]), a1 = fabs(ax[r][1]), a2 = fabs(ax[r][2]);
            const double lead = (a0 >= a1 && a0 >= a2) ? ax[r][0] : (a1 >= a2 ? ax[r][1] : ax[r][2]);
            if (lead < 0) { ax[r][0] = -ax[r][0]; ax[r][1] = -ax[r][1]; ax[r][2] = -ax[r][2]; }
        }
        // CC = [k_1 u_1 | k_2 u_2 | k_3 u_3] with orthonormal u: its (pseudo-)inverse has the rows u_j / k_j; a k_j below the threshold of cvInvert(CV_SVD) gives a zero row
        const double thr = (kk[0] + kk[1] + kk[2]) * 2.0 * DBL_EPSILON;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double inv = kk[j] > thr ? 1.0 / kk[j] : 0.0;
#pragma unroll
            for (int m = 0; m < 3; m++) { E.cw[j][m] = kk[j] * ax[j][m]; E.ci[j][m] = ax[j][m] * inv; }
        }
    }
    // ---- MtM (:482-492) straight from the correspondences: lane c owns entries c, c + 16, .. of the 12 x 12 image and adds the points in order ----
    {
        double acc[9];
        int qj[9], mj[9], qk[9], mk[9];
#pragma unroll
        for (int m = 0; m < 9; m++) {
            const int e = c + kG * m, j = e / 12, k = e % 12;
            acc[m] = 0.0; qj[m] = j / 3; mj[m] = j % 3; qk[m] = k / 3; mk[m] = k % 3;
        }
        for (int i = 0; i < P.n; i++) {
            const Pt p = pt_load(P, i);
            double a[4];
            alphas_of(E, p, a);
            const double du = P.uc - p.u, dv = P.vc - p.v;
#pragma unroll
            for (int m = 0; m < 9; m++) {
                const double aj = qj[m] == 0 ? a[0] : qj[m] == 1 ? a[1] : qj[m] == 2 ? a[2] : a[3];
                const double ak = qk[m] == 0 ? a[0] : qk[m] == 1 ? a[1] : qk[m] == 2 ? a[2] : a[3];
                const double m1j = mj[m] == 0 ? aj * P.fu : mj[m] == 1 ? 0.0 : aj * du, m2j = mj[m] == 0 ? 0.0 : mj[m] == 1 ? aj * P.fv : aj * dv;
                const double m1k = mk[m] == 0 ? ak * P.fu : mk[m] == 1 ? 0.0 : ak * du, m2k = mk[m] == 0 ? 0.0 : mk[m] == 1 ? ak * P.fv : ak * dv;
                acc[m] += m1j * m1k + m2j * m2k;
            }
        }
#pragma unroll
        for (int m = 0; m < 9; m++) {
            const int e = c + kG * m;
            S.A[e] = acc[m];
            S.V[e] = (e / 12 == e % 12) ? 1.0 : 0.0;
        }
    }
    __syncthreads();
    jacobi12(S, c);
    {   // the four smallest eigenvalues, ascending, ties by index
        double d[12];
#pragma unroll
        for (int i = 0; i < 12; i++) d[i] = S.A[i * 12 + i];
#pragma unroll
        for (int r = 0; r < 4; r++) E.vidx[r] = 0;
#pragma unroll
        for (int i = 0; i < 12; i++) {
            int rank = 0;
#pragma unroll
            for (int j = 0; j < 12; j++) rank += (d[j] < d[i] || (d[j] == d[i] && j < i)) ? 1 : 0;
#pragma unroll
            for (int r = 0; r < 4; r++) if (rank == r) E.vidx[r] = i;
        }
    }
    // ---- compute_L_6x10 (:760-800), compute_rho (:802-810): lane i < 6 takes row i = the control-point pair (a, b) in the order 01 02 03 12 13 23 ----
    if (c < 6) {
        const int a = c < 3 ? 0 : c < 5 ? 1 : 2, b = c < 3 ? c + 1 : c < 5 ? c - 1 : 3;
        double dv[4][3];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) dv[i][k] = S.V[(3 * a + k) * 12 + E.vidx[i]] - S.V[(3 * b + k) * 12 + E.vidx[i]];
        auto dot = [](const double* x, const double* y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; };
        double* row = &S.L[10 * c];
        row[0] = dot(dv[0], dv[0]);
        row[1] = 2.0 * dot(dv[0], dv[1]);
        row[2] = dot(dv[1], dv[1]);
        row[3] = 2.0 * dot(dv[0], dv[2]);
        row[4] = 2.0 * dot(dv[1], dv[2]);
        row[5] = dot(dv[2], dv[2]);
        row[6] = 2.0 * dot(dv[0], dv[3]);
        row[7] = 2.0 * dot(dv[1], dv[3]);
        row[8] = 2.0 * dot(dv[2], dv[3]);
        row[9] = dot(dv[3], dv[3]);
        // dist2(cws[a], cws[b]) with cws[j] - cws[0] = cw[j - 1]
        double d2 = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double xa = a == 0 ? 0.0 : a == 1 ? E.cw[0][k] : E.cw[1][k], xb = b == 1 ? E.cw[0][k] : b == 2 ? E.cw[1][k] : E.cw[2][k];
            d2 += (xa - xb) * (xa - xb);
        }
        S.rho[c] = d2;
    }
    __syncthreads();
    const double* L = S.L;
    const double* rho = S.rho;
    // ---- the three beta initialisations (:667-758), each refined by gauss_newton; cvSolve(CV_SVD) is the least-squares solution, here by the same Householder QR ----
    double best_err = 0.0;
    double Rb[3][3], tb[3];
    for (int method = 1; method <= 3; method++) {
        double betas[4] = {0, 0, 0, 0};
        double rb[6];
#pragma unroll
        for (int i = 0; i < 6; i++) rb[i] = rho[i];
        if (method == 1) {
            double A[24], b4[4];
#pragma unroll
            for (int i = 0; i < 6; i++) { A[i * 4] = L[i * 10]; A[i * 4 + 1] = L[i * 10 + 1]; A[i * 4 + 2] = L[i * 10 + 3]; A[i * 4 + 3] = L[i * 10 + 6]; }
            qr_solve6<4>(A, rb, b4);
            if (b4[0] < 0) { betas[0] = sqrt(-b4[0]); betas[1] = -b4[1] / betas[0]; betas[2] = -b4[2] / betas[0]; betas[3] = -b4[3] / betas[0]; }
            else { betas[0] = sqrt(b4[0]); betas[1] = b4[1] / betas[0]; betas[2] = b4[2] / betas[0]; betas[3] = b4[3] / betas[0]; }
        } else if (method == 2) {
            double A[18], b3[3];
#pragma unroll
            for (int i = 0; i < 6; i++) { A[i * 3] = L[i * 10]; A[i * 3 + 1] = L[i * 10 + 1]; A[i * 3 + 2] = L[i * 10 + 2]; }
            qr_solve6<3>(A, rb, b3);
            if (b3[0] < 0) { betas[0] = sqrt(-b3[0]); betas[1] = (b3[2] < 0) ? sqrt(-b3[2]) : 0.0; }
            else { betas[0] = sqrt(b3[0]); betas[1] = (b3[2] > 0) ? sqrt(b3[2]) : 0.0; }
            if (b3[1] < 0) betas[0] = -betas[0];
            betas[2] = 0.0; betas[3] = 0.0;
        } else {
            double A[30], b5[5];
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int k = 0; k < 5; k++) A[i * 5 + k] = L[i * 10 + k];
            qr_solve6<5>(A, rb, b5);
            if (b5[0] < 0) { betas[0] = sqrt(-b5[0]); betas[1] = (b5[2] < 0) ? sqrt(-b5[2]) : 0.0; }
            else { betas[0] = sqrt(b5[0]); betas[1] = (b5[2] > 0) ? sqrt(b5[2]) : 0.0; }
            if (b5[1] < 0) betas[0] = -betas[0];
            betas[2] = b5[3] / betas[0];
            betas[3] = 0.0;
        }
        gauss_newton(L, rho, betas);
        double Rm[3][3], tm[3];
        const double err = compute_R_and_t(P, E, S, betas, c, Rm, tm);
        // int N = 1; if (rep_errors[2] < rep_errors[1]) N = 2; if (rep_errors[3] < rep_errors[N]) N = 3;
        if (method == 1 || err < best_err) {
            best_err = err;
#pragma unroll
            for (int i = 0; i < 3; i++) { tb[i] = tm[i]; for (int j = 0; j < 3; j++) Rb[i][j] = Rm[i][j]; }
        }
    }
#pragma unroll
    for (int i = 0; i < 3; i++) { t[i] = tb[i]; for (int j = 0; j < 3; j++) R[i][j] = Rb[i][j]; }
    __syncthreads();   // S is free again
    return best_err;
}

__device__ __forceinline__ bool pose_finite(const double R[3][3], const double t[3]) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; i++) { ok = ok && isfinite(t[i]); for (int j = 0; j < 3; j++) ok = ok && isfinite(R[i][j]); }
    return ok;
}

struct PnpProblemDev { const float* p3; const float* p2; const float* sig; int N; double fu, fv, uc, vc; float th2; };

// CheckInliers (:308-339) of correspondence i: Xc, Yc, invZc, distX, distY, error2 float; ue, ve double; strict comparison against mvMaxError[i] = sigma2[i] * th2.
__device__ __forceinline__ bool is_inlier(const PnpProblemDev& Q, const double R[3][3], const double t[3], int i) {
    const float x = Q.p3[3 * i], y = Q.p3[3 * i + 1], z = Q.p3[3 * i + 2];
    const float Xc = (float)(R[0][0] * x + R[0][1] * y + R[0][2] * z + t[0]);
    const float Yc = (float)(R[1][0] * x + R[1][1] * y + R[1][2] * z + t[1]);
    const float invZc = (float)(1 / (R[2][0] * x + R[2][1] * y + R[2][2] * z + t[2]));
    const double ue = Q.uc + Q.fu * Xc * invZc;
    const double ve = Q.vc + Q.fv * Yc * invZc;
    const float distX = (float)(Q.p2[2 * i] - ue);
    const float distY = (float)(Q.p2[2 * i + 1] - ve);
    const float error2 = distX * distX + distY * distY;
    const float maxError = Q.sig[i] * Q.th2;
    return error2 < maxError;
}

// The count over all N by the group's lanes; `sel` (or NULL) receives the inlier indices in ascending order, `flags` (or NULL) the inlier bytes.
// A pose that is not finite counts zero.
__device__ inline int check_inliers(const PnpProblemDev& Q, const double R[3][3], const double t[3], int c, int lane_base, int* sel, uint8_t* flags) {
    const bool fin = pose_finite(R, t);
    int cnt = 0, placed = 0;
    for (int base = 0; base < Q.N; base += kG) {
        const int i = base + c;
        const bool in = i < Q.N && fin && is_inlier(Q, R, t, i);
        cnt += in ? 1 : 0;
        if (flags && i < Q.N) flags[i] = in ? 1 : 0;
        if (sel) {
            const uint32_t m = (uint32_t)((__ballot(in) >> lane_base) & 0xffffull);
            if (in) sel[placed + __popc(m & ((1u << c) - 1u))] = i;
            placed += __popc(m);
        }
    }
    return oslam::row16_sum_i32(cnt);
}

struct PnpArgs {
    const oslam_pnp_problem_t* problems;
    const float* p3; const float* p2; const float* sig;
    int n_corr;           // entries of the packed arrays
    int it_stride;        // = params.max_iterations: row length of samples, iter_inliers and the arena
    oslam_pnp_params_t prm;
    const int32_t* samples;
    double* pose; int32_t* counts; int32_t* sel;   // arena
    float* Tcw; uint8_t* inliers; int32_t* status; int32_t* iter_inliers;
};

__device__ __forceinline__ bool problem_valid(const oslam_pnp_problem_t& pr, int n_corr) {
    return pr.count >= 0 && pr.offset >= 0 && pr.count <= n_corr && pr.offset <= n_corr - pr.count;
}
__device__ __forceinline__ PnpProblemDev problem_dev(const PnpArgs& a, const oslam_pnp_problem_t& pr) {
    PnpProblemDev Q;
    Q.p3 = a.p3 + 3 * (size_t)pr.offset; Q.p2 = a.p2 + 2 * (size_t)pr.offset; Q.sig = a.sig + pr.offset;
    Q.N = pr.count; Q.fu = pr.fx; Q.fv = pr.fy; Q.uc = pr.cx; Q.vc = pr.cy; Q.th2 = a.prm.th2;
    return Q;
}

// One hypothesis per group of 16 lanes: grid (ceil(max_iterations / 4), problems), 64 threads.  Workgroups beyond a problem's iteration count leave at once.
__global__ __launch_bounds__(kG* kHypPerBlock) void k_pnp_hypotheses(PnpArgs a) {
    __shared__ PnpLds s_lds[kHypPerBlock];
    __shared__ int s_sel[kHypPerBlock][4];
    const int b = blockIdx.y;
    const oslam_pnp_problem_t pr = a.problems[b];
    if (!problem_valid(pr, a.n_corr)) return;
    const RansacAdj ra = ransac_adjust(pr.count, a.prm.probability, a.prm.min_inliers, a.prm.max_iterations, a.prm.min_set, a.prm.epsilon);
    const int first = blockIdx.x * kHypPerBlock;
    if (ra.no_more || first >= ra.iterations) return;   // (uniform over the workgroup)
    const int g = threadIdx.x / kG, c = threadIdx.x % kG, lane_base = (threadIdx.x & 63) & ~(kG - 1);
    const bool live = first + g < ra.iterations;
    const int it = live ? first + g : ra.iterations - 1;   // a spare group repeats the last iteration and writes nothing
    int idx[4];
    bool ok = true;
    if (a.samples) {
        const int32_t* s = a.samples + ((size_t)b * a.it_stride + it) * 4;
#pragma unroll
        for (int k = 0; k < 4; k++) { idx[k] = s[k]; ok = ok && idx[k] >= 0 && idx[k] < pr.count; }
        ok = ok && idx[0] != idx[1] && idx[0] != idx[2] && idx[0] != idx[3] && idx[1] != idx[2] && idx[1] != idx[3] && idx[2] != idx[3];
    } else {
        oslam::ransac_draw<4>(pr.seed, it, pr.count, idx);
    }
    if (c < 4) s_sel[g][c] = ok ? idx[c] : c;   // (count >= min_inliers >= min_set = 4)
    __syncthreads();
    const PnpProblemDev Q = problem_dev(a, pr);
    PnpPts P;
    P.p3 = Q.p3; P.p2 = Q.p2; P.sel = s_sel[g]; P.n = 4; P.fu = Q.fu; P.fv = Q.fv; P.uc = Q.uc; P.vc = Q.vc;
    double R[3][3], t[3];
    epnp_group(P, s_lds[g], c, R, t);
    int cnt = check_inliers(Q, R, t, c, lane_base, nullptr, nullptr);
    if (!ok) cnt = 0;
    if (live && c == 0) {
        const size_t o = (size_t)b * a.it_stride + it;
        a.counts[o] = cnt;
        double* po = a.pose + o * 12;
#pragma unroll
        for (int i = 0; i < 3; i++) { po[9 + i] = t[i]; for (int j = 0; j < 3; j++) po[3 * i + j] = R[i][j]; }
    }
}

__device__ inline void write_Tcw(float* T, const double R[3][3], const double t[3]) {   // convertTo(CV_32F) into eye(4, 4) (:217-223, :294-300)
#pragma unroll
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) T[4 * i + j] = (float)R[i][j]; T[4 * i + 3] = (float)t[i]; }
    T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}

// iterate() (:165-258) over the counts of the hypotheses, one workgroup of 16 lanes per problem.  Refine() depends on the best set alone, so only the
// record iterations (count >= minInliers and above every earlier count) can change the outcome: the result is the first record whose Refine succeeds,
// otherwise the last record unrefined.
__global__ __launch_bounds__(kG) void k_pnp_select(PnpArgs a) {
    __shared__ PnpLds s_lds;
    const int b = blockIdx.x, c = threadIdx.x;
    const oslam_pnp_problem_t pr = a.problems[b];
    int32_t* st = a.status + 4 * (size_t)b;
    if (!problem_valid(pr, a.n_corr)) { if (c == 0) { st[0] = -1; st[1] = 0; st[2] = 0; st[3] = -1; } return; }
    const RansacAdj ra = ransac_adjust(pr.count, a.prm.probability, a.prm.min_inliers, a.prm.max_iterations, a.prm.min_set, a.prm.epsilon);
    if (ra.no_more) { if (c == 0) { st[0] = 0; st[1] = 0; st[2] = 0; st[3] = -1; } return; }
    const PnpProblemDev Q = problem_dev(a, pr);
    {   // input validation: a problem with a number that is not finite has no pose (its hypotheses are not looked at)
        int bad = (isfinite(pr.fx) && isfinite(pr.fy) && isfinite(pr.cx) && isfinite(pr.cy)) ? 0 : 1;
        for (int i = c; i < Q.N; i += kG)
            bad |= (isfinite(Q.p3[3 * i]) && isfinite(Q.p3[3 * i + 1]) && isfinite(Q.p3[3 * i + 2]) && isfinite(Q.p2[2 * i]) && isfinite(Q.p2[2 * i + 1]) && isfinite(Q.sig[i])) ? 0 : 1;
        if (oslam::row16_sum_i32(bad) != 0) { if (c == 0) { st[0] = 0; st[1] = 0; st[2] = 0; st[3] = -1; } return; }
    }
    const size_t o = (size_t)b * a.it_stride;
    int* sel = a.sel + pr.offset;
    uint8_t* flags = a.inliers + pr.offset;
    float* Tcw = a.Tcw + 16 * (size_t)b;
    if (a.iter_inliers)
        for (int it = c; it < ra.iterations; it += kG) a.iter_inliers[o + it] = a.counts[o + it];
    int best = 0, last = -1;
    for (int it = 0; it < ra.iterations; it++) {
        const int cnt = a.counts[o + it];
        if (cnt < ra.min_inliers || cnt <= best) continue;   // (uniform: every lane reads the same count)
        best = cnt; last = it;
        double R[3][3], t[3];
        const double* po = a.pose + (o + it) * 12;
#pragma unroll
        for (int i = 0; i < 3; i++) { t[i] = po[9 + i]; for (int j = 0; j < 3; j++) R[i][j] = po[3 * i + j]; }
        const int n = check_inliers(Q, R, t, c, 0, sel, nullptr);   // mvbBestInliers as an index list (n == cnt)
        __syncthreads();
        PnpPts P;
        P.p3 = Q.p3; P.p2 = Q.p2; P.sel = sel; P.n = n; P.fu = Q.fu; P.fv = Q.fv; P.uc = Q.uc; P.vc = Q.vc;
        double Rr[3][3], tr[3];
        epnp_group(P, s_lds, c, Rr, tr);
        const int nref = check_inliers(Q, Rr, tr, c, 0, nullptr, nullptr);
        if (nref > ra.min_inliers) {   // Refine() succeeded (:292)
            check_inliers(Q, Rr, tr, c, 0, nullptr, flags);
            if (c == 0) { write_Tcw(Tcw, Rr, tr); st[0] = 1; st[1] = nref; st[2] = it + 1; st[3] = it; }
            return;
        }
    }
    if (last >= 0) {   // bNoMore: the best unrefined pose (:241-255)
        double R[3][3], t[3];
        const double* po = a.pose + (o + last) * 12;
#pragma unroll
        for (int i = 0; i < 3; i++) { t[i] = po[9 + i]; for (int j = 0; j < 3; j++) R[i][j] = po[3 * i + j]; }
        check_inliers(Q, R, t, c, 0, nullptr, flags);
        if (c == 0) { write_Tcw(Tcw, R, t); st[0] = 2; st[1] = best; st[2] = ra.iterations; st[3] = last; }
    } else if (c == 0) { st[0] = 0; st[1] = 0; st[2] = ra.iterations; st[3] = -1; }
}

// compute_pose alone: one workgroup of 16 lanes per set.
__global__ __launch_bounds__(kG) void k_pnp_epnp(const int32_t* counts, const int32_t* offsets, const float* p3, const float* p2, double fu, double fv, double uc, double vc,
                                                 double* outR, double* outT, double* outErr) {
    __shared__ PnpLds s_lds;
    const int b = blockIdx.x, c = threadIdx.x;
    PnpPts P;
    P.p3 = p3 + 3 * (size_t)offsets[b]; P.p2 = p2 + 2 * (size_t)offsets[b]; P.sel = nullptr; P.n = counts[b]; P.fu = fu; P.fv = fv; P.uc = uc; P.vc = vc;
    double R[3][3], t[3];
    const double err = epnp_group(P, s_lds, c, R, t);
    if (c == 0) {
#pragma unroll
        for (int i = 0; i < 3; i++) { outT[3 * (size_t)b + i] = t[i]; for (int j = 0; j < 3; j++) outR[9 * (size_t)b + 3 * i + j] = R[i][j]; }
        outErr[b] = err;
    }
}

int check_params(const char* fn, const oslam_pnp_t* h, const oslam_pnp_params_t* p) {
    if (!p) { set_error("%s: params is NULL", fn); return OSLAM_E_INVALID; }
    if (p->min_set != 4) { set_error("%s: min_set = %d: only the minimal set of 4 is implemented", fn, p->min_set); return OSLAM_E_INVALID; }
    if (p->max_iterations < 1 || !(p->probability > 0.0 && p->probability < 1.0) || !(p->epsilon >= 0.f) || !(p->th2 >= 0.f)) {
        set_error("%s: bad parameter block", fn);
        return OSLAM_E_INVALID;
    }
    if (p->max_iterations > h->max_iterations) {
        set_error("%s: max_iterations = %d exceeds the handle's %d", fn, p->max_iterations, h->max_iterations);
        return OSLAM_E_CAPACITY;
    }
    return OSLAM_OK;
}

}  // namespace

extern "C" {

int oslam_pnp_ransac_params(int N, double probability, int min_inliers, int max_iterations, int min_set, float epsilon, oslam_pnp_ransac_t* out) {
    if (!out || N < 0 || max_iterations < 1) { set_error("oslam_pnp_ransac_params: bad argument"); return OSLAM_E_INVALID; }
    const RansacAdj r = ransac_adjust(N, probability, min_inliers, max_iterations, min_set, epsilon);
    out->min_inliers = r.min_inliers; out->epsilon = r.epsilon; out->iterations = r.iterations; out->no_more = r.no_more;
    return OSLAM_OK;
}

int oslam_pnp_draw(uint32_t seed, int iteration, int N, int32_t idx[4]) {
    if (!idx || N < 4 || iteration < 0) { set_error("oslam_pnp_draw: bad argument"); return OSLAM_E_INVALID; }
    int v[4];
    oslam::ransac_draw<4>(seed, iteration, N, v);
    for (int k = 0; k < 4; k++) idx[k] = v[k];
    return OSLAM_OK;
}

void oslam_pnp_destroy(oslam_pnp_t* h) {
    if (!h) return;
    delete h;
}

int oslam_pnp_create(oslam_pnp_t** out, int max_problems, int max_correspondences_total, int max_iterations) {
    if (!out) { set_error("oslam_pnp_create: out is NULL"); return OSLAM_E_INVALID; }
    *out = nullptr;
    if (max_problems < 1 || max_correspondences_total < 1 || max_iterations < 1 || max_problems > 65535 * 16) { set_error("oslam_pnp_create: bad argument"); return OSLAM_E_INVALID; }
    if (oslam_device_count() <= 0) return oslam::no_device("oslam_pnp_create");
    oslam_pnp* h = new oslam_pnp;
    h->max_problems = max_problems; h->max_corr = max_correspondences_total; h->max_iterations = max_iterations;
    const size_t hyp = (size_t)max_problems * max_iterations;
    int rc;
    if ((rc = h->pose.alloc(hyp * 12 * sizeof(double))) || (rc = h->counts.alloc(hyp * sizeof(int32_t))) || (rc = h->sel.alloc((size_t)max_correspondences_total * sizeof(int32_t)))) {
        delete h;
        return rc;
    }
    *out = h;
    return OSLAM_OK;
}

int oslam_pnp_ransac_batch_device(oslam_pnp_t* h, int n_problems, const oslam_pnp_problem_t* d_problems, int n_corr, const float* d_P3Dw, const float* d_P2D,
                                  const float* d_sigma2, const oslam_pnp_params_t* params, const int32_t* d_samples, float* d_Tcw, uint8_t* d_inliers,
                                  int32_t* d_status, int32_t* d_iter_inliers, void* stream) {
    if (!h || n_problems < 0 || n_corr < 0 || !d_status || (n_problems > 0 && (!d_problems || !d_Tcw)) || (n_corr > 0 && (!d_P3Dw || !d_P2D || !d_sigma2 || !d_inliers))) {
        set_error("oslam_pnp_ransac_batch_device: bad argument");
        return OSLAM_E_INVALID;
    }
    OSLAM_CHECK(check_params("oslam_pnp_ransac_batch_device", h, params));
    if (n_problems > h->max_problems || n_corr > h->max_corr) {
        set_error("oslam_pnp_ransac_batch_device: %d problems / %d correspondences exceed the handle's %d / %d", n_problems, n_corr, h->max_problems, h->max_corr);
        return OSLAM_E_CAPACITY;
    }
    if (n_problems == 0) return OSLAM_OK;
    PnpArgs a;
    a.problems = d_problems; a.p3 = d_P3Dw; a.p2 = d_P2D; a.sig = d_sigma2; a.n_corr = n_corr; a.it_stride = params->max_iterations; a.prm = *params;
    a.samples = d_samples; a.pose = h->pose.as<double>(); a.counts = h->counts.as<int32_t>(); a.sel = h->sel.as<int32_t>();
    a.Tcw = d_Tcw; a.inliers = d_inliers; a.status = d_status; a.iter_inliers = d_iter_inliers;
    const int gx = oslam::div_up(params->max_iterations, kHypPerBlock);
    for (int at = 0; at < n_problems; at += 65535) {   // (grid.y limit)
        const int m = std::min(n_problems - at, 65535);
        PnpArgs s = a;
        s.problems += at; s.pose += (size_t)at * a.it_stride * 12; s.counts += (size_t)at * a.it_stride;
        if (s.samples) s.samples += (size_t)at * a.it_stride * 4;
        hipLaunchKernelGGL(k_pnp_hypotheses, dim3(gx, m), dim3(kG * kHypPerBlock), 0, (hipStream_t)stream, s);
    }
    hipLaunchKernelGGL(k_pnp_select, dim3(n_problems), dim3(kG), 0, (hipStream_t)stream, a);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int oslam_pnp_ransac_batch(oslam_pnp_t* h, int n_problems, const oslam_pnp_problem_t* problems, int n_corr, const float* P3Dw, const float* P2D, const float* sigma2,
                           const oslam_pnp_params_t* params, const int32_t* samples, float* Tcw, uint8_t* inliers, int32_t* status, int32_t* iter_inliers) {
    if (!h || n_problems < 0 || n_corr < 0 || (n_problems > 0 && (!problems || !Tcw || !status)) || (n_corr > 0 && (!P3Dw || !P2D || !sigma2 || !inliers))) {
        set_error("oslam_pnp_ransac_batch: bad argument");
        return OSLAM_E_INVALID;
    }
    OSLAM_CHECK(check_params("oslam_pnp_ransac_batch", h, params));
    if (n_problems > h->max_problems || n_corr > h->max_corr) {
        set_error("oslam_pnp_ransac_batch: %d problems / %d correspondences exceed the handle's %d / %d", n_problems, n_corr, h->max_problems, h->max_corr);
        return OSLAM_E_CAPACITY;
    }
    for (int b = 0; b < n_problems; b++) {
        const oslam_pnp_problem_t& pr = problems[b];
        if (pr.count < 0 || pr.offset < 0 || pr.count > n_corr || pr.offset > n_corr - pr.count) {
            set_error("oslam_pnp_ransac_batch: problem %d (offset %d, count %d) lies outside the %d correspondences", b, pr.offset, pr.count, n_corr);
            return OSLAM_E_INVALID;
        }
    }
    if (n_problems == 0) return OSLAM_OK;
    std::lock_guard<std::mutex> lock(h->mu);
    const size_t np = (size_t)n_problems, nc = (size_t)n_corr, its = (size_t)params->max_iterations;
    oslam::StageLayout up, down;   // one upload, one download
    const auto uProb = up.add<oslam_pnp_problem_t>(np);
    const auto uP3 = up.add<float>(nc * 3), uP2 = up.add<float>(nc * 2), uSig = up.add<float>(nc);
    const auto uSam = up.add<int32_t>(np * its * 4, samples != nullptr);
    const auto dSt = down.add<int32_t>(np * 4);
    const auto dT = down.add<float>(np * 16);
    const auto dIn = down.add<uint8_t>(nc);
    const auto dIt = down.add<int32_t>(np * its, iter_inliers != nullptr);
    OSLAM_CHECK(h->up.grow(up.total(), 4096));
    OSLAM_CHECK(h->down.grow(down.total(), 4096));
    uint8_t *uh = h->up.h.bytes(), *ud = h->up.d.bytes(), *dh = h->down.h.bytes(), *dd = h->down.d.bytes();
    put(uProb, uh, problems); put(uP3, uh, P3Dw); put(uP2, uh, P2D); put(uSig, uh, sigma2); put(uSam, uh, samples);
    OSLAM_HIP_CHECK(hipMemcpyAsync(ud, uh, up.total(), hipMemcpyHostToDevice, nullptr));
    if (iter_inliers) OSLAM_HIP_CHECK(hipMemsetAsync(at(dIt, dd), 0xff, dIt.bytes, nullptr));   // -1 = not run
    OSLAM_CHECK(oslam_pnp_ransac_batch_device(h, n_problems, at(uProb, ud), n_corr, at(uP3, ud), at(uP2, ud), at(uSig, ud), params, at(uSam, ud), at(dT, dd), at(dIn, dd),
                                              at(dSt, dd), at(dIt, dd), nullptr));
    OSLAM_HIP_CHECK(hipMemcpyAsync(dh, dd, down.total(), hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(dSt, dh, status); get(dIt, dh, iter_inliers);
    for (int b = 0; b < n_problems; b++) {   // a problem without a pose keeps the caller's Tcw and inlier bytes
        if (status[4 * b] <= 0) continue;
        memcpy(Tcw + 16 * (size_t)b, at(dT, dh) + 16 * (size_t)b, 16 * sizeof(float));
        memcpy(inliers + problems[b].offset, at(dIn, dh) + problems[b].offset, (size_t)problems[b].count);
    }
    return OSLAM_OK;
}

int oslam_pnp_epnp(oslam_pnp_t* h, int n_sets, const int32_t* counts, const int32_t* offsets, int n_corr, const float* P3Dw, const float* P2D, const float K4[4], double* R,
                   double* t, double* err) {
    if (!h || n_sets < 0 || n_corr < 0 || !K4 || (n_sets > 0 && (!counts || !offsets || !P3Dw || !P2D || !R || !t || !err))) {
        set_error("oslam_pnp_epnp: bad argument");
        return OSLAM_E_INVALID;
    }
    if (n_sets > h->max_problems || n_corr > h->max_corr) {
        set_error("oslam_pnp_epnp: %d sets / %d correspondences exceed the handle's %d / %d", n_sets, n_corr, h->max_problems, h->max_corr);
        return OSLAM_E_CAPACITY;
    }
    for (int b = 0; b < n_sets; b++)
        if (counts[b] < 4 || offsets[b] < 0 || counts[b] > n_corr || offsets[b] > n_corr - counts[b]) {
            set_error("oslam_pnp_epnp: set %d (offset %d, count %d): at least 4 points inside the %d correspondences", b, offsets[b], counts[b], n_corr);
            return OSLAM_E_INVALID;
        }
    if (n_sets == 0) return OSLAM_OK;
    std::lock_guard<std::mutex> lock(h->mu);
    const size_t ns = (size_t)n_sets, nc = (size_t)n_corr;
    oslam::StageLayout up, down;
    const auto uCnt = up.add<int32_t>(ns), uOff = up.add<int32_t>(ns);
    const auto uP3 = up.add<float>(nc * 3), uP2 = up.add<float>(nc * 2);
    const auto dR = down.add<double>(ns * 9), dT = down.add<double>(ns * 3), dE = down.add<double>(ns);
    OSLAM_CHECK(h->up.grow(up.total(), 4096));
    OSLAM_CHECK(h->down.grow(down.total(), 4096));
    uint8_t *uh = h->up.h.bytes(), *ud = h->up.d.bytes(), *dh = h->down.h.bytes(), *dd = h->down.d.bytes();
    put(uCnt, uh, counts); put(uOff, uh, offsets); put(uP3, uh, P3Dw); put(uP2, uh, P2D);
    OSLAM_HIP_CHECK(hipMemcpyAsync(ud, uh, up.total(), hipMemcpyHostToDevice, nullptr));
    hipLaunchKernelGGL(k_pnp_epnp, dim3(n_sets), dim3(kG), 0, nullptr, at(uCnt, ud), at(uOff, ud), at(uP3, ud), at(uP2, ud), (double)K4[0], (double)K4[1], (double)K4[2],
                       (double)K4[3], at(dR, dd), at(dT, dd), at(dE, dd));
    OSLAM_HIP_CHECK(hipGetLastError());
    OSLAM_HIP_CHECK(hipMemcpyAsync(dh, dd, down.total(), hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(dR, dh, R); get(dT, dh, t); get(dE, dh, err);
    return OSLAM_OK;
}

}  // extern "C"
