// Singular value decompositions of 3 x 3 and 4 x 4 matrices in registers, shared by the solvers: svd3 (fp64, EPnP's estimate_R_and_t and control points,
// the Initializer's rank-2 projection and motion decompositions) and svd4_last_row (float, the DLT of Triangulate in LocalMapping::CreateNewMapPoints
// and in Initializer::CheckRT).
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

namespace oslam {

constexpr int kSvd3Sweeps = 12;

// A = U diag(w) V^T by one-sided Jacobi rotations on the columns (the method of cv::SVD), in registers.  Columns of U that belong to w = 0 are zero.
__device__ inline void svd3(const double A[3][3], double U[3][3], double w[3], double V[3][3]) {
    double B[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) { B[i][j] = A[i][j]; V[i][j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < kSvd3Sweeps; sweep++) {
#pragma unroll
        for (int pr = 0; pr < 3; pr++) {
            const int i = pr == 2 ? 1 : 0, j = pr == 0 ? 1 : 2;
            double a = 0, b = 0, g = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) { a += B[k][i] * B[k][i]; b += B[k][j] * B[k][j]; g += B[k][i] * B[k][j]; }
            if (fabs(g) > DBL_EPSILON * sqrt(a * b)) {
                const double zeta = (b - a) / (2.0 * g);
                const double t = (zeta < 0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const double bi = B[k][i], bj = B[k][j];
                    B[k][i] = c * bi - s * bj; B[k][j] = s * bi + c * bj;
                    const double vi = V[k][i], vj = V[k][j];
                    V[k][i] = c * vi - s * vj; V[k][j] = s * vi + c * vj;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        w[j] = sqrt(B[0][j] * B[0][j] + B[1][j] * B[1][j] + B[2][j] * B[2][j]);
        const double inv = w[j] > 0 ? 1.0 / w[j] : 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) U[k][j] = B[k][j] * inv;
    }
}

// one Jacobi rotation between rows I and J of At (and of Vt); returns whether it rotated
template <int I, int J>
__device__ __forceinline__ bool jacobi_pair(float (&At)[16], float (&Vt)[16], double (&W)[4]) {
    double a = W[I], b = W[J], p = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) p += (double)At[I * 4 + k] * (double)At[J * 4 + k];
    const float eps = 2.0f * 1.1920928955078125e-07f;
    if (fabs(p) <= (double)eps * sqrt(a * b)) return false;
    p *= 2;
    const double beta = a - b, gamma = hypot(p, beta);
    float c, s;
    if (beta < 0) {
        const double delta = (gamma - beta) * 0.5;
        s = (float)sqrt(delta / gamma);
        c = (float)(p / (gamma * (double)s * 2));
    } else {
        c = (float)sqrt((gamma + beta) / (gamma * 2));
        s = (float)(p / (gamma * (double)c * 2));
    }
    a = b = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float ai = At[I * 4 + k], aj = At[J * 4 + k];
        const float t0 = c * ai + s * aj, t1 = -s * ai + c * aj;
        At[I * 4 + k] = t0; At[J * 4 + k] = t1;
        a += (double)t0 * (double)t0; b += (double)t1 * (double)t1;
    }
    W[I] = a; W[J] = b;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float vi = Vt[I * 4 + k], vj = Vt[J * 4 + k];
        Vt[I * 4 + k] = c * vi + s * vj;
        Vt[J * 4 + k] = -s * vi + c * vj;
    }
    return true;
}

// last right singular vector of a 4x4 float matrix (row-major A), as cv::SVD::compute(...).vt.row(3)
__device__ inline void svd4_last_row(const float (&A)[16], float (&out)[4]) {
    float At[16], Vt[16];
    double W[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { At[i * 4 + k] = A[k * 4 + i]; sd += (double)At[i * 4 + k] * (double)At[i * 4 + k]; Vt[i * 4 + k] = (i == k) ? 1.f : 0.f; }
        W[i] = sd;
    }
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
        changed |= jacobi_pair<0, 1>(At, Vt, W);
        changed |= jacobi_pair<0, 2>(At, Vt, W);
        changed |= jacobi_pair<0, 3>(At, Vt, W);
        changed |= jacobi_pair<1, 2>(At, Vt, W);
        changed |= jacobi_pair<1, 3>(At, Vt, W);
        changed |= jacobi_pair<2, 3>(At, Vt, W);
        if (!changed) break;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) sd += (double)At[i * 4 + k] * (double)At[i * 4 + k];
        W[i] = sqrt(sd);
    }
    // selection sort by decreasing W (strict <), tracking only which original row ends up last
    int perm[4] = {0, 1, 2, 3};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        int j = i;
#pragma unroll
        for (int k = i + 1; k < 4; k++)
            if (W[j] < W[k]) j = k;
        if (j != i) {
            // static-index swap
#pragma unroll
            for (int k = i + 1; k < 4; k++)
                if (k == j) { const double tw = W[i]; W[i] = W[k]; W[k] = tw; const int tp = perm[i]; perm[i] = perm[k]; perm[k] = tp; }
        }
    }
    const int r = perm[3];
#pragma unroll
    for (int k = 0; k < 4; k++) out[k] = r == 0 ? Vt[k] : r == 1 ? Vt[4 + k] : r == 2 ? Vt[8 + k] : Vt[12 + k];
}

}  // namespace oslam
