// g2o::Sim3 on Eigen::Quaterniond for the kernels that optimise Sim3 vertices (sim3_opt.hip, essential_graph.hip): the constructor from a 7-vector (the
// exponential map), its inverse Sim3::log, the product, the inverse and VertexSim3Expmap::oplusImpl, restated from the published ORB_SLAM2 Thirdparty/g2o
// sources (sim3.h, types_seven_dof_expmap) in the way se3_math.h restates the SE3 ones.  Device code; product code, never includes oracle/.
#pragma once
#include <hip/hip_runtime.h>

#include "se3_math.h"

namespace oslam {

constexpr int kSim3PackN = 16;   // q[4] t[3] s of a Sim3 and of its inverse (pack_sim3)

struct Sim3 { double q[4], t[3], s; };   // g2o::Sim3: r (x y z w), t, s

__device__ __forceinline__ void quat_mul(const double a[4], const double b[4], double r[4]) {   // Eigen quaternion product
    const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
    r[3] = aw * bw - ax * bx - ay * by - az * bz;
    r[0] = aw * bx + ax * bw + ay * bz - az * by;
    r[1] = aw * by + ay * bw + az * bx - ax * bz;
    r[2] = aw * bz + az * bw + ax * by - ay * bx;
}

// Sim3(const Vector7d& update) of sim3.h: (omega, upsilon, sigma), four branches on |sigma| < eps and theta < eps
__device__ inline Sim3 sim3_exp(const double u[7]) {
    const double wx = u[0], wy = u[1], wz = u[2], sigma = u[6];
    const double theta = sqrt(wx * wx + wy * wy + wz * wz);
    const double W[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
    double W2[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) W2[i * 3 + j] = W[i * 3] * W[j] + W[i * 3 + 1] * W[3 + j] + W[i * 3 + 2] * W[6 + j];
    Sim3 S;
    S.s = exp(sigma);
    const double eps = 0.00001;
    double A, B, C, ra, rb;   // R = I + ra Omega + rb Omega^2
    const bool small_theta = theta < eps;
    if (small_theta) { ra = 1.0; rb = 1.0; }
    else { ra = sin(theta) / theta; rb = (1 - cos(theta)) / (theta * theta); }
    if (fabs(sigma) < eps) {
        C = 1;
        if (small_theta) { A = 1. / 2.; B = 1. / 6.; }
        else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        const double sigma2 = sigma * sigma;
        if (small_theta) {
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);   // as published (the series of this branch would subtract 1 from the numerator)
        } else {
            const double a = S.s * sin(theta), b = S.s * cos(theta);
            const double theta2 = theta * theta;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    double R[9], V[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const double I = (i % 4) == 0 ? 1.0 : 0.0;
        R[i] = small_theta ? (I + W[i]) + W2[i] : (I + ra * W[i]) + rb * W2[i];
        V[i] = (A * W[i] + B * W2[i]) + C * I;
    }
    quat_from_R(R, S.q);
#pragma unroll
    for (int i = 0; i < 3; i++) S.t[i] = V[i * 3] * u[3] + V[i * 3 + 1] * u[4] + V[i * 3 + 2] * u[5];
    return S;
}

__device__ __forceinline__ Sim3 sim3_mul(const Sim3& a, const Sim3& b) {   // Sim3::operator*
    Sim3 r;
    quat_mul(a.q, b.q, r.q);
    double rt[3];
    quat_rot(a.q, b.t, rt);
#pragma unroll
    for (int i = 0; i < 3; i++) r.t[i] = a.s * rt[i] + a.t[i];
    r.s = a.s * b.s;
    return r;
}

__device__ __forceinline__ Sim3 sim3_inv(const Sim3& a) {   // Sim3::inverse
    Sim3 r;
    r.q[0] = -a.q[0]; r.q[1] = -a.q[1]; r.q[2] = -a.q[2]; r.q[3] = a.q[3];
    const double m = -1. / a.s;
    const double v[3] = {m * a.t[0], m * a.t[1], m * a.t[2]};
    quat_rot(r.q, v, r.t);
    r.s = 1. / a.s;
    return r;
}

// VertexSim3Expmap::oplusImpl
__device__ __forceinline__ Sim3 sim3_oplus(const Sim3& S, const double x[7], bool fix_scale) {
    double u[7];
#pragma unroll
    for (int i = 0; i < 7; i++) u[i] = x[i];
    if (fix_scale) u[6] = 0;
    return sim3_mul(sim3_exp(u), S);
}

__device__ __forceinline__ void pack_sim3(const Sim3& S, double* p) {
    const Sim3 Si = sim3_inv(S);
#pragma unroll
    for (int k = 0; k < 4; k++) { p[k] = S.q[k]; p[8 + k] = Si.q[k]; }
#pragma unroll
    for (int k = 0; k < 3; k++) { p[4 + k] = S.t[k]; p[12 + k] = Si.t[k]; }
    p[7] = S.s; p[15] = Si.s;
}

// Sim3::log of sim3.h: (omega, upsilon, sigma).  Four branches on |sigma| < eps and d > 1 - eps with d = (tr R - 1) / 2, R = r.toRotationMatrix();
// omega = 0.5 deltaR(R) or theta / (2 sqrt(1 - d^2)) deltaR(R) with theta = acos(d); A, B, C as in the constructor (the published B of the |sigma| >= eps,
// small-angle branch included); upsilon = (A Omega + B Omega^2 + C I)^-1 t.  Eigen's W.lu().solve(t) is a PartialPivLU: here Gaussian elimination of the
// 3 x 3 system with row pivoting on the largest magnitude (the first of equal ones), then back substitution.
__device__ inline void sim3_log(const Sim3& S, double u[7]) {
    const double sigma = log(S.s);
    SE3 qq;
#pragma unroll
    for (int k = 0; k < 4; k++) qq.q[k] = S.q[k];
    double R[9];
    se3_R(qq, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};   // deltaR
    const double eps = 0.00001;
    double om[3], A, B, C;
    if (fabs(sigma) < eps) {
        C = 1;
        if (d > 1 - eps) {
#pragma unroll
            for (int k = 0; k < 3; k++) om[k] = 0.5 * dR[k];
            A = 1. / 2.; B = 1. / 6.;
        } else {
            const double theta = acos(d), theta2 = theta * theta;
            const double f = theta / (2 * sqrt(1 - d * d));
#pragma unroll
            for (int k = 0; k < 3; k++) om[k] = f * dR[k];
            A = (1 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        if (d > 1 - eps) {
            const double sigma2 = sigma * sigma;
#pragma unroll
            for (int k = 0; k < 3; k++) om[k] = 0.5 * dR[k];
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);   // as published
        } else {
            const double theta = acos(d);
            const double f = theta / (2 * sqrt(1 - d * d));
#pragma unroll
            for (int k = 0; k < 3; k++) om[k] = f * dR[k];
            const double theta2 = theta * theta;
            const double a = S.s * sin(theta), b = S.s * cos(theta);
            const double c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    const double O[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
    double m0[4], m1[4], m2[4];   // the rows of [W | t], W = A Omega + B Omega^2 + C I
#pragma unroll
    for (int j = 0; j < 3; j++) {
        m0[j] = (A * O[j] + B * (O[0] * O[j] + O[1] * O[3 + j] + O[2] * O[6 + j])) + (j == 0 ? C : 0.0);
        m1[j] = (A * O[3 + j] + B * (O[3] * O[j] + O[4] * O[3 + j] + O[5] * O[6 + j])) + (j == 1 ? C : 0.0);
        m2[j] = (A * O[6 + j] + B * (O[6] * O[j] + O[7] * O[3 + j] + O[8] * O[6 + j])) + (j == 2 ? C : 0.0);
    }
    m0[3] = S.t[0]; m1[3] = S.t[1]; m2[3] = S.t[2];
    auto swap_rows = [](double (&a)[4], double (&b)[4]) {
#pragma unroll
        for (int k = 0; k < 4; k++) { const double t = a[k]; a[k] = b[k]; b[k] = t; }
    };
    if (fabs(m1[0]) > fabs(m0[0])) swap_rows(m0, m1);
    if (fabs(m2[0]) > fabs(m0[0])) swap_rows(m0, m2);
    {
        const double f1 = m1[0] / m0[0], f2 = m2[0] / m0[0];
#pragma unroll
        for (int k = 1; k < 4; k++) { m1[k] -= f1 * m0[k]; m2[k] -= f2 * m0[k]; }
    }
    if (fabs(m2[1]) > fabs(m1[1])) swap_rows(m1, m2);
    {
        const double f2 = m2[1] / m1[1];
#pragma unroll
        for (int k = 2; k < 4; k++) m2[k] -= f2 * m1[k];
    }
    const double u2 = m2[3] / m2[2];
    const double u1 = (m1[3] - m1[2] * u2) / m1[1];
    const double u0 = (m0[3] - m0[1] * u1 - m0[2] * u2) / m0[0];
    u[0] = om[0]; u[1] = om[1]; u[2] = om[2];
    u[3] = u0; u[4] = u1; u[5] = u2;
    u[6] = sigma;
}

}  // namespace oslam
