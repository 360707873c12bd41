// sim3_opt.hip — Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1046-1241) for batches of independent problems on gfx950 (include/oslam_hip.h,
// "OptimizeSim3").  One launch, one 64-lane wavefront per problem: both optimize() calls and both chi2 passes run inside the kernel.  The lanes stride over
// the correspondences; each evaluates both edges' errors at the estimate and at the fourteen perturbed estimates of the numeric Jacobian (which lanes
// 0-13 prepare once per linearisation and share through LDS), the 28 + 7 + 1 sums go through the vector-ALU butterfly of lane_ops.h, and every lane then
// runs the 7 x 7 LDLT, the exponential map and the Levenberg-Marquardt bookkeeping on the same numbers.  No atomics, no inter-wavefront traffic: a
// problem's result does not depend on what else is in the batch.  An edge's stored _error is a function of the estimate it was last evaluated at, so the
// "stale error" of a rejected last trial is kept as that trial's Sim3 (eight doubles), not per edge; the dropped flags live in the problem's own bytes
// of `inliers`.  The g2o Sim3 pieces are restated from the published ORB_SLAM2 Thirdparty/g2o sources.  Product code; never includes oracle/.
#include <cmath>
#include <mutex>

#include "common.h"
#include "lane_ops.h"
#include "se3_math.h"
#include "sim3_math.h"
#include "stage_layout.h"

using oslam::set_error;
using oslam::Sim3; using oslam::pack_sim3; using oslam::sim3_exp; using oslam::sim3_inv; using oslam::sim3_mul; using oslam::sim3_oplus;

struct oslam_sim3_opt {
    int device = 0, max_problems = 0, max_corr = 0;
    oslam::StagePair io;   // staging of the host-pointer entry point: inputs | outputs
    std::mutex mu;
};

namespace {

constexpr int kLanes = 64;
constexpr int kTraceRows = OSLAM_SIM3_OPT_TRACE_ROWS;
constexpr int kPert = 14;      // +delta, -delta for each of the 7 dimensions of VertexSim3Expmap
constexpr int kPertN = oslam::kSim3PackN;
constexpr double kDBL_MAX = 1.7976931348623157e308;

struct Sim3OptArgs {
    const oslam_sim3_opt_problem_t* problems;
    int n_problems, n_corr;
    const float *X1, *X2, *obs1, *obs2, *inv1, *inv2;
    double* S12; uint8_t* inliers; int32_t* status;
    double* trace; int32_t* trace_n;
};

// obs - cam_map(project(S.map(P))): EdgeSim3ProjectXYZ with (S12, P3D2c, camera 1), EdgeInverseSim3ProjectXYZ with (S12.inverse(), P3D1c, camera 2)
__device__ __forceinline__ void edge_error(const double q[4], const double t[3], double s, const double P[3], double fx, double fy, double cx, double cy, const double obs[2],
                                           double e[2]) {
    double r[3];
    oslam::quat_rot(q, P, r);
    const double x = s * r[0] + t[0], y = s * r[1] + t[1], z = s * r[2] + t[2];
    e[0] = obs[0] - ((x / z) * fx + cx);
    e[1] = obs[1] - ((y / z) * fy + cy);
}

struct Edge {   // one correspondence: both edges' fixed points, measurements and information
    double P1[3], P2[3], o1[2], o2[2], i1, i2;
};

struct Camera2 { double fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2; };

// both errors at (S, Si): e[0..1] = e12, e[2..3] = e21
__device__ __forceinline__ void errors_at(const double* S, const Edge& E, const Camera2& K, double e[4]) {
    edge_error(S, S + 4, S[7], E.P2, K.fx1, K.fy1, K.cx1, K.cy1, E.o1, e);
    edge_error(S + 8, S + 12, S[15], E.P1, K.fx2, K.fy2, K.cx2, K.cy2, E.o2, e + 2);
}

__device__ __forceinline__ void huber(double e2, double delta, double& rho0, double& rho1) {   // RobustKernelHuber::robustify
    const double dsqr = delta * delta;
    if (e2 <= dsqr) { rho0 = e2; rho1 = 1.; }
    else {
        const double sqrte = sqrt(e2);
        rho0 = 2 * sqrte * delta - dsqr;
        rho1 = delta / sqrte;
    }
}

// (H + lambda I) x = b by an unpivoted LDL^T; false when a pivot is not positive and finite (LinearSolverDense: !isPositive)
__device__ bool solve7(const double (&H)[28], const double (&b)[7], double lambda, double (&x)[7]) {
    double L[7][7], d[7];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 7; j++) {
        double dj = H[j * (15 - j) / 2] + lambda;   // (index of (j, j) in the packed upper triangle)
#pragma unroll
        for (int k = 0; k < j; k++) dj -= (L[j][k] * L[j][k]) * d[k];
        ok = ok && dj > 0 && (dj - dj) == 0;
        d[j] = dj;
#pragma unroll
        for (int i = j + 1; i < 7; i++) {
            double s = H[j * (15 - j) / 2 + (i - j)];
#pragma unroll
            for (int k = 0; k < j; k++) s -= (L[i][k] * L[j][k]) * d[k];
            L[i][j] = s / dj;
        }
    }
    double y[7];
#pragma unroll
    for (int i = 0; i < 7; i++) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) s -= L[i][k] * y[k];
        y[i] = s;
    }
#pragma unroll
    for (int i = 6; i >= 0; i--) {
        double s = y[i] / d[i];
#pragma unroll
        for (int k = i + 1; k < 7; k++) s -= L[k][i] * x[k];
        x[i] = s;
    }
    return ok;
}

struct Problem {
    int count; size_t off;
    Camera2 K;
    double delta, th2;
    bool fix_scale;
};

__device__ __forceinline__ Edge load_edge(const Sim3OptArgs& a, size_t o) {
    Edge E;
#pragma unroll
    for (int k = 0; k < 3; k++) { E.P1[k] = (double)a.X1[3 * o + k]; E.P2[k] = (double)a.X2[3 * o + k]; }
#pragma unroll
    for (int k = 0; k < 2; k++) { E.o1[k] = (double)a.obs1[2 * o + k]; E.o2[k] = (double)a.obs2[2 * o + k]; }
    E.i1 = (double)a.inv1[o]; E.i2 = (double)a.inv2[o];
    return E;
}

// activeRobustChi2 after computeActiveErrors at S: the sum of rho[0] over the live edges
__device__ double robust_chi2(const Sim3OptArgs& a, const Problem& P, const Sim3& S) {
    const int lane = threadIdx.x;
    double Sp[kPertN];
    pack_sim3(S, Sp);
    double acc = 0;
    for (int base = 0; base < P.count; base += kLanes) {
        const int i = base + lane;
        if (i < P.count && a.inliers[P.off + i]) {
            const Edge E = load_edge(a, P.off + i);
            double e[4], r0, r1;
            errors_at(Sp, E, P.K, e);
            huber((e[0] * E.i1) * e[0] + (e[1] * E.i1) * e[1], P.delta, r0, r1);
            acc += r0;
            huber((e[2] * E.i2) * e[2] + (e[3] * E.i2) * e[3], P.delta, r0, r1);
            acc += r0;
        }
    }
    return oslam::wave_sum_xor(acc);
}

// `chi2() > th2` of both edges with the errors the last trial left (:1186-1203, :1220-1234): clears the entries, returns how many live pairs failed
__device__ int chi2_pass(const Sim3OptArgs& a, const Problem& P, const Sim3& S_last, int& n_kept) {
    const int lane = threadIdx.x;
    double Sp[kPertN];
    pack_sim3(S_last, Sp);
    int bad = 0, kept = 0;
    for (int base = 0; base < P.count; base += kLanes) {
        const int i = base + lane;
        bool live = false, out = false;
        if (i < P.count && a.inliers[P.off + i]) {
            live = true;
            const Edge E = load_edge(a, P.off + i);
            double e[4];
            errors_at(Sp, E, P.K, e);
            const double c12 = (e[0] * E.i1) * e[0] + (e[1] * E.i1) * e[1], c21 = (e[2] * E.i2) * e[2] + (e[3] * E.i2) * e[3];
            out = c12 > P.th2 || c21 > P.th2;
            if (out) a.inliers[P.off + i] = 0;
        }
        bad += __popcll(__ballot(live && out));
        kept += __popcll(__ballot(live && !out));
    }
    n_kept = kept;
    return bad;
}

// SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg over BlockSolverX / LinearSolverDense.  S: the estimate, S_last: the
// estimate of the last trial (accepted or not), which the edges' _error belongs to afterwards.
__device__ void optimize(const Sim3OptArgs& a, const Problem& P, int iterations, Sim3& S, Sim3& S_last, double* s_pert, int& n_its, int& n_trials, double* trace) {
    const int lane = threadIdx.x;
    const double delta = 1e-9, scalar = 1.0 / (2 * delta);   // BaseBinaryEdge::linearizeOplus: the column is scalar * (e+ - e-)
    double lambda = 0, ni = 2;
    for (int it = 0; it < iterations; it++) {
        // the fourteen perturbed estimates (push, oplus(+-delta e_d), pop), one per lane 0-13, and their inverses
        __syncthreads();
        {
            const int p = lane % kPert, dim = p >> 1;
            double u[7];
#pragma unroll
            for (int k = 0; k < 7; k++) u[k] = k == dim ? ((p & 1) ? -delta : delta) : 0.0;
            const Sim3 Sd = sim3_oplus(S, u, P.fix_scale);
            double pk[kPertN];
            pack_sim3(Sd, pk);
            if (lane < kPert)
#pragma unroll
                for (int k = 0; k < kPertN; k++) s_pert[p * kPertN + k] = pk[k];
        }
        __syncthreads();
        double Sp[kPertN];
        pack_sim3(S, Sp);
        // computeActiveErrors, activeRobustChi2, buildSystem: acc = upper triangle of H (28) | b (7) | F
        double acc[36];
#pragma unroll
        for (int k = 0; k < 36; k++) acc[k] = 0;
        for (int base = 0; base < P.count; base += kLanes) {
            const int i = base + lane;
            if (i < P.count && a.inliers[P.off + i]) {
                const Edge E = load_edge(a, P.off + i);
#pragma unroll 1
                for (int g = 0; g < 2; g++) {   // e12 (S12, X3Dc2, camera 1), then e21 (S12.inverse(), X3Dc1, camera 2)
                    const int so = 8 * g;
                    const double* X = g ? E.P1 : E.P2;
                    const double* ob = g ? E.o2 : E.o1;
                    const double fx = g ? P.K.fx2 : P.K.fx1, fy = g ? P.K.fy2 : P.K.fy1, cx = g ? P.K.cx2 : P.K.cx1, cy = g ? P.K.cy2 : P.K.cy1;
                    const double info = g ? E.i2 : E.i1;
                    double e[2], J[2][7];
                    edge_error(Sp + so, Sp + so + 4, Sp[so + 7], X, fx, fy, cx, cy, ob, e);
#pragma unroll
                    for (int d = 0; d < 7; d++) {
                        const double* pp = s_pert + (2 * d) * kPertN + so;
                        const double* pm = pp + kPertN;
                        double ep[2], em[2];
                        edge_error(pp, pp + 4, pp[7], X, fx, fy, cx, cy, ob, ep);
                        edge_error(pm, pm + 4, pm[7], X, fx, fy, cx, cy, ob, em);
                        J[0][d] = scalar * (ep[0] - em[0]);
                        J[1][d] = scalar * (ep[1] - em[1]);
                    }
                    double r0, r1;
                    huber((e[0] * info) * e[0] + (e[1] * info) * e[1], P.delta, r0, r1);
                    acc[35] += r0;
                    const double w = r1 * info;                                           // robustInformation
                    const double or0 = (-(info * e[0])) * r1, or1 = (-(info * e[1])) * r1;   // omega_r = -information * error, times rho[1]
                    int idx = 0;
#pragma unroll
                    for (int r = 0; r < 7; r++) {
                        const double j0w = J[0][r] * w, j1w = J[1][r] * w;
#pragma unroll
                        for (int c = r; c < 7; c++) { acc[idx] += j0w * J[0][c] + j1w * J[1][c]; idx++; }
                        acc[28 + r] += J[0][r] * or0 + J[1][r] * or1;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 36; k++) acc[k] = oslam::wave_sum_xor(acc[k]);
        double H[28], b[7];
#pragma unroll
        for (int k = 0; k < 28; k++) H[k] = acc[k];
#pragma unroll
        for (int k = 0; k < 7; k++) b[k] = acc[28 + k];
        double currentChi = acc[35];
        if (it == 0) {   // computeLambdaInit: 1e-5 * max |H_jj|
            double md = 0;
#pragma unroll
            for (int j = 0; j < 7; j++) md = fmax(fabs(H[j * (15 - j) / 2]), md);
            lambda = 1e-5 * md;
            ni = 2;
        }
        double rho = 0;
        int qmax = 0;
        do {
            double x[7];
            const bool ok2 = solve7(H, b, lambda, x);
            if (!ok2)
#pragma unroll
                for (int k = 0; k < 7; k++) x[k] = 0;
            const Sim3 Sn = sim3_oplus(S, x, P.fix_scale);
            double tempChi = robust_chi2(a, P, Sn);
            S_last = Sn;
            if (!ok2) tempChi = kDBL_MAX;
            rho = currentChi - tempChi;
            double scale = 0;   // computeScale
#pragma unroll
            for (int k = 0; k < 7; k++) scale += x[k] * (lambda * x[k] + b[k]);
            scale += 1e-3;
            rho /= scale;
            const bool accepted = rho > 0 && (tempChi - tempChi) == 0;
            if (trace && lane == 0 && n_trials < kTraceRows) {
                double* t = trace + 6 * n_trials;
                t[0] = currentChi; t[1] = tempChi; t[2] = rho; t[3] = lambda; t[4] = accepted ? 1.0 : 0.0; t[5] = (it == 0 && qmax == 0) ? 1.0 : 0.0;
            }
            if (accepted) {
                double alpha = 1. - (2 * rho - 1) * (2 * rho - 1) * (2 * rho - 1);
                alpha = fmin(alpha, 2. / 3.);
                lambda *= fmax(1. / 3., alpha);
                ni = 2;
                currentChi = tempChi;
                S = Sn;
            } else {
                lambda *= ni;
                ni *= 2;
            }
            qmax++;
            n_trials++;
        } while (rho < 0 && qmax < 10);
        n_its++;
        if (qmax == 10 || rho == 0) break;   // OptimizationAlgorithm::Terminate
    }
}

__device__ __forceinline__ bool finite_f(float v) { return (v - v) == 0.0f; }

__global__ __launch_bounds__(kLanes) void k_optimize_sim3(Sim3OptArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const oslam_sim3_opt_problem_t& R = a.problems[b];
    int32_t* status = a.status + 4 * (size_t)b;
    const int count = R.count, offset = R.offset;
    // a record that does not lie inside the arrays: -2, nothing else is written (the host-pointer entry point refuses the call instead)
    if (count < 0 || offset < 0 || offset > a.n_corr - count) {
        if (lane == 0) status[0] = -2;
        return;
    }
    __shared__ double s_pert[kPert * kPertN];
    Problem P;
    P.count = count; P.off = (size_t)offset;
    P.K.fx1 = (double)R.fx1; P.K.fy1 = (double)R.fy1; P.K.cx1 = (double)R.cx1; P.K.cy1 = (double)R.cy1;
    P.K.fx2 = (double)R.fx2; P.K.fy2 = (double)R.fy2; P.K.cx2 = (double)R.cx2; P.K.cy2 = (double)R.cy2;
    P.delta = (double)sqrtf(R.th2);   // const float deltaHuber = sqrt(th2) (:1095)
    P.th2 = (double)R.th2;
    P.fix_scale = R.fix_scale != 0;
    if (a.trace_n && lane == 0) a.trace_n[b] = 0;

    bool ok = finite_f(R.fx1) && finite_f(R.fy1) && finite_f(R.cx1) && finite_f(R.cy1) && finite_f(R.fx2) && finite_f(R.fy2) && finite_f(R.cx2) && finite_f(R.cy2) &&
              finite_f(R.s12) && R.s12 > 0.0f && finite_f(R.th2);
#pragma unroll
    for (int k = 0; k < 9; k++) ok = ok && finite_f(R.R12[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) ok = ok && finite_f(R.t12[k]);
    for (int i = lane; i < count; i += kLanes) {
        const size_t o = P.off + i;
        bool f = finite_f(a.inv1[o]) && finite_f(a.inv2[o]);
#pragma unroll
        for (int k = 0; k < 3; k++) f = f && finite_f(a.X1[3 * o + k]) && finite_f(a.X2[3 * o + k]);
#pragma unroll
        for (int k = 0; k < 2; k++) f = f && finite_f(a.obs1[2 * o + k]) && finite_f(a.obs2[2 * o + k]);
        ok = ok && f;
    }
    ok = __all(ok);   // (lanes that left the loop early are active again here)
    for (int i = lane; i < count; i += kLanes) a.inliers[P.off + i] = ok ? 1 : 0;
    if (!ok) {
        if (lane == 0) { status[0] = -1; status[1] = count; status[2] = 0; status[3] = 0; }
        return;
    }
    if (count == 0) {
        if (lane == 0) { status[0] = 0; status[1] = 0; status[2] = 0; status[3] = 0; }
        return;
    }

    // g2o::Sim3 gScm(Converter::toMatrix3d(R), Converter::toVector3d(t), s) (src/LoopClosing.cc:326)
    Sim3 S, S_last;
    {
        double Rd[9];
#pragma unroll
        for (int k = 0; k < 9; k++) Rd[k] = (double)R.R12[k];
        oslam::quat_from_R(Rd, S.q);
#pragma unroll
        for (int k = 0; k < 3; k++) S.t[k] = (double)R.t12[k];
        S.s = (double)R.s12;
    }
    S_last = S;
    double* trace = a.trace ? a.trace + (size_t)b * kTraceRows * 6 : nullptr;
    int n_its = 0, n_trials = 0, kept = 0;
    optimize(a, P, 5, S, S_last, s_pert, n_its, n_trials, trace);
    const int nBad = chi2_pass(a, P, S_last, kept);
    int ret = 0;
    bool write = false;
    if (count - nBad >= 10) {
        optimize(a, P, nBad > 0 ? 10 : 5, S, S_last, s_pert, n_its, n_trials, trace);
        chi2_pass(a, P, S_last, kept);
        ret = kept;
        write = true;
    }
    if (lane == 0) {
        if (write) {
            double* o = a.S12 + 13 * (size_t)b;
            oslam::SE3 q;
#pragma unroll
            for (int k = 0; k < 4; k++) q.q[k] = S.q[k];
            double Rm[9];
            oslam::se3_R(q, Rm);
#pragma unroll
            for (int k = 0; k < 9; k++) o[k] = Rm[k];
#pragma unroll
            for (int k = 0; k < 3; k++) o[9 + k] = S.t[k];
            o[12] = S.s;
        }
        status[0] = ret; status[1] = count; status[2] = nBad; status[3] = n_its * 256 + n_trials;
        if (a.trace_n) a.trace_n[b] = n_trials;
    }
}

int check_call(const char* fn, const oslam_sim3_opt* h, int n_problems, int n_corr) {
    if (!h) { set_error("%s: NULL handle", fn); return OSLAM_E_INVALID; }
    if (n_problems < 0 || n_corr < 0) { set_error("%s: %d problems, %d correspondences: neither may be negative", fn, n_problems, n_corr); return OSLAM_E_CAPACITY; }
    if (n_problems > h->max_problems) { set_error("%s: %d problems exceed the handle's %d", fn, n_problems, h->max_problems); return OSLAM_E_CAPACITY; }
    if (n_corr > h->max_corr) { set_error("%s: %d correspondences exceed the handle's %d", fn, n_corr, h->max_corr); return OSLAM_E_CAPACITY; }
    return OSLAM_OK;
}

}  // namespace

extern "C" {

void oslam_sim3_opt_destroy(oslam_sim3_opt_t* h) {
    if (!h) return;
    delete h;
}

int oslam_sim3_opt_create(oslam_sim3_opt_t** out, int max_problems, int max_correspondences_total, int device) {
    if (!out) { set_error("oslam_sim3_opt_create: out is NULL"); return OSLAM_E_INVALID; }
    *out = nullptr;
    if (max_problems < 1 || max_correspondences_total < 1) { set_error("oslam_sim3_opt_create: bad argument"); return OSLAM_E_INVALID; }
    const int ndev = oslam_device_count();
    if (ndev <= 0) return oslam::no_device("oslam_sim3_opt_create");
    if (device < 0 || device >= ndev) { set_error("oslam_sim3_opt_create: device out of range"); return OSLAM_E_INVALID; }
    oslam_sim3_opt* h = new oslam_sim3_opt;
    h->device = device; h->max_problems = max_problems; h->max_corr = max_correspondences_total;
    *out = h;
    return OSLAM_OK;
}

int oslam_optimize_sim3_batch_device(oslam_sim3_opt_t* h, int n_problems, const oslam_sim3_opt_problem_t* d_problems, int n_corr, const float* d_X3Dc1, const float* d_X3Dc2,
                                     const float* d_obs1, const float* d_obs2, const float* d_invSigma2_1, const float* d_invSigma2_2, double* d_S12, uint8_t* d_inliers,
                                     int32_t* d_status, double* d_trace, int32_t* d_trace_n, void* stream) {
    const char* fn = "oslam_optimize_sim3_batch_device";
    OSLAM_CHECK(check_call(fn, h, n_problems, n_corr));
    if (n_problems == 0) return OSLAM_OK;
    if (!d_problems || !d_S12 || !d_status || (n_corr > 0 && (!d_X3Dc1 || !d_X3Dc2 || !d_obs1 || !d_obs2 || !d_invSigma2_1 || !d_invSigma2_2 || !d_inliers)) ||
        (d_trace && !d_trace_n)) {
        set_error("%s: NULL argument", fn);
        return OSLAM_E_INVALID;
    }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    Sim3OptArgs a;
    a.problems = d_problems; a.n_problems = n_problems; a.n_corr = n_corr;
    a.X1 = d_X3Dc1; a.X2 = d_X3Dc2; a.obs1 = d_obs1; a.obs2 = d_obs2; a.inv1 = d_invSigma2_1; a.inv2 = d_invSigma2_2;
    a.S12 = d_S12; a.inliers = d_inliers; a.status = d_status; a.trace = d_trace; a.trace_n = d_trace_n;
    hipLaunchKernelGGL(k_optimize_sim3, dim3(n_problems), dim3(kLanes), 0, (hipStream_t)stream, a);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int oslam_optimize_sim3_batch(oslam_sim3_opt_t* h, int n_problems, const oslam_sim3_opt_problem_t* problems, int n_corr, const float* X3Dc1, const float* X3Dc2, const float* obs1,
                              const float* obs2, const float* invSigma2_1, const float* invSigma2_2, double* S12, uint8_t* inliers, int32_t* status, double* trace,
                              int32_t* trace_n) {
    const char* fn = "oslam_optimize_sim3_batch";
    OSLAM_CHECK(check_call(fn, h, n_problems, n_corr));
    if (n_problems == 0) return OSLAM_OK;
    if (!problems || !S12 || !status || (n_corr > 0 && (!X3Dc1 || !X3Dc2 || !obs1 || !obs2 || !invSigma2_1 || !invSigma2_2 || !inliers)) || (trace && !trace_n)) {
        set_error("%s: NULL argument", fn);
        return OSLAM_E_INVALID;
    }
    for (int b = 0; b < n_problems; b++) {
        const oslam_sim3_opt_problem_t& P = problems[b];
        if (P.count < 0 || P.offset < 0 || P.offset > n_corr - P.count) {
            set_error("%s: problem %d (count %d at offset %d) lies outside the %d correspondences", fn, b, P.count, P.offset, n_corr);
            return OSLAM_E_INVALID;
        }
    }
    std::lock_guard<std::mutex> lock(h->mu);
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t np = (size_t)n_problems, M = (size_t)n_corr;
    oslam::StageLayout lay;   // one block, inputs then outputs: one upload, one download
    const auto fPr = lay.add<oslam_sim3_opt_problem_t>(np);
    const auto fX1 = lay.add<float>(M * 3), fX2 = lay.add<float>(M * 3), fO1 = lay.add<float>(M * 2), fO2 = lay.add<float>(M * 2), fI1 = lay.add<float>(M), fI2 = lay.add<float>(M);
    const auto fS = lay.add<double>(np * 13);
    const auto fIn = lay.add<uint8_t>(M);
    const auto fSt = lay.add<int32_t>(np * 4), fTn = lay.add<int32_t>(np);   // (trace_n has its room with or without a trace)
    const auto fTr = lay.add<double>(np * kTraceRows * 6, trace != nullptr);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fPr, ph, problems); put(fX1, ph, X3Dc1); put(fX2, ph, X3Dc2); put(fO1, ph, obs1); put(fO2, ph, obs2); put(fI1, ph, invSigma2_1); put(fI2, ph, invSigma2_2);
    // the caller's output bytes travel too: what no problem owns, or the kernel leaves alone, comes back as it was
    put(fS, ph, S12); put(fIn, ph, inliers); put(fSt, ph, status);
    if (trace) { put(fTn, ph, trace_n); put(fTr, ph, trace); }
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, nullptr));
    OSLAM_CHECK(oslam_optimize_sim3_batch_device(h, n_problems, at(fPr, pd), n_corr, at(fX1, pd), at(fX2, pd), at(fO1, pd), at(fO2, pd), at(fI1, pd), at(fI2, pd), at(fS, pd),
                                                 at(fIn, pd), at(fSt, pd), at(fTr, pd), trace ? at(fTn, pd) : nullptr, nullptr));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fS.off, pd + fS.off, lay.total() - fS.off, hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(fS, ph, S12); get(fIn, ph, inliers); get(fSt, ph, status);
    if (trace) { get(fTn, ph, trace_n); get(fTr, ph, trace); }
    return OSLAM_OK;
}

}  // extern "C"
