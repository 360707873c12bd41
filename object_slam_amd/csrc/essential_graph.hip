// essential_graph.hip — Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:781-1044) for batches of independent pose graphs on gfx950
// (include/oslam_hip.h, "OptimizeEssentialGraph").  One launch, one workgroup of 256 lanes per graph: the measurements, the twenty Levenberg-Marquardt
// iterations, every refactorisation and the SE3 recovery run inside the kernel.  H = sum J^T J is stored as a block envelope (per free vertex, the
// 7 x 7 blocks from its first connected column to the diagonal) in a global-memory workspace of the handle, and H + lambda I is factored in place by a
// right-looking block Cholesky over the envelope: per block column the diagonal block is factored (every lane, in registers), the blocks below it are
// solved (one lane per scalar row, which also carries the forward substitution of b), and the trailing blocks are updated (one lane per entry).  Nothing
// is summed with atomics: an entry of H, b or L has one owner lane per step, the steps run in column order, and F goes through a fixed butterfly.  The
// g2o pieces are restated from the published ORB_SLAM2 Thirdparty/g2o sources (sim3_math.h).  Product code; never includes oracle/.
#include <cmath>
#include <mutex>
#include <vector>

#include "common.h"
#include "lane_ops.h"
#include "se3_math.h"
#include "sim3_math.h"
#include "stage_layout.h"

using oslam::set_error;
using oslam::Sim3;

struct oslam_essential_graph {
    int device = 0, max_problems = 0, max_kf = 0, max_edges = 0;
    long long max_blocks = 0;
    oslam::DeviceBuffer ws;   // the factor, H and the per-keyframe / per-edge working arrays
    oslam::StagePair io;      // staging of the host-pointer entry points
    std::mutex mu;
};

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTraceRows = OSLAM_ESSENTIAL_GRAPH_TRACE_ROWS;
constexpr int kEdgeJ = 105;   // per edge: J of vertex 0 (7 x 7 row-major), J of vertex 1, the error (7)
constexpr double kDBL_MAX = 1.7976931348623157e308;

struct Workspace {   // device pointers into oslam_essential_graph::ws
    double *S_cur, *S_try;         // [max_kf][8] q t s
    double *b, *bw, *y, *x;        // [max_kf][7], indexed by kf_offset + free index
    double *Ld;                    // [max_kf][28] the factored diagonal blocks (lower triangle, row-major packed)
    double *C, *JE, *chi;          // [max_edges][8], [max_edges][105], [max_edges]
    double *H, *L;                 // [max_blocks][49]
    int32_t *fidx, *kfof, *ffirst, *rowstart, *colstart, *colcnt, *incstart, *inccnt;   // [max_kf]
    int32_t *inc;                  // [2 max_edges]
    int32_t *collist;              // [max_blocks]
};

struct EGArgs {
    const oslam_essential_graph_problem_t* problems;
    int n_problems, n_kf_total, n_edges_total;
    long long max_blocks;
    const float *Scw, *Snc;
    const uint8_t *has_nc, *fixed;
    const int32_t *edges, *row_first;
    double* Scw_out; float* Tcw_out; int32_t* status; double* trace; int32_t* trace_n;
    Workspace w;
};

__device__ __forceinline__ bool finite_f(float v) { return (v - v) == 0.0f; }

__device__ __forceinline__ Sim3 load_sim3(const double* p) {
    Sim3 S;
#pragma unroll
    for (int k = 0; k < 4; k++) S.q[k] = p[k];
#pragma unroll
    for (int k = 0; k < 3; k++) S.t[k] = p[4 + k];
    S.s = p[7];
    return S;
}
__device__ __forceinline__ void store_sim3(const Sim3& S, double* p) {
#pragma unroll
    for (int k = 0; k < 4; k++) p[k] = S.q[k];
#pragma unroll
    for (int k = 0; k < 3; k++) p[4 + k] = S.t[k];
    p[7] = S.s;
}
// g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s) of the 13 floats s, R[9], t[3]
__device__ __forceinline__ Sim3 sim3_from_floats(const float* p) {
    Sim3 S;
    double Rd[9];
#pragma unroll
    for (int k = 0; k < 9; k++) Rd[k] = (double)p[1 + k];
    oslam::quat_from_R(Rd, S.q);
#pragma unroll
    for (int k = 0; k < 3; k++) S.t[k] = (double)p[10 + k];
    S.s = (double)p[0];
    return S;
}

// EdgeSim3::computeError: (C * v0 * v1.inverse()).log()
__device__ __forceinline__ void edge_error(const Sim3& C, const Sim3& Si, const Sim3& Sj, double e[7]) {
    oslam::sim3_log(oslam::sim3_mul(oslam::sim3_mul(C, Si), oslam::sim3_inv(Sj)), e);
}

// The sum of v over the workgroup in a fixed order: the xor butterfly inside each wavefront, then the wavefronts' sums from 0 upwards.  Every lane gets it.
__device__ __forceinline__ double block_sum(double v, double* s_red) {
    v = oslam::wave_sum_xor(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = s_red[0];
#pragma unroll
    for (int k = 1; k < kWaves; k++) r += s_red[k];
    return r;
}

// Cholesky of a 7 x 7 block given by its lower triangle (packed by rows: (r, c) at r (r + 1) / 2 + c), in registers; false on a pivot that is not
// positive and finite
__device__ __forceinline__ bool chol7(double (&A)[28]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 7; j++) {
        double d = A[j * (j + 1) / 2 + j];
#pragma unroll
        for (int k = 0; k < j; k++) d -= A[j * (j + 1) / 2 + k] * A[j * (j + 1) / 2 + k];
        ok = ok && d > 0 && (d - d) == 0;
        d = sqrt(d);
        A[j * (j + 1) / 2 + j] = d;
#pragma unroll
        for (int i = j + 1; i < 7; i++) {
            double s = A[i * (i + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; k++) s -= A[i * (i + 1) / 2 + k] * A[j * (j + 1) / 2 + k];
            A[i * (i + 1) / 2 + j] = s / d;
        }
    }
    return ok;
}

struct Problem {
    int n_kf, n_edges, n_free;
    size_t kf0, e0, blk0;
    bool fix_scale;
};

// chi2 of every edge at the estimates S (S_cur or S_try), summed: F
__device__ double graph_chi2(const EGArgs& a, const Problem& P, const double* S, double* s_red) {
    double acc = 0;
    for (int e = threadIdx.x; e < P.n_edges; e += kThreads) {
        const int32_t* ed = a.edges + 3 * (P.e0 + e);
        double er[7];
        edge_error(load_sim3(a.w.C + 8 * (P.e0 + e)), load_sim3(S + 8 * (P.kf0 + ed[0])), load_sim3(S + 8 * (P.kf0 + ed[1])), er);
        double c = 0;
#pragma unroll
        for (int k = 0; k < 7; k++) c += er[k] * er[k];
        acc += c;
    }
    return block_sum(acc, s_red);
}

// computeActiveErrors and linearizeOplus of every edge (BaseBinaryEdge's numeric Jacobian, both vertices), then buildSystem by gathering per block row
__device__ double linearize(const EGArgs& a, const Problem& P, double* s_red) {
    const Workspace& w = a.w;
    const int tid = threadIdx.x;
    const double delta = 1e-9, scalar = 1.0 / (2 * delta);
    // items: (edge, p) with p = 0..13 a column of a Jacobian (vertex p / 7, dimension p % 7), p = 14 the error itself
    for (int it = tid; it < P.n_edges * 15; it += kThreads) {
        const int e = it / 15, p = it - 15 * e;
        const int32_t* ed = a.edges + 3 * (P.e0 + e);
        const Sim3 C = load_sim3(w.C + 8 * (P.e0 + e));
        Sim3 Si = load_sim3(w.S_cur + 8 * (P.kf0 + ed[0])), Sj = load_sim3(w.S_cur + 8 * (P.kf0 + ed[1]));
        double* JE = w.JE + kEdgeJ * (P.e0 + e);
        if (p == 14) {
            double er[7];
            edge_error(C, Si, Sj, er);
            double c = 0;
#pragma unroll
            for (int k = 0; k < 7; k++) { JE[98 + k] = er[k]; c += er[k] * er[k]; }
            w.chi[P.e0 + e] = c;
            continue;
        }
        const int side = p >= 7 ? 1 : 0, dim = p - 7 * side;
        if (a.fixed[P.kf0 + ed[side]]) continue;   // a fixed vertex gets no Jacobian
        double u[7], ep[7], em[7];
#pragma unroll
        for (int k = 0; k < 7; k++) u[k] = k == dim ? delta : 0.0;
        const Sim3 S0 = side ? Sj : Si;
        {
            const Sim3 Sp = oslam::sim3_oplus(S0, u, P.fix_scale);
            edge_error(C, side ? Si : Sp, side ? Sp : Sj, ep);
        }
#pragma unroll
        for (int k = 0; k < 7; k++) u[k] = k == dim ? -delta : 0.0;
        {
            const Sim3 Sm = oslam::sim3_oplus(S0, u, P.fix_scale);
            edge_error(C, side ? Si : Sm, side ? Sm : Sj, em);
        }
#pragma unroll
        for (int k = 0; k < 7; k++) JE[49 * side + 7 * k + dim] = scalar * (ep[k] - em[k]);
    }
    // H := 0 over the envelope
    {
        const size_t nb = (size_t)(w.rowstart[P.kf0 + P.n_free - 1] + (P.n_free - 1) - w.ffirst[P.kf0 + P.n_free - 1] + 1) * 49;
        double* H = w.H + P.blk0 * 49;
        for (size_t i = tid; i < nb; i += kThreads) H[i] = 0;
    }
    __syncthreads();
    // items: (free vertex f, entry): entries 0..48 of the blocks of row f, 49..55 of b.  The incident edges are visited in edge order.
    for (int it = tid; it < P.n_free * 56; it += kThreads) {
        const int f = it / 56, ent = it - 56 * f;
        const int k = w.kfof[P.kf0 + f];
        const int i0 = w.incstart[P.kf0 + k], cnt = w.inccnt[P.kf0 + k];
        const int ff = w.ffirst[P.kf0 + f];
        double* Hrow = w.H + (P.blk0 + w.rowstart[P.kf0 + f]) * 49;
        double acc = 0;
        const int r = ent < 49 ? ent / 7 : ent - 49, c = ent < 49 ? ent - 7 * (ent / 7) : 0;
        for (int q = 0; q < cnt; q++) {
            const int e = w.inc[2 * P.e0 + i0 + q];
            const int32_t* ed = a.edges + 3 * (P.e0 + e);
            const int side = ed[0] == k ? 0 : 1, other = ed[1 - side];
            const double* JE = w.JE + kEdgeJ * (P.e0 + e);
            const double* Ja = JE + 49 * side;
            if (ent >= 49) {   // b += A^T (-(Omega e))
                double s = 0;
#pragma unroll
                for (int m = 0; m < 7; m++) s += Ja[7 * m + r] * (-JE[98 + m]);
                acc += s;
                continue;
            }
            double s = 0;
#pragma unroll
            for (int m = 0; m < 7; m++) s += Ja[7 * m + r] * Ja[7 * m + c];
            acc += s;
            if (!a.fixed[P.kf0 + other]) {
                const int fo = w.fidx[P.kf0 + other];
                if (fo < f) {   // the block (f, fo) = J_f^T J_fo; the row of the higher vertex owns it
                    const double* Jo = JE + 49 * (1 - side);
                    double t = 0;
#pragma unroll
                    for (int m = 0; m < 7; m++) t += Ja[7 * m + r] * Jo[7 * m + c];
                    Hrow[(size_t)(fo - ff) * 49 + ent] += t;
                }
            }
        }
        if (ent >= 49) w.b[7 * (P.kf0 + f) + r] = acc;
        else Hrow[(size_t)(f - ff) * 49 + ent] = acc;
    }
    double facc = 0;
    for (int e = tid; e < P.n_edges; e += kThreads) facc += w.chi[P.e0 + e];
    return block_sum(facc, s_red);   // (its barriers also publish H and b)
}

// (H + lambda I) x = b over the envelope; false when a pivot is not positive and finite
__device__ bool factor_solve(const EGArgs& a, const Problem& P, double lambda) {
    const Workspace& w = a.w;
    const int tid = threadIdx.x, n = P.n_free;
    const int32_t *rowstart = w.rowstart + P.kf0, *ffirst = w.ffirst + P.kf0, *colstart = w.colstart + P.kf0, *colcnt = w.colcnt + P.kf0;
    const int32_t* collist = w.collist + P.blk0;
    double* L = w.L + P.blk0 * 49;
    const double* H = w.H + P.blk0 * 49;
    double *bw = w.bw + 7 * P.kf0, *y = w.y + 7 * P.kf0, *x = w.x + 7 * P.kf0, *Ld = w.Ld + 28 * P.kf0;
    // L := H + lambda I, bw := b
    for (int it = tid; it < n * 7; it += kThreads) bw[it] = w.b[7 * P.kf0 + it];
    for (int f = 0; f < n; f++) {
        const int nb = (f - ffirst[f] + 1) * 49;
        const size_t o = (size_t)rowstart[f] * 49;
        for (int i = tid; i < nb; i += kThreads) {
            double v = H[o + i];
            const int ent = i - (nb - 49);
            if (ent >= 0 && ent / 7 == ent % 7) v += lambda;
            L[o + i] = v;
        }
    }
    __syncthreads();
    for (int J = 0; J < n; J++) {
        // the diagonal block and y_J = L_JJ^-1 b_J, by every lane
        double D[28], yj[7];
        {
            const double* p = L + (size_t)(rowstart[J] + J - ffirst[J]) * 49;
#pragma unroll
            for (int r = 0; r < 7; r++)
#pragma unroll
                for (int c = 0; c <= r; c++) D[r * (r + 1) / 2 + c] = p[7 * r + c];
        }
        if (!chol7(D)) return false;   // (uniform: every lane has the same numbers)
#pragma unroll
        for (int r = 0; r < 7; r++) {
            double s = bw[7 * J + r];
#pragma unroll
            for (int c = 0; c < r; c++) s -= D[r * (r + 1) / 2 + c] * yj[c];
            yj[r] = s / D[r * (r + 1) / 2 + r];
        }
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < 28; k++) Ld[28 * J + k] = D[k];
#pragma unroll
            for (int k = 0; k < 7; k++) y[7 * J + k] = yj[k];
        }
        const int cnt = colcnt[J], c0 = colstart[J];
        // the blocks below: L_IJ = A_IJ L_JJ^-T, one lane per scalar row, which also subtracts L_IJ y_J from b_I
        for (int it = tid; it < cnt * 7; it += kThreads) {
            const int I = collist[c0 + it / 7], r = it % 7;
            double* p = L + (size_t)(rowstart[I] + J - ffirst[I]) * 49 + 7 * r;
            double l[7], s = 0;
#pragma unroll
            for (int c = 0; c < 7; c++) {
                double v = p[c];
#pragma unroll
                for (int k = 0; k < c; k++) v -= l[k] * D[c * (c + 1) / 2 + k];
                l[c] = v / D[c * (c + 1) / 2 + c];
                s += l[c] * yj[c];
            }
#pragma unroll
            for (int c = 0; c < 7; c++) p[c] = l[c];
            bw[7 * I + r] -= s;
        }
        __syncthreads();
        // the trailing blocks: A_IK -= L_IJ L_KJ^T for the rows I >= K of this column, one lane per entry
        const int npair = cnt * (cnt + 1) / 2;
        for (int it = tid; it < npair * 49; it += kThreads) {
            const int pr = it / 49, ent = it - 49 * pr;
            int ai = (int)((sqrtf(8.0f * (float)pr + 1.0f) - 1.0f) * 0.5f);
            while (ai * (ai + 1) / 2 > pr) ai--;
            while ((ai + 1) * (ai + 2) / 2 <= pr) ai++;
            const int bi = pr - ai * (ai + 1) / 2;
            const int I = collist[c0 + ai], K = collist[c0 + bi];   // the list ascends: I >= K
            const int r = ent / 7, c = ent - 7 * r;
            const double* li = L + (size_t)(rowstart[I] + J - ffirst[I]) * 49 + 7 * r;
            const double* lk = L + (size_t)(rowstart[K] + J - ffirst[K]) * 49 + 7 * c;
            double s = 0;
#pragma unroll
            for (int m = 0; m < 7; m++) s += li[m] * lk[m];
            L[(size_t)(rowstart[I] + K - ffirst[I]) * 49 + ent] -= s;
        }
        __syncthreads();
    }
    // L^T x = y, from the last block row upwards: x_I = L_II^-T y_I, then y_K -= L_IK^T x_I along the row's envelope
    for (int I = n - 1; I >= 0; I--) {
        double D[28], xi[7];
#pragma unroll
        for (int k = 0; k < 28; k++) D[k] = Ld[28 * I + k];
#pragma unroll
        for (int r = 6; r >= 0; r--) {
            double s = y[7 * I + r];
#pragma unroll
            for (int m = r + 1; m < 7; m++) s -= D[m * (m + 1) / 2 + r] * xi[m];
            xi[r] = s / D[r * (r + 1) / 2 + r];
        }
        if (tid == 0)
#pragma unroll
            for (int k = 0; k < 7; k++) x[7 * I + k] = xi[k];
        const int ff = ffirst[I];
        for (int it = tid; it < (I - ff) * 7; it += kThreads) {
            const int K = ff + it / 7, c = it % 7;
            const double* p = L + (size_t)(rowstart[I] + K - ff) * 49 + c;
            double s = 0;
#pragma unroll
            for (int r = 0; r < 7; r++) s += p[7 * r] * xi[r];
            y[7 * K + c] -= s;
        }
        __syncthreads();
    }
    return true;
}

__global__ __launch_bounds__(kThreads) void k_optimize_essential_graph(EGArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const oslam_essential_graph_problem_t& R = a.problems[b];
    const Workspace& w = a.w;
    int32_t* status = a.status + 4 * (size_t)b;
    __shared__ double s_red[kWaves];
    __shared__ int s_int[4];
    Problem P;
    P.n_kf = R.n_kf; P.n_edges = R.n_edges; P.fix_scale = R.fix_scale != 0;
    // a record that does not lie inside the arrays: -2, nothing else is written
    if (R.n_kf < 0 || R.kf_offset < 0 || R.kf_offset > a.n_kf_total - R.n_kf || R.n_edges < 0 || R.edge_offset < 0 || R.edge_offset > a.n_edges_total - R.n_edges ||
        R.env_blocks < 0 || R.env_offset < 0 || (long long)R.env_offset > a.max_blocks - (long long)R.env_blocks) {
        if (tid == 0) status[0] = -2;
        return;
    }
    P.kf0 = (size_t)R.kf_offset; P.e0 = (size_t)R.edge_offset; P.blk0 = (size_t)R.env_offset;

    // ---- validation ----
    bool ok = true, any_fixed = false;
    for (int k = tid; k < P.n_kf; k += kThreads) {
        const float* s = a.Scw + 13 * (P.kf0 + k);
        bool f = s[0] > 0.0f;
#pragma unroll
        for (int m = 0; m < 13; m++) f = f && finite_f(s[m]);
        if (a.has_nc[P.kf0 + k]) {
            const float* nc = a.Snc + 13 * (P.kf0 + k);
            f = f && nc[0] > 0.0f;
#pragma unroll
            for (int m = 0; m < 13; m++) f = f && finite_f(nc[m]);
        }
        ok = ok && f;
        any_fixed = any_fixed || a.fixed[P.kf0 + k] != 0;
    }
    for (int e = tid; e < P.n_edges; e += kThreads) {
        const int32_t* ed = a.edges + 3 * (P.e0 + e);
        ok = ok && ed[0] >= 0 && ed[0] < P.n_kf && ed[1] >= 0 && ed[1] < P.n_kf && ed[0] != ed[1] && (ed[2] == 0 || ed[2] == 1);
    }
    ok = __syncthreads_and(ok) != 0;
    any_fixed = __syncthreads_or(any_fixed) != 0;
    if (!ok || (P.n_kf > 0 && !any_fixed)) {
        if (tid == 0) { status[0] = -1; status[1] = 0; status[2] = P.n_edges; status[3] = 0; }
        return;
    }

    // ---- the free vertices, the envelope's rows (serial prefix sums by lane 0) ----
    if (tid == 0) {
        int nf = 0;
        for (int k = 0; k < P.n_kf; k++) {
            w.fidx[P.kf0 + k] = nf;   // a fixed keyframe gets the index of the next free one: a first column named by it starts there
            if (!a.fixed[P.kf0 + k]) { w.kfof[P.kf0 + nf] = k; nf++; }
        }
        long long acc = 0;
        bool good = true;
        for (int f = 0; f < nf; f++) {
            const int k = w.kfof[P.kf0 + f], rf = a.row_first[P.kf0 + k];
            if (rf < 0 || rf > k) { good = false; break; }
            const int ff = w.fidx[P.kf0 + rf];
            w.ffirst[P.kf0 + f] = ff;
            w.rowstart[P.kf0 + f] = (int)acc;
            acc += f - ff + 1;
            if (acc > (long long)R.env_blocks) { good = false; break; }
        }
        s_int[0] = nf; s_int[1] = good ? 1 : 0;
    }
    __syncthreads();
    P.n_free = s_int[0];
    bool env_ok = s_int[1] != 0;
    if (env_ok)
        for (int e = tid; e < P.n_edges; e += kThreads) {   // every edge between two free vertices must lie inside the envelope
            const int32_t* ed = a.edges + 3 * (P.e0 + e);
            if (a.fixed[P.kf0 + ed[0]] || a.fixed[P.kf0 + ed[1]]) continue;
            const int f0 = w.fidx[P.kf0 + ed[0]], f1 = w.fidx[P.kf0 + ed[1]];
            const int hi = f0 > f1 ? f0 : f1, lo = f0 > f1 ? f1 : f0;
            env_ok = env_ok && w.ffirst[P.kf0 + hi] <= lo;
        }
    env_ok = __syncthreads_and(env_ok) != 0;
    if (!env_ok) {
        if (tid == 0) status[0] = -2;
        return;
    }

    // ---- estimates and measurements ----
    for (int k = tid; k < P.n_kf; k += kThreads) {
        const Sim3 S = sim3_from_floats(a.Scw + 13 * (P.kf0 + k));
        store_sim3(S, w.S_cur + 8 * (P.kf0 + k));
        store_sim3(S, w.S_try + 8 * (P.kf0 + k));
    }
    for (int e = tid; e < P.n_edges; e += kThreads) {
        const int32_t* ed = a.edges + 3 * (P.e0 + e);
        const size_t ki = P.kf0 + ed[0], kj = P.kf0 + ed[1];
        const bool nc = ed[2] == 1;   // kind 1: the non-corrected Sim3 where the keyframe has one
        const Sim3 Siw = sim3_from_floats((nc && a.has_nc[ki] ? a.Snc : a.Scw) + 13 * ki);
        const Sim3 Sjw = sim3_from_floats((nc && a.has_nc[kj] ? a.Snc : a.Scw) + 13 * kj);
        store_sim3(oslam::sim3_mul(Sjw, oslam::sim3_inv(Siw)), w.C + 8 * (P.e0 + e));   // Sji = Sjw * Swi
    }

    int n_its = 0, n_trials = 0;
    if (P.n_free > 0 && P.n_edges > 0) {
        const int n = P.n_free;
        // ---- structure: the incident edges of every keyframe in edge order, the rows of every block column in ascending order ----
        for (int k = tid; k < P.n_kf; k += kThreads) {
            int c = 0;
            for (int e = 0; e < P.n_edges; e++) {
                const int32_t* ed = a.edges + 3 * (P.e0 + e);
                c += (ed[0] == k || ed[1] == k) ? 1 : 0;
            }
            w.inccnt[P.kf0 + k] = c;
        }
        for (int J = tid; J < n; J += kThreads) {
            int c = 0;
            for (int I = J + 1; I < n; I++) c += w.ffirst[P.kf0 + I] <= J ? 1 : 0;
            w.colcnt[P.kf0 + J] = c;
        }
        __syncthreads();
        if (tid == 0) {
            int acc = 0;
            for (int k = 0; k < P.n_kf; k++) { w.incstart[P.kf0 + k] = acc; acc += w.inccnt[P.kf0 + k]; }
            acc = 0;
            for (int J = 0; J < n; J++) { w.colstart[P.kf0 + J] = acc; acc += w.colcnt[P.kf0 + J]; }   // (at most the envelope's blocks less its diagonal)
        }
        __syncthreads();
        for (int k = tid; k < P.n_kf; k += kThreads) {
            int o = w.incstart[P.kf0 + k];
            for (int e = 0; e < P.n_edges; e++) {
                const int32_t* ed = a.edges + 3 * (P.e0 + e);
                if (ed[0] == k || ed[1] == k) w.inc[2 * P.e0 + o++] = e;
            }
        }
        for (int J = tid; J < n; J += kThreads) {
            int o = w.colstart[P.kf0 + J];
            for (int I = J + 1; I < n; I++)
                if (w.ffirst[P.kf0 + I] <= J) w.collist[P.blk0 + o++] = I;
        }
        __syncthreads();

        // ---- SparseOptimizer::optimize(20) with OptimizationAlgorithmLevenberg, setUserLambdaInit(1e-16) ----
        double* trace = a.trace ? a.trace + (size_t)b * kTraceRows * 6 : nullptr;
        double lambda = 1e-16, ni = 2;
        for (int it = 0; it < 20; it++) {
            double currentChi = linearize(a, P, s_red);
            double rho = 0;
            int qmax = 0;
            do {
                const bool ok2 = factor_solve(a, P, lambda);
                __syncthreads();
                double sc = 0;   // computeScale
                for (int i = tid; i < 7 * n; i += kThreads) {
                    const double xv = ok2 ? w.x[7 * P.kf0 + i] : 0.0;
                    sc += xv * (lambda * xv + w.b[7 * P.kf0 + i]);
                }
                for (int f = tid; f < n; f += kThreads) {
                    const int k = w.kfof[P.kf0 + f];
                    double xv[7];
#pragma unroll
                    for (int m = 0; m < 7; m++) xv[m] = ok2 ? w.x[7 * (P.kf0 + f) + m] : 0.0;
                    store_sim3(oslam::sim3_oplus(load_sim3(w.S_cur + 8 * (P.kf0 + k)), xv, P.fix_scale), w.S_try + 8 * (P.kf0 + k));
                }
                double scale = block_sum(sc, s_red);
                double tempChi = graph_chi2(a, P, w.S_try, s_red);
                if (!ok2) tempChi = kDBL_MAX;
                rho = currentChi - tempChi;
                scale += 1e-3;
                rho /= scale;
                const bool accepted = rho > 0 && (tempChi - tempChi) == 0;
                if (trace && tid == 0 && n_trials < kTraceRows) {
                    double* t = trace + 6 * n_trials;
                    t[0] = currentChi; t[1] = tempChi; t[2] = rho; t[3] = lambda; t[4] = accepted ? 1.0 : 0.0; t[5] = (it == 0 && qmax == 0) ? 1.0 : 0.0;
                }
                if (accepted) {
                    double alpha = 1. - (2 * rho - 1) * (2 * rho - 1) * (2 * rho - 1);
                    alpha = fmin(alpha, 2. / 3.);
                    lambda *= fmax(1. / 3., alpha);
                    ni = 2;
                    currentChi = tempChi;
                    for (int f = tid; f < n; f += kThreads) {
                        const int k = w.kfof[P.kf0 + f];
#pragma unroll
                        for (int m = 0; m < 8; m++) w.S_cur[8 * (P.kf0 + k) + m] = w.S_try[8 * (P.kf0 + k) + m];
                    }
                } else {
                    lambda *= ni;
                    ni *= 2;
                }
                __syncthreads();
                qmax++;
                n_trials++;
            } while (rho < 0 && qmax < 10);
            n_its++;
            if (qmax == 10 || rho == 0) break;   // OptimizationAlgorithm::Terminate
        }
    }
    __syncthreads();

    // ---- SE3 recovery (:992-1009): [R | t / s] ----
    for (int k = tid; k < P.n_kf; k += kThreads) {
        const Sim3 S = load_sim3(w.S_cur + 8 * (P.kf0 + k));
        oslam::SE3 q;
#pragma unroll
        for (int m = 0; m < 4; m++) q.q[m] = S.q[m];
        double Rm[9];
        oslam::se3_R(q, Rm);
        double* o = a.Scw_out + 13 * (P.kf0 + k);
#pragma unroll
        for (int m = 0; m < 9; m++) o[m] = Rm[m];
#pragma unroll
        for (int m = 0; m < 3; m++) o[9 + m] = S.t[m];
        o[12] = S.s;
        const double is = 1. / S.s;
        float* T = a.Tcw_out + 16 * (P.kf0 + k);
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) T[4 * r + c] = (float)Rm[3 * r + c];
            T[4 * r + 3] = (float)(S.t[r] * is);
        }
        T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
    }
    if (tid == 0) {
        status[0] = 0; status[1] = P.n_free; status[2] = P.n_edges; status[3] = 256 * n_its + n_trials;
        if (a.trace_n) a.trace_n[b] = n_trials;
    }
}

struct PointArgs {
    const oslam_essential_graph_problem_t* problems;
    int n_problems, n_kf_total, n_points;
    const float* Scw; const double* Scw_out; const int32_t* status;
    const int32_t *point_problem, *ref;
    const float* P; float* P_out;
};

// :1013-1043: P' = correctedSwr.map(Srw.map(P)) with the keyframe's Sim3 before and after the optimisation
__global__ __launch_bounds__(256) void k_correct_points(PointArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.n_points) return;
    const int r = a.ref[i], pp = a.point_problem[i];
    if (r < 0 || pp < 0 || pp >= a.n_problems) return;
    const oslam_essential_graph_problem_t& R = a.problems[pp];
    if (a.status[4 * (size_t)pp] != 0 || R.n_kf < 0 || r >= R.n_kf || R.kf_offset < 0 || R.kf_offset > a.n_kf_total - R.n_kf) return;
    const size_t k = (size_t)R.kf_offset + r;
    const Sim3 Srw = sim3_from_floats(a.Scw + 13 * k);
    Sim3 Sc;
    const double* o = a.Scw_out + 13 * k;
    oslam::quat_from_R(o, Sc.q);
#pragma unroll
    for (int m = 0; m < 3; m++) Sc.t[m] = o[9 + m];
    Sc.s = o[12];
    const Sim3 Swr = oslam::sim3_inv(Sc);
    const double X[3] = {(double)a.P[3 * i], (double)a.P[3 * i + 1], (double)a.P[3 * i + 2]};
    double c[3], rc[3], v[3];
    oslam::quat_rot(Srw.q, X, rc);
#pragma unroll
    for (int m = 0; m < 3; m++) c[m] = Srw.s * rc[m] + Srw.t[m];
    oslam::quat_rot(Swr.q, c, rc);
#pragma unroll
    for (int m = 0; m < 3; m++) v[m] = Swr.s * rc[m] + Swr.t[m];
#pragma unroll
    for (int m = 0; m < 3; m++) a.P_out[3 * i + m] = (float)v[m];
}

int check_call(const char* fn, const oslam_essential_graph* h, int n_problems, int n_kf, int n_edges) {
    if (!h) { set_error("%s: NULL handle", fn); return OSLAM_E_INVALID; }
    if (n_problems < 0 || n_kf < 0 || n_edges < 0) { set_error("%s: %d problems, %d keyframes, %d edges: none may be negative", fn, n_problems, n_kf, n_edges); return OSLAM_E_CAPACITY; }
    if (n_problems > h->max_problems) { set_error("%s: %d problems exceed the handle's %d", fn, n_problems, h->max_problems); return OSLAM_E_CAPACITY; }
    if (n_kf > h->max_kf) { set_error("%s: %d keyframes exceed the handle's %d", fn, n_kf, h->max_kf); return OSLAM_E_CAPACITY; }
    if (n_edges > h->max_edges) { set_error("%s: %d edges exceed the handle's %d", fn, n_edges, h->max_edges); return OSLAM_E_CAPACITY; }
    return OSLAM_OK;
}

// the workspace's arrays, laid out once at creation
struct WsLayout {
    oslam::StageLayout lay;
    oslam::Field<double> S_cur, S_try, b, bw, y, x, Ld, C, JE, chi, H, L;
    oslam::Field<int32_t> fidx, kfof, ffirst, rowstart, colstart, colcnt, incstart, inccnt, inc, collist;
    WsLayout(size_t kf, size_t ed, size_t blk) {
        S_cur = lay.add<double>(kf * 8); S_try = lay.add<double>(kf * 8);
        b = lay.add<double>(kf * 7); bw = lay.add<double>(kf * 7); y = lay.add<double>(kf * 7); x = lay.add<double>(kf * 7);
        Ld = lay.add<double>(kf * 28);
        C = lay.add<double>(ed * 8); JE = lay.add<double>(ed * kEdgeJ); chi = lay.add<double>(ed);
        H = lay.add<double>(blk * 49); L = lay.add<double>(blk * 49);
        fidx = lay.add<int32_t>(kf); kfof = lay.add<int32_t>(kf); ffirst = lay.add<int32_t>(kf); rowstart = lay.add<int32_t>(kf);
        colstart = lay.add<int32_t>(kf); colcnt = lay.add<int32_t>(kf); incstart = lay.add<int32_t>(kf); inccnt = lay.add<int32_t>(kf);
        inc = lay.add<int32_t>(ed * 2); collist = lay.add<int32_t>(blk);
    }
    Workspace on(uint8_t* base) const {
        Workspace w;
        w.S_cur = at(S_cur, base); w.S_try = at(S_try, base); w.b = at(b, base); w.bw = at(bw, base); w.y = at(y, base); w.x = at(x, base); w.Ld = at(Ld, base);
        w.C = at(C, base); w.JE = at(JE, base); w.chi = at(chi, base); w.H = at(H, base); w.L = at(L, base);
        w.fidx = at(fidx, base); w.kfof = at(kfof, base); w.ffirst = at(ffirst, base); w.rowstart = at(rowstart, base); w.colstart = at(colstart, base);
        w.colcnt = at(colcnt, base); w.incstart = at(incstart, base); w.inccnt = at(inccnt, base); w.inc = at(inc, base); w.collist = at(collist, base);
        return w;
    }
};

}  // namespace

extern "C" {

void oslam_essential_graph_destroy(oslam_essential_graph_t* h) {
    if (!h) return;
    delete h;
}

int oslam_essential_graph_create(oslam_essential_graph_t** out, int max_problems, int max_keyframes_total, int max_edges_total, long long max_envelope_blocks_total, int device) {
    const char* fn = "oslam_essential_graph_create";
    if (!out) { set_error("%s: out is NULL", fn); return OSLAM_E_INVALID; }
    *out = nullptr;
    if (max_problems < 1 || max_keyframes_total < 1 || max_edges_total < 1 || max_envelope_blocks_total < 1 || max_envelope_blocks_total > 0x7fffffffLL) {
        set_error("%s: bad argument", fn);
        return OSLAM_E_INVALID;
    }
    const int ndev = oslam_device_count();
    if (ndev <= 0) return oslam::no_device(fn);
    if (device < 0 || device >= ndev) { set_error("%s: device out of range", fn); return OSLAM_E_INVALID; }
    oslam_essential_graph* h = new oslam_essential_graph;
    h->device = device; h->max_problems = max_problems; h->max_kf = max_keyframes_total; h->max_edges = max_edges_total; h->max_blocks = max_envelope_blocks_total;
    const WsLayout L((size_t)h->max_kf, (size_t)h->max_edges, (size_t)h->max_blocks);
    int rc = hipSetDevice(device) == hipSuccess ? OSLAM_OK : OSLAM_E_HIP;
    if (rc) set_error("%s: hipSetDevice failed", fn);
    if (!rc) rc = h->ws.alloc(L.lay.total());
    if (rc) { delete h; return rc; }
    *out = h;
    return OSLAM_OK;
}

int oslam_optimize_essential_graph_batch_device(oslam_essential_graph_t* h, int n_problems, const oslam_essential_graph_problem_t* d_problems, int n_kf_total, const float* d_Scw,
                                                const float* d_Snc, const uint8_t* d_has_noncorrected, const uint8_t* d_fixed, const int32_t* d_row_first, int n_edges_total,
                                                const int32_t* d_edges, double* d_Scw_out, float* d_Tcw_out, int32_t* d_status, double* d_trace, int32_t* d_trace_n, void* stream) {
    const char* fn = "oslam_optimize_essential_graph_batch_device";
    OSLAM_CHECK(check_call(fn, h, n_problems, n_kf_total, n_edges_total));
    if (n_problems == 0) return OSLAM_OK;
    if (!d_problems || !d_status || (n_kf_total > 0 && (!d_Scw || !d_Snc || !d_has_noncorrected || !d_fixed || !d_row_first || !d_Scw_out || !d_Tcw_out)) ||
        (n_edges_total > 0 && !d_edges) || (d_trace && !d_trace_n)) {
        set_error("%s: NULL argument", fn);
        return OSLAM_E_INVALID;
    }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const WsLayout L((size_t)h->max_kf, (size_t)h->max_edges, (size_t)h->max_blocks);
    EGArgs a;
    a.problems = d_problems; a.n_problems = n_problems; a.n_kf_total = n_kf_total; a.n_edges_total = n_edges_total; a.max_blocks = h->max_blocks;
    a.Scw = d_Scw; a.Snc = d_Snc; a.has_nc = d_has_noncorrected; a.fixed = d_fixed; a.edges = d_edges; a.row_first = d_row_first;
    a.Scw_out = d_Scw_out; a.Tcw_out = d_Tcw_out; a.status = d_status; a.trace = d_trace; a.trace_n = d_trace_n;
    a.w = L.on(h->ws.bytes());
    hipLaunchKernelGGL(k_optimize_essential_graph, dim3(n_problems), dim3(kThreads), 0, (hipStream_t)stream, a);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int oslam_essential_graph_envelope(int n_problems, const oslam_essential_graph_problem_t* problems, int n_kf_total, const uint8_t* fixed, int n_edges_total, const int32_t* edges,
                                   int32_t* row_first, int64_t* env_blocks) {
    const char* fn = "oslam_essential_graph_envelope";
    if (n_problems < 0 || n_kf_total < 0 || n_edges_total < 0 || (n_problems > 0 && (!problems || !env_blocks)) || (n_kf_total > 0 && (!fixed || !row_first)) ||
        (n_edges_total > 0 && !edges)) {
        set_error("%s: bad argument", fn);
        return OSLAM_E_INVALID;
    }
    for (int b = 0; b < n_problems; b++) {
        const oslam_essential_graph_problem_t& P = problems[b];
        if (P.n_kf < 0 || P.kf_offset < 0 || P.kf_offset > n_kf_total - P.n_kf || P.n_edges < 0 || P.edge_offset < 0 || P.edge_offset > n_edges_total - P.n_edges) {
            set_error("%s: problem %d (%d keyframes at %d, %d edges at %d) lies outside the %d keyframes or the %d edges", fn, b, P.n_kf, P.kf_offset, P.n_edges, P.edge_offset,
                      n_kf_total, n_edges_total);
            return OSLAM_E_INVALID;
        }
        int32_t* rf = row_first + P.kf_offset;
        const uint8_t* fx = fixed + P.kf_offset;
        for (int k = 0; k < P.n_kf; k++) rf[k] = k;
        for (int e = 0; e < P.n_edges; e++) {
            const int32_t* ed = edges + 3 * ((size_t)P.edge_offset + e);
            const int i = ed[0], j = ed[1];
            if (i < 0 || i >= P.n_kf || j < 0 || j >= P.n_kf) continue;   // (the kernel reports the problem as invalid)
            const int hi = i > j ? i : j, lo = i > j ? j : i;
            if (lo < rf[hi]) rf[hi] = lo;
        }
        int64_t blocks = 0;
        std::vector<int32_t> fidx((size_t)P.n_kf);
        int nf = 0;
        for (int k = 0; k < P.n_kf; k++) { fidx[k] = nf; if (!fx[k]) nf++; }
        for (int k = 0; k < P.n_kf; k++)
            if (!fx[k]) blocks += fidx[k] - fidx[rf[k]] + 1;
        env_blocks[b] = blocks;
    }
    return OSLAM_OK;
}

int oslam_optimize_essential_graph_batch(oslam_essential_graph_t* h, int n_problems, const oslam_essential_graph_problem_t* problems, int n_kf_total, const float* Scw,
                                         const float* Snc, const uint8_t* has_noncorrected, const uint8_t* fixed, int n_edges_total, const int32_t* edges, double* Scw_out,
                                         float* Tcw_out, int32_t* status, double* trace, int32_t* trace_n) {
    const char* fn = "oslam_optimize_essential_graph_batch";
    OSLAM_CHECK(check_call(fn, h, n_problems, n_kf_total, n_edges_total));
    if (n_problems == 0) return OSLAM_OK;
    if (!problems || !status || (n_kf_total > 0 && (!Scw || !Snc || !has_noncorrected || !fixed || !Scw_out || !Tcw_out)) || (n_edges_total > 0 && !edges) || (trace && !trace_n)) {
        set_error("%s: NULL argument", fn);
        return OSLAM_E_INVALID;
    }
    const size_t np = (size_t)n_problems, N = (size_t)n_kf_total, E = (size_t)n_edges_total;
    std::vector<oslam_essential_graph_problem_t> pr(problems, problems + np);
    std::vector<int32_t> row_first(N);
    std::vector<int64_t> blocks(np);
    OSLAM_CHECK(oslam_essential_graph_envelope(n_problems, problems, n_kf_total, fixed, n_edges_total, edges, row_first.data(), blocks.data()));
    int64_t total = 0;
    for (size_t b = 0; b < np; b++) {
        pr[b].env_offset = (int32_t)total; pr[b].env_blocks = (int32_t)blocks[b];
        total += blocks[b];
        if (total > h->max_blocks) {
            set_error("%s: the envelopes of problems 0..%zu hold %lld 7 x 7 blocks, more than the handle's %lld", fn, b, (long long)total, h->max_blocks);
            return OSLAM_E_CAPACITY;
        }
    }
    std::lock_guard<std::mutex> lock(h->mu);
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    oslam::StageLayout lay;   // one block, inputs then outputs: one upload, one download
    const auto fPr = lay.add<oslam_essential_graph_problem_t>(np);
    const auto fS = lay.add<float>(N * 13), fN = lay.add<float>(N * 13);
    const auto fHn = lay.add<uint8_t>(N), fFx = lay.add<uint8_t>(N);
    const auto fRf = lay.add<int32_t>(N), fEd = lay.add<int32_t>(E * 3);
    const auto fSo = lay.add<double>(N * 13);
    const auto fTo = lay.add<float>(N * 16);
    const auto fSt = lay.add<int32_t>(np * 4), fTn = lay.add<int32_t>(np);
    const auto fTr = lay.add<double>(np * kTraceRows * 6, trace != nullptr);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fPr, ph, (const oslam_essential_graph_problem_t*)pr.data()); put(fS, ph, Scw); put(fN, ph, Snc); put(fHn, ph, has_noncorrected); put(fFx, ph, fixed);
    put(fRf, ph, (const int32_t*)row_first.data()); put(fEd, ph, edges);
    // the caller's output bytes travel too: what no problem owns, or the kernel leaves alone, comes back as it was
    put(fSo, ph, (const double*)Scw_out); put(fTo, ph, (const float*)Tcw_out); put(fSt, ph, (const int32_t*)status);
    if (trace) { put(fTn, ph, (const int32_t*)trace_n); put(fTr, ph, (const double*)trace); }
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, nullptr));
    OSLAM_CHECK(oslam_optimize_essential_graph_batch_device(h, n_problems, at(fPr, pd), n_kf_total, at(fS, pd), at(fN, pd), at(fHn, pd), at(fFx, pd), at(fRf, pd), n_edges_total,
                                                            at(fEd, pd), at(fSo, pd), at(fTo, pd), at(fSt, pd), at(fTr, pd), trace ? at(fTn, pd) : nullptr, nullptr));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fSo.off, pd + fSo.off, lay.total() - fSo.off, hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(fSo, ph, Scw_out); get(fTo, ph, Tcw_out); get(fSt, ph, status);
    if (trace) { get(fTn, ph, trace_n); get(fTr, ph, trace); }
    return OSLAM_OK;
}

int oslam_essential_graph_correct_points_device(oslam_essential_graph_t* h, int n_problems, const oslam_essential_graph_problem_t* d_problems, int n_kf_total, const float* d_Scw,
                                                const double* d_Scw_out, const int32_t* d_status, int n_points, const int32_t* d_point_problem, const int32_t* d_ref,
                                                const float* d_P, float* d_P_out, void* stream) {
    const char* fn = "oslam_essential_graph_correct_points_device";
    OSLAM_CHECK(check_call(fn, h, n_problems, n_kf_total, 0));
    if (n_points < 0) { set_error("%s: %d points", fn, n_points); return OSLAM_E_CAPACITY; }
    if (n_points == 0 || n_problems == 0) return OSLAM_OK;
    if (!d_problems || !d_Scw || !d_Scw_out || !d_status || !d_point_problem || !d_ref || !d_P || !d_P_out) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    PointArgs a;
    a.problems = d_problems; a.n_problems = n_problems; a.n_kf_total = n_kf_total; a.n_points = n_points;
    a.Scw = d_Scw; a.Scw_out = d_Scw_out; a.status = d_status; a.point_problem = d_point_problem; a.ref = d_ref; a.P = d_P; a.P_out = d_P_out;
    hipLaunchKernelGGL(k_correct_points, dim3(oslam::div_up(n_points, 256)), dim3(256), 0, (hipStream_t)stream, a);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int oslam_essential_graph_correct_points(oslam_essential_graph_t* h, int n_problems, const oslam_essential_graph_problem_t* problems, int n_kf_total, const float* Scw,
                                         const double* Scw_out, const int32_t* status, int n_points, const int32_t* point_problem, const int32_t* ref, const float* P,
                                         float* P_out) {
    const char* fn = "oslam_essential_graph_correct_points";
    OSLAM_CHECK(check_call(fn, h, n_problems, n_kf_total, 0));
    if (n_points < 0) { set_error("%s: %d points", fn, n_points); return OSLAM_E_CAPACITY; }
    if (n_points == 0 || n_problems == 0) return OSLAM_OK;
    if (!problems || !Scw || !Scw_out || !status || !point_problem || !ref || !P || !P_out) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    std::lock_guard<std::mutex> lock(h->mu);
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t np = (size_t)n_problems, N = (size_t)n_kf_total, M = (size_t)n_points;
    oslam::StageLayout lay;
    const auto fPr = lay.add<oslam_essential_graph_problem_t>(np);
    const auto fS = lay.add<float>(N * 13);
    const auto fSo = lay.add<double>(N * 13);
    const auto fSt = lay.add<int32_t>(np * 4), fPp = lay.add<int32_t>(M), fRe = lay.add<int32_t>(M);
    const auto fP = lay.add<float>(M * 3);
    const auto fPo = lay.add<float>(M * 3);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fPr, ph, problems); put(fS, ph, Scw); put(fSo, ph, Scw_out); put(fSt, ph, status); put(fPp, ph, point_problem); put(fRe, ph, ref); put(fP, ph, P);
    put(fPo, ph, (const float*)P_out);   // skipped points keep the caller's bytes
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, nullptr));
    OSLAM_CHECK(oslam_essential_graph_correct_points_device(h, n_problems, at(fPr, pd), n_kf_total, at(fS, pd), at(fSo, pd), at(fSt, pd), n_points, at(fPp, pd), at(fRe, pd),
                                                            at(fP, pd), at(fPo, pd), nullptr));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fPo.off, pd + fPo.off, fPo.bytes, hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(fPo, ph, P_out);
    return OSLAM_OK;
}

}  // extern "C"
