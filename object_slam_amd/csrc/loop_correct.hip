// loop_correct.hip — the map corrections of LoopClosing (reference src/LoopClosing.cc) for batches of independent sequences on gfx950 (include/oslam_hip.h,
// "LoopClosing: map corrections"): mg2oScw = gScm * gSmw (:334-336), CorrectLoop's Sim3 propagation with its point correction and corrected poses
// (:436-517), and the map update after global BA (:677-738).  The points and keyframe entries of all problems are one flat index space: every problem is
// spread over kSplit workgroups, so a single large problem does not sit on one CU.  The point claims are integer atomicMin, the counters integer atomicAdd;
// no floating-point sum depends on the batch.  The Sim3 / SE3 / quaternion pieces are those of sim3_math.h and se3_math.h.  Product code; never includes oracle/.
#include <climits>
#include <cmath>
#include <mutex>
#include <vector>

#include "common.h"
#include "loop_parent_check.h"
#include "se3_math.h"
#include "sim3_math.h"
#include "stage_layout.h"

using oslam::set_error;
using oslam::Sim3;

struct oslam_loop_correct {
    int device = 0, max_problems = 0, max_kf = 0, max_entries = 0, max_points = 0;
    int epoch = 0;            // the number of the propagation call: ws.bad[b] == epoch marks problem b of this call as invalid
    oslam::DeviceBuffer ws;   // Workspace
    oslam::StagePair io;      // staging of the host-pointer entry points
    std::mutex mu;
};

namespace {

constexpr int kThreads = 256;
constexpr int kSplit = 32;   // workgroups per problem (grid.y)

struct Workspace {
    double* S;        // [max_kf][16]: Corrected q[4] t[3] s, NonCorrected q[4] t[3] s
    int32_t* claim;   // [max_points]: the smallest keyframe index that holds the point, INT_MAX without one
    int32_t* bad;     // [max_problems]: the epoch of the last call that found the problem invalid
    int32_t* done;    // [max_kf]: the round (from 1) in which the GBA sweep settled the keyframe, 0 = not reached
};

struct WsLayout {
    oslam::StageLayout lay;
    oslam::Field<double> S;
    oslam::Field<int32_t> claim, bad, done;
    WsLayout(size_t np, size_t kf, size_t pts) { S = lay.add<double>(kf * 16); claim = lay.add<int32_t>(pts); bad = lay.add<int32_t>(np); done = lay.add<int32_t>(kf); }
    Workspace on(uint8_t* base) const {
        Workspace w;
        w.S = at(S, base); w.claim = at(claim, base); w.bad = at(bad, base); w.done = at(done, base);
        return w;
    }
};

__device__ __forceinline__ bool finite_f(float v) { return (v - v) == 0.0f; }
__device__ __forceinline__ bool finite_d(double v) { return (v - v) == 0.0; }

// KeyFrame::SetPose (src/KeyFrame.cc:74-81): Twc = [Rcw.t() | -Rcw.t() * tcw; 0 0 0 1], Ow the three float products summed in float from left to right, negated
__device__ __forceinline__ void set_pose_twc(const float* Tcw, float* Twc) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float a = Tcw[r], b = Tcw[4 + r], c = Tcw[8 + r];   // row r of Rwc = column r of Rcw
        Twc[4 * r] = a; Twc[4 * r + 1] = b; Twc[4 * r + 2] = c;
        Twc[4 * r + 3] = -(a * Tcw[3] + b * Tcw[7] + c * Tcw[11]);
    }
    Twc[12] = 0.f; Twc[13] = 0.f; Twc[14] = 0.f; Twc[15] = 1.f;
}

// CV_32F 4 x 4 product: every entry the float sum, left to right, of its four float products (cv::gemm's small-matrix branch)
__device__ __forceinline__ void mat4_mul(const float* A, const float* B, float* C) {
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) C[4 * r + c] = A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c] + A[4 * r + 2] * B[8 + c] + A[4 * r + 3] * B[12 + c];
}

// cv::Mat 3x3 * 3x1 + 3x1 as one cv::gemm (gemm_row of window_search.h): the float sum of the three products, the + t in double, rounded once
__device__ __forceinline__ float rx_plus_t(float a0, float a1, float a2, const float* x, float t) {
    const float t0 = a0 * x[0] + a1 * x[1] + a2 * x[2];
    return (float)((double)t0 + (double)t);
}

// g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0) of a CV_32F pose
__device__ __forceinline__ Sim3 sim3_from_pose(const float* T) {
    Sim3 S;
    const double R[9] = {(double)T[0], (double)T[1], (double)T[2], (double)T[4], (double)T[5], (double)T[6], (double)T[8], (double)T[9], (double)T[10]};
    oslam::quat_from_R(R, S.q);
    S.t[0] = (double)T[3]; S.t[1] = (double)T[7]; S.t[2] = (double)T[11];
    S.s = 1.0;
    return S;
}

// g2o::Sim3(Quaterniond(R), t, s) of 13 doubles R row-major, t, s
__device__ __forceinline__ Sim3 sim3_from_Rts(const double* p) {
    Sim3 S;
    oslam::quat_from_R(p, S.q);
    S.t[0] = p[9]; S.t[1] = p[10]; S.t[2] = p[11];
    S.s = p[12];
    return S;
}

__device__ __forceinline__ void sim3_R(const Sim3& S, double R[9]) {   // r.toRotationMatrix()
    oslam::SE3 q;
#pragma unroll
    for (int k = 0; k < 4; k++) q.q[k] = S.q[k];
    oslam::se3_R(q, R);
}

__device__ __forceinline__ void store_Rts(const Sim3& S, double* p) {
    sim3_R(S, p);
    p[9] = S.t[0]; p[10] = S.t[1]; p[11] = S.t[2];
    p[12] = S.s;
}

__device__ __forceinline__ void sim3_map(const Sim3& S, const double x[3], double o[3]) {   // Sim3::map: s (r x) + t
    double rx[3];
    oslam::quat_rot(S.q, x, rx);
#pragma unroll
    for (int m = 0; m < 3; m++) o[m] = S.s * rx[m] + S.t[m];
}

// ---------------------------------------------------------------- mg2oScw (:334-336)
struct ComposeArgs { int n; const double* Scm; const float* Tmw; double* Scw; float* mScw; };

__global__ __launch_bounds__(kThreads) void k_compose_scw(ComposeArgs a) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= a.n) return;
    const Sim3 gScm = sim3_from_Rts(a.Scm + 13 * (size_t)b);
    const Sim3 gSmw = sim3_from_pose(a.Tmw + 16 * (size_t)b);
    const Sim3 S = oslam::sim3_mul(gScm, gSmw);
    double* o = a.Scw + 13 * (size_t)b;
    store_Rts(S, o);
    float* M = a.mScw + 16 * (size_t)b;   // Converter::toCvMat(Sim3) = toCvSE3(s * R, t) (src/Converter.cc:56-62)
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) M[4 * r + c] = (float)(S.s * o[3 * r + c]);
        M[4 * r + 3] = (float)S.t[r];
    }
    M[12] = 0.f; M[13] = 0.f; M[14] = 0.f; M[15] = 1.f;
}

// ---------------------------------------------------------------- CorrectLoop's propagation (:436-517)
struct PropArgs {
    const oslam_loop_correct_problem_t* problems;
    int n_problems, n_kf_total, n_entries_total, n_points_total, epoch;
    const float* Tiw; const double* Scw; const int32_t* kf_entries; const int32_t* entries; const float* P; const uint8_t* bad;
    double *Scorr_out, *Snc_out; float *Tiw_out, *P_out; int32_t *corrected_ref, *status;
    Workspace w;
};

__device__ __forceinline__ bool prop_inside(const oslam_loop_correct_problem_t& R, const PropArgs& a) {
    return R.n_kf >= 0 && R.kf_offset >= 0 && R.kf_offset <= a.n_kf_total - R.n_kf && R.n_entries >= 0 && R.entry_offset >= 0 &&
           R.entry_offset <= a.n_entries_total - R.n_entries && R.n_points >= 0 && R.point_offset >= 0 && R.point_offset <= a.n_points_total - R.n_points;
}

// launch 1: what makes a problem invalid, and the claim words of its points
__global__ __launch_bounds__(kThreads) void k_prop_check(PropArgs a) {
    const int b = blockIdx.x, y = blockIdx.y, tid = threadIdx.x;
    const oslam_loop_correct_problem_t R = a.problems[b];
    if (!prop_inside(R, a)) {
        if (y == 0 && tid == 0) { int32_t* st = a.status + 4 * (size_t)b; st[0] = -2; st[1] = 0; st[2] = 0; st[3] = 0; }
        return;
    }
    bool ok = true;
    if (y == 0 && tid == 0) {
        const double* S = a.Scw + 13 * (size_t)b;
        for (int m = 0; m < 13; m++) ok = ok && finite_d(S[m]);
        ok = ok && S[12] > 0 && R.cur >= 0 && R.cur < R.n_kf;
        int32_t* st = a.status + 4 * (size_t)b;
        st[0] = 0; st[1] = R.n_kf; st[2] = 0; st[3] = 0;
    }
    for (int k = y; k < R.n_kf; k += kSplit) {
        const size_t row = (size_t)R.kf_offset + k;
        if (tid < 16) ok = ok && finite_f(a.Tiw[16 * row + tid]);
        const int first = a.kf_entries[2 * row], cnt = a.kf_entries[2 * row + 1];
        if (first < 0 || cnt < 0 || first > R.n_entries - cnt) { ok = false; continue; }
        const int32_t* e = a.entries + (size_t)R.entry_offset + first;
        for (int j = tid; j < cnt; j += kThreads) ok = ok && e[j] >= -1 && e[j] < R.n_points;
    }
    if (!ok) a.w.bad[b] = a.epoch;   // every writer stores the same value
    for (int i = y * kThreads + tid; i < R.n_points; i += kSplit * kThreads) a.w.claim[(size_t)R.point_offset + i] = INT_MAX;
}

// launch 2: the Sim3 of every keyframe, its corrected pose, and the claims of its entries
__global__ __launch_bounds__(kThreads) void k_prop_keyframes(PropArgs a) {
    const int b = blockIdx.x, y = blockIdx.y, tid = threadIdx.x;
    const oslam_loop_correct_problem_t R = a.problems[b];
    if (!prop_inside(R, a)) return;
    if (a.w.bad[b] == a.epoch) {
        if (y == 0 && tid == 0) a.status[4 * (size_t)b] = -1;
        return;
    }
    __shared__ int s_cnt;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (int k = y + kSplit * tid; k < R.n_kf; k += kSplit * kThreads) {   // one lane per keyframe of this workgroup's share
        const size_t row = (size_t)R.kf_offset + k;
        const float* Tiw = a.Tiw + 16 * row;
        const Sim3 Scw = sim3_from_Rts(a.Scw + 13 * (size_t)b);
        Sim3 Sc;
        if (k != R.cur) {
            float Twc[16], Tic[16];
            set_pose_twc(a.Tiw + 16 * ((size_t)R.kf_offset + R.cur), Twc);   // mpCurrentKF->GetPoseInverse() (:441)
            mat4_mul(Tiw, Twc, Tic);                                          // :456
            Sc = oslam::sim3_mul(sim3_from_pose(Tic), Scw);                   // :459-460
        } else Sc = Scw;                                                      // :440
        const Sim3 Snc = sim3_from_pose(Tiw);                                 // :465-469
        double* ws = a.w.S + 16 * row;
#pragma unroll
        for (int m = 0; m < 4; m++) { ws[m] = Sc.q[m]; ws[8 + m] = Snc.q[m]; }
#pragma unroll
        for (int m = 0; m < 3; m++) { ws[4 + m] = Sc.t[m]; ws[12 + m] = Snc.t[m]; }
        ws[7] = Sc.s; ws[15] = Snc.s;
        double* so = a.Scorr_out + 13 * row;
        store_Rts(Sc, so);
        store_Rts(Snc, a.Snc_out + 13 * row);
        const double inv = 1. / Sc.s;   // eigt *= (1. / s) (:509)
        float* To = a.Tiw_out + 16 * row;
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) To[4 * r + c] = (float)so[3 * r + c];
            To[4 * r + 3] = (float)(Sc.t[r] * inv);
        }
        To[12] = 0.f; To[13] = 0.f; To[14] = 0.f; To[15] = 1.f;
    }
    int local = 0;
    for (int k = y; k < R.n_kf; k += kSplit) {
        const size_t row = (size_t)R.kf_offset + k;
        const int first = a.kf_entries[2 * row], cnt = a.kf_entries[2 * row + 1];
        const int32_t* e = a.entries + (size_t)R.entry_offset + first;
        for (int j = tid; j < cnt; j += kThreads) {
            const int p = e[j];
            if (p < 0) continue;                                  // !pMPi (:485)
            local++;
            if (a.bad[(size_t)R.point_offset + p]) continue;      // isBad() (:487)
            atomicMin(&a.w.claim[(size_t)R.point_offset + p], k); // mnCorrectedByKF (:489), in ascending keyframe index
        }
    }
    if (local) atomicAdd(&s_cnt, local);
    __syncthreads();
    if (tid == 0 && s_cnt) atomicAdd(&a.status[4 * (size_t)b + 3], s_cnt);
}

// launch 3: the points
__global__ __launch_bounds__(kThreads) void k_prop_points(PropArgs a) {
    const int b = blockIdx.x, y = blockIdx.y, tid = threadIdx.x;
    const oslam_loop_correct_problem_t R = a.problems[b];
    if (!prop_inside(R, a) || a.w.bad[b] == a.epoch) return;
    __shared__ int s_cnt;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    int local = 0;
    for (int i = y * kThreads + tid; i < R.n_points; i += kSplit * kThreads) {
        const size_t pi = (size_t)R.point_offset + i;
        const int k = a.w.claim[pi];
        if (k == INT_MAX) { a.corrected_ref[pi] = -1; continue; }
        a.corrected_ref[pi] = k;                                   // mnCorrectedReference (:500)
        const double* ws = a.w.S + 16 * ((size_t)R.kf_offset + k);
        Sim3 Sc, Snc;
#pragma unroll
        for (int m = 0; m < 4; m++) { Sc.q[m] = ws[m]; Snc.q[m] = ws[8 + m]; }
#pragma unroll
        for (int m = 0; m < 3; m++) { Sc.t[m] = ws[4 + m]; Snc.t[m] = ws[12 + m]; }
        Sc.s = ws[7]; Snc.s = ws[15];
        const Sim3 Swi = oslam::sim3_inv(Sc);                      // :477
        const double X[3] = {(double)a.P[3 * pi], (double)a.P[3 * pi + 1], (double)a.P[3 * pi + 2]};
        double c[3], v[3];
        sim3_map(Snc, X, c);                                       // :495
        sim3_map(Swi, c, v);
#pragma unroll
        for (int m = 0; m < 3; m++) a.P_out[3 * pi + m] = (float)v[m];
        local++;
    }
    if (local) atomicAdd(&s_cnt, local);
    __syncthreads();
    if (tid == 0 && s_cnt) atomicAdd(&a.status[4 * (size_t)b + 2], s_cnt);
}

// ---------------------------------------------------------------- the map update after global BA (:677-738)
struct GbaArgs {
    const oslam_loop_gba_problem_t* problems;
    int n_problems, n_kf_total, n_points_total;
    const int32_t* parent; const uint8_t* kf_in_ba; const float *Tcw, *TcwGBA;
    const float *P, *PosGBA; const uint8_t *pt_in_ba, *bad; const int32_t* ref;
    float* Tcw_out; uint8_t* reached; float* P_out; int32_t* status;
    Workspace w;
};

__device__ __forceinline__ bool gba_inside(const oslam_loop_gba_problem_t& R, const GbaArgs& a) {
    return R.n_kf >= 0 && R.kf_offset >= 0 && R.kf_offset <= a.n_kf_total - R.n_kf && R.n_points >= 0 && R.point_offset >= 0 &&
           R.point_offset <= a.n_points_total - R.n_points;
}

// launch 1, one workgroup per map: the sweep over the spanning tree by depth.  Round 1 settles the roots; round r + 1 settles every keyframe whose parent
// was settled in a round <= r.  Every round but the last settles at least one keyframe, so there are at most n_kf of them.
__global__ __launch_bounds__(kThreads) void k_gba_keyframes(GbaArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const oslam_loop_gba_problem_t R = a.problems[b];
    int32_t* st = a.status + 4 * (size_t)b;
    if (!gba_inside(R, a)) {
        if (tid == 0) { st[0] = -2; st[1] = 0; st[2] = 0; st[3] = 0; }
        return;
    }
    __shared__ int s_bad, s_any, s_prop;
    if (tid == 0) { s_bad = R.refuse != 0; s_any = 0; s_prop = 0; }
    __syncthreads();
    const size_t ko = (size_t)R.kf_offset;
    for (int k = tid; k < R.n_kf; k += kThreads) {
        const int p = a.parent[ko + k];
        const bool in_ba = a.kf_in_ba[ko + k] != 0;
        bool ok = p >= -1 && p < R.n_kf && p != k && (p >= 0 || in_ba);   // a root outside the BA: the reference would read an unset mTcwGBA
        for (int m = 0; m < 16; m++) ok = ok && finite_f(a.Tcw[16 * (ko + k) + m]) && (!in_ba || finite_f(a.TcwGBA[16 * (ko + k) + m]));
        if (!ok) s_bad = 1;
    }
    __syncthreads();
    if (s_bad) {
        if (tid == 0) { st[0] = -1; st[1] = 0; st[2] = 0; st[3] = 0; }
        return;
    }
    for (int k = tid; k < R.n_kf; k += kThreads) {
        const bool root = a.parent[ko + k] < 0;
        a.w.done[ko + k] = root ? 1 : 0;
        if (root) {
            for (int m = 0; m < 16; m++) a.Tcw_out[16 * (ko + k) + m] = a.TcwGBA[16 * (ko + k) + m];
            s_any = 1;
        }
    }
    __syncthreads();
    int rounds = s_any ? 1 : 0;
    for (int r = 1; r < R.n_kf && rounds == r; r++) {
        __syncthreads();
        if (tid == 0) s_any = 0;
        __syncthreads();
        int prop = 0;
        for (int k = tid; k < R.n_kf; k += kThreads) {
            if (a.w.done[ko + k] != 0) continue;
            const int p = a.parent[ko + k];
            const int dp = a.w.done[ko + p];
            if (dp == 0 || dp > r) continue;
            float* To = a.Tcw_out + 16 * (ko + k);
            if (a.kf_in_ba[ko + k]) {
                for (int m = 0; m < 16; m++) To[m] = a.TcwGBA[16 * (ko + k) + m];
            } else {
                float Twc[16], Tchildc[16], T[16], Tp[16];
                set_pose_twc(a.Tcw + 16 * (ko + p), Twc);             // pKF->GetPoseInverse() of the pose before the update (:684)
                mat4_mul(a.Tcw + 16 * (ko + k), Twc, Tchildc);        // :690
                for (int m = 0; m < 16; m++) Tp[m] = a.Tcw_out[16 * (ko + p) + m];
                mat4_mul(Tchildc, Tp, T);                             // :691
                for (int m = 0; m < 16; m++) To[m] = T[m];
                prop++;
            }
            a.w.done[ko + k] = r + 1;
            s_any = 1;
        }
        if (prop) atomicAdd(&s_prop, prop);
        __syncthreads();
        if (s_any) rounds = r + 1;
    }
    __syncthreads();
    for (int k = tid; k < R.n_kf; k += kThreads) {
        const bool got = a.w.done[ko + k] != 0;
        a.reached[ko + k] = got ? 1 : 0;
        if (!got) for (int m = 0; m < 16; m++) a.Tcw_out[16 * (ko + k) + m] = a.Tcw[16 * (ko + k) + m];
    }
    if (tid == 0) { st[0] = 0; st[1] = s_prop; st[2] = 0; st[3] = rounds; }
}

// launch 2: the points of all maps (:706-738)
__global__ __launch_bounds__(kThreads) void k_gba_points(GbaArgs a) {
    const int b = blockIdx.x, y = blockIdx.y, tid = threadIdx.x;
    const oslam_loop_gba_problem_t R = a.problems[b];
    if (!gba_inside(R, a) || a.status[4 * (size_t)b] != 0) return;
    __shared__ int s_cnt;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    int local = 0;
    for (int i = y * kThreads + tid; i < R.n_points; i += kSplit * kThreads) {
        const size_t pi = (size_t)R.point_offset + i;
        if (a.bad[pi]) continue;                                   // :710
        if (a.pt_in_ba[pi]) {                                      // :713-717
#pragma unroll
            for (int m = 0; m < 3; m++) a.P_out[3 * pi + m] = a.PosGBA[3 * pi + m];
            local++;
            continue;
        }
        const int r = a.ref[pi];
        if (r < 0 || r >= R.n_kf || !a.reached[(size_t)R.kf_offset + r]) continue;   // :723
        const float* Tb = a.Tcw + 16 * ((size_t)R.kf_offset + r);                      // mTcwBefGBA
        const float X[3] = {a.P[3 * pi], a.P[3 * pi + 1], a.P[3 * pi + 2]};
        const float Xc[3] = {rx_plus_t(Tb[0], Tb[1], Tb[2], X, Tb[3]), rx_plus_t(Tb[4], Tb[5], Tb[6], X, Tb[7]), rx_plus_t(Tb[8], Tb[9], Tb[10], X, Tb[11])};   // :729
        float Tn[16], Twc[16];
        for (int m = 0; m < 16; m++) Tn[m] = a.Tcw_out[16 * ((size_t)R.kf_offset + r) + m];
        set_pose_twc(Tn, Twc);                                     // :732
#pragma unroll
        for (int m = 0; m < 3; m++) a.P_out[3 * pi + m] = rx_plus_t(Twc[4 * m], Twc[4 * m + 1], Twc[4 * m + 2], Xc, Twc[4 * m + 3]);   // :736
        local++;
    }
    if (local) atomicAdd(&s_cnt, local);
    __syncthreads();
    if (tid == 0 && s_cnt) atomicAdd(&a.status[4 * (size_t)b + 2], s_cnt);
}

int check_call(const char* fn, const oslam_loop_correct* h, int n_problems, int n_kf, int n_entries, int n_points) {
    if (!h) { set_error("%s: NULL handle", fn); return OSLAM_E_INVALID; }
    if (n_problems < 0 || n_kf < 0 || n_entries < 0 || n_points < 0) {
        set_error("%s: %d problems, %d keyframes, %d entries, %d points: none may be negative", fn, n_problems, n_kf, n_entries, n_points);
        return OSLAM_E_CAPACITY;
    }
    if (n_problems > h->max_problems) { set_error("%s: %d problems exceed the handle's %d", fn, n_problems, h->max_problems); return OSLAM_E_CAPACITY; }
    if (n_kf > h->max_kf) { set_error("%s: %d keyframes exceed the handle's %d", fn, n_kf, h->max_kf); return OSLAM_E_CAPACITY; }
    if (n_entries > h->max_entries) { set_error("%s: %d entries exceed the handle's %d", fn, n_entries, h->max_entries); return OSLAM_E_CAPACITY; }
    if (n_points > h->max_points) { set_error("%s: %d points exceed the handle's %d", fn, n_points, h->max_points); return OSLAM_E_CAPACITY; }
    return OSLAM_OK;
}

Workspace workspace(const oslam_loop_correct* h) {
    return WsLayout((size_t)h->max_problems, (size_t)h->max_kf, (size_t)h->max_points).on(h->ws.bytes());
}

}  // namespace

extern "C" {

void oslam_loop_correct_destroy(oslam_loop_correct_t* h) {
    if (!h) return;
    delete h;
}

int oslam_loop_correct_create(oslam_loop_correct_t** out, int max_problems, int max_keyframes_total, int max_entries_total, int max_points_total, int device) {
    const char* fn = "oslam_loop_correct_create";
    if (!out) { set_error("%s: out is NULL", fn); return OSLAM_E_INVALID; }
    *out = nullptr;
    if (max_problems < 1 || max_keyframes_total < 1 || max_entries_total < 1 || max_points_total < 1) { set_error("%s: bad argument", fn); return OSLAM_E_INVALID; }
    const int ndev = oslam_device_count();
    if (ndev <= 0) return oslam::no_device(fn);
    if (device < 0 || device >= ndev) { set_error("%s: device out of range", fn); return OSLAM_E_INVALID; }
    oslam_loop_correct* h = new oslam_loop_correct;
    h->device = device; h->max_problems = max_problems; h->max_kf = max_keyframes_total; h->max_entries = max_entries_total; h->max_points = max_points_total;
    const WsLayout L((size_t)max_problems, (size_t)max_keyframes_total, (size_t)max_points_total);
    int rc = hipSetDevice(device) == hipSuccess ? OSLAM_OK : OSLAM_E_HIP;
    if (rc) set_error("%s: hipSetDevice failed", fn);
    if (!rc) rc = h->ws.alloc(L.lay.total());
    if (!rc && hipMemset(h->ws.bytes(), 0, L.lay.total()) != hipSuccess) { set_error("%s: hipMemset failed", fn); rc = OSLAM_E_HIP; }   // bad[] = 0: no epoch yet
    if (rc) { delete h; return rc; }
    *out = h;
    return OSLAM_OK;
}

int oslam_loop_compose_scw_device(oslam_loop_correct_t* h, int n, const double* d_Scm, const float* d_Tmw, double* d_Scw, float* d_mScw, void* stream) {
    const char* fn = "oslam_loop_compose_scw_device";
    OSLAM_CHECK(check_call(fn, h, n, 0, 0, 0));
    if (n == 0) return OSLAM_OK;
    if (!d_Scm || !d_Tmw || !d_Scw || !d_mScw) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    ComposeArgs a;
    a.n = n; a.Scm = d_Scm; a.Tmw = d_Tmw; a.Scw = d_Scw; a.mScw = d_mScw;
    hipLaunchKernelGGL(k_compose_scw, dim3(oslam::div_up(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, a);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int oslam_loop_compose_scw(oslam_loop_correct_t* h, int n, const double* Scm, const float* Tmw, double* Scw, float* mScw) {
    const char* fn = "oslam_loop_compose_scw";
    OSLAM_CHECK(check_call(fn, h, n, 0, 0, 0));
    if (n == 0) return OSLAM_OK;
    if (!Scm || !Tmw || !Scw || !mScw) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    std::lock_guard<std::mutex> lock(h->mu);
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    oslam::StageLayout lay;
    const auto fS = lay.add<double>((size_t)n * 13);
    const auto fT = lay.add<float>((size_t)n * 16);
    const auto fSo = lay.add<double>((size_t)n * 13);
    const auto fMo = lay.add<float>((size_t)n * 16);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fS, ph, Scm); put(fT, ph, Tmw);
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, fSo.off, hipMemcpyHostToDevice, nullptr));
    OSLAM_CHECK(oslam_loop_compose_scw_device(h, n, at(fS, pd), at(fT, pd), at(fSo, pd), at(fMo, pd), nullptr));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fSo.off, pd + fSo.off, lay.total() - fSo.off, hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(fSo, ph, Scw); get(fMo, ph, mScw);
    return OSLAM_OK;
}

int oslam_loop_propagate_device(oslam_loop_correct_t* h, int n_problems, const oslam_loop_correct_problem_t* d_problems, int n_kf_total, const float* d_Tiw, const double* d_Scw,
                                const int32_t* d_kf_entries, int n_entries_total, const int32_t* d_entries, int n_points_total, const float* d_P, const uint8_t* d_bad,
                                double* d_Scorr_out, double* d_Snc_out, float* d_Tiw_out, float* d_P_out, int32_t* d_corrected_ref, int32_t* d_status, void* stream) {
    const char* fn = "oslam_loop_propagate_device";
    OSLAM_CHECK(check_call(fn, h, n_problems, n_kf_total, n_entries_total, n_points_total));
    if (n_problems == 0) return OSLAM_OK;
    if (!d_problems || !d_Scw || !d_status || (n_kf_total > 0 && (!d_Tiw || !d_kf_entries || !d_Scorr_out || !d_Snc_out || !d_Tiw_out)) || (n_entries_total > 0 && !d_entries) ||
        (n_points_total > 0 && (!d_P || !d_bad || !d_P_out || !d_corrected_ref))) {
        set_error("%s: NULL argument", fn);
        return OSLAM_E_INVALID;
    }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    PropArgs a;
    a.problems = d_problems; a.n_problems = n_problems; a.n_kf_total = n_kf_total; a.n_entries_total = n_entries_total; a.n_points_total = n_points_total;
    a.epoch = ++h->epoch;
    a.Tiw = d_Tiw; a.Scw = d_Scw; a.kf_entries = d_kf_entries; a.entries = d_entries; a.P = d_P; a.bad = d_bad;
    a.Scorr_out = d_Scorr_out; a.Snc_out = d_Snc_out; a.Tiw_out = d_Tiw_out; a.P_out = d_P_out; a.corrected_ref = d_corrected_ref; a.status = d_status;
    a.w = workspace(h);
    const dim3 grid(n_problems, kSplit);
    hipLaunchKernelGGL(k_prop_check, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(k_prop_keyframes, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(k_prop_points, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int oslam_loop_propagate(oslam_loop_correct_t* h, int n_problems, const oslam_loop_correct_problem_t* problems, int n_kf_total, const float* Tiw, const double* Scw,
                         const int32_t* kf_entries, int n_entries_total, const int32_t* entries, int n_points_total, const float* P, const uint8_t* bad, double* Scorr_out,
                         double* Snc_out, float* Tiw_out, float* P_out, int32_t* corrected_ref, int32_t* status) {
    const char* fn = "oslam_loop_propagate";
    OSLAM_CHECK(check_call(fn, h, n_problems, n_kf_total, n_entries_total, n_points_total));
    if (n_problems == 0) return OSLAM_OK;
    if (!problems || !Scw || !status || (n_kf_total > 0 && (!Tiw || !kf_entries || !Scorr_out || !Snc_out || !Tiw_out)) || (n_entries_total > 0 && !entries) ||
        (n_points_total > 0 && (!P || !bad || !P_out || !corrected_ref))) {
        set_error("%s: NULL argument", fn);
        return OSLAM_E_INVALID;
    }
    for (int b = 0; b < n_problems; b++) {
        const oslam_loop_correct_problem_t& R = problems[b];
        if (R.n_kf < 0 || R.kf_offset < 0 || R.kf_offset > n_kf_total - R.n_kf || R.n_entries < 0 || R.entry_offset < 0 || R.entry_offset > n_entries_total - R.n_entries ||
            R.n_points < 0 || R.point_offset < 0 || R.point_offset > n_points_total - R.n_points) {
            set_error("%s: problem %d (%d keyframes at %d, %d entries at %d, %d points at %d) lies outside the %d keyframes, %d entries or %d points", fn, b, R.n_kf, R.kf_offset,
                      R.n_entries, R.entry_offset, R.n_points, R.point_offset, n_kf_total, n_entries_total, n_points_total);
            return OSLAM_E_INVALID;
        }
    }
    std::lock_guard<std::mutex> lock(h->mu);
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    const size_t np = (size_t)n_problems, N = (size_t)n_kf_total, E = (size_t)n_entries_total, M = (size_t)n_points_total;
    oslam::StageLayout lay;   // one block, inputs then outputs: one upload, one download
    const auto fPr = lay.add<oslam_loop_correct_problem_t>(np);
    const auto fT = lay.add<float>(N * 16);
    const auto fS = lay.add<double>(np * 13);
    const auto fKe = lay.add<int32_t>(N * 2), fEn = lay.add<int32_t>(E);
    const auto fP = lay.add<float>(M * 3);
    const auto fBd = lay.add<uint8_t>(M);
    const auto fSc = lay.add<double>(N * 13), fSn = lay.add<double>(N * 13);
    const auto fTo = lay.add<float>(N * 16), fPo = lay.add<float>(M * 3);
    const auto fCr = lay.add<int32_t>(M), fSt = lay.add<int32_t>(np * 4);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fPr, ph, problems); put(fT, ph, Tiw); put(fS, ph, Scw); put(fKe, ph, kf_entries); put(fEn, ph, entries); put(fP, ph, P); put(fBd, ph, bad);
    // the caller's output bytes travel too: what no problem owns, or the kernels leave alone, comes back as it was
    put(fSc, ph, (const double*)Scorr_out); put(fSn, ph, (const double*)Snc_out); put(fTo, ph, (const float*)Tiw_out); put(fPo, ph, (const float*)P_out);
    put(fCr, ph, (const int32_t*)corrected_ref); put(fSt, ph, (const int32_t*)status);
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, nullptr));
    OSLAM_CHECK(oslam_loop_propagate_device(h, n_problems, at(fPr, pd), n_kf_total, at(fT, pd), at(fS, pd), at(fKe, pd), n_entries_total, at(fEn, pd), n_points_total, at(fP, pd),
                                            at(fBd, pd), at(fSc, pd), at(fSn, pd), at(fTo, pd), at(fPo, pd), at(fCr, pd), at(fSt, pd), nullptr));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fSc.off, pd + fSc.off, lay.total() - fSc.off, hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(fSc, ph, Scorr_out); get(fSn, ph, Snc_out); get(fTo, ph, Tiw_out); get(fPo, ph, P_out); get(fCr, ph, corrected_ref); get(fSt, ph, status);
    return OSLAM_OK;
}

int oslam_loop_update_after_gba_device(oslam_loop_correct_t* h, int n_problems, const oslam_loop_gba_problem_t* d_problems, int n_kf_total, const int32_t* d_parent,
                                       const uint8_t* d_kf_in_ba, const float* d_Tcw, const float* d_TcwGBA, int n_points_total, const float* d_P, const float* d_PosGBA,
                                       const uint8_t* d_pt_in_ba, const uint8_t* d_bad, const int32_t* d_ref, float* d_Tcw_out, uint8_t* d_reached, float* d_P_out,
                                       int32_t* d_status, void* stream) {
    const char* fn = "oslam_loop_update_after_gba_device";
    OSLAM_CHECK(check_call(fn, h, n_problems, n_kf_total, 0, n_points_total));
    if (n_problems == 0) return OSLAM_OK;
    if (!d_problems || !d_status || (n_kf_total > 0 && (!d_parent || !d_kf_in_ba || !d_Tcw || !d_TcwGBA || !d_Tcw_out || !d_reached)) ||
        (n_points_total > 0 && (!d_P || !d_PosGBA || !d_pt_in_ba || !d_bad || !d_ref || !d_P_out))) {
        set_error("%s: NULL argument", fn);
        return OSLAM_E_INVALID;
    }
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    GbaArgs a;
    a.problems = d_problems; a.n_problems = n_problems; a.n_kf_total = n_kf_total; a.n_points_total = n_points_total;
    a.parent = d_parent; a.kf_in_ba = d_kf_in_ba; a.Tcw = d_Tcw; a.TcwGBA = d_TcwGBA; a.P = d_P; a.PosGBA = d_PosGBA; a.pt_in_ba = d_pt_in_ba; a.bad = d_bad; a.ref = d_ref;
    a.Tcw_out = d_Tcw_out; a.reached = d_reached; a.P_out = d_P_out; a.status = d_status;
    a.w = workspace(h);
    hipLaunchKernelGGL(k_gba_keyframes, dim3(n_problems), dim3(kThreads), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(k_gba_points, dim3(n_problems, kSplit), dim3(kThreads), 0, (hipStream_t)stream, a);
    OSLAM_HIP_CHECK(hipGetLastError());
    return OSLAM_OK;
}

int oslam_loop_update_after_gba(oslam_loop_correct_t* h, int n_problems, const oslam_loop_gba_problem_t* problems, int n_kf_total, const int32_t* parent, const uint8_t* kf_in_ba,
                                const float* Tcw, const float* TcwGBA, int n_points_total, const float* P, const float* PosGBA, const uint8_t* pt_in_ba, const uint8_t* bad,
                                const int32_t* ref, float* Tcw_out, uint8_t* reached, float* P_out, int32_t* status) {
    const char* fn = "oslam_loop_update_after_gba";
    OSLAM_CHECK(check_call(fn, h, n_problems, n_kf_total, 0, n_points_total));
    if (n_problems == 0) return OSLAM_OK;
    if (!problems || !status || (n_kf_total > 0 && (!parent || !kf_in_ba || !Tcw || !TcwGBA || !Tcw_out || !reached)) ||
        (n_points_total > 0 && (!P || !PosGBA || !pt_in_ba || !bad || !ref || !P_out))) {
        set_error("%s: NULL argument", fn);
        return OSLAM_E_INVALID;
    }
    const size_t np = (size_t)n_problems, N = (size_t)n_kf_total, M = (size_t)n_points_total;
    std::vector<oslam_loop_gba_problem_t> pr(problems, problems + np);
    std::vector<uint8_t> mark;
    bool any = false;
    for (size_t b = 0; b < np; b++) {
        const oslam_loop_gba_problem_t& R = pr[b];
        if (R.n_kf < 0 || R.kf_offset < 0 || R.kf_offset > n_kf_total - R.n_kf || R.n_points < 0 || R.point_offset < 0 || R.point_offset > n_points_total - R.n_points) {
            set_error("%s: problem %zu (%d keyframes at %d, %d points at %d) lies outside the %d keyframes or %d points", fn, b, R.n_kf, R.kf_offset, R.n_points, R.point_offset,
                      n_kf_total, n_points_total);
            return OSLAM_E_INVALID;
        }
        // indices inside the problem and no cycle, before anything is launched: the sweep would leave the keyframes of a cycle unreached and call that a result
        pr[b].refuse = oslam::parent_tree_check(parent + R.kf_offset, R.n_kf, mark) != oslam::kParentOk;
        any = any || !pr[b].refuse;
    }
    if (!any) {   // nothing to launch
        for (size_t b = 0; b < np; b++) { status[4 * b] = -1; status[4 * b + 1] = 0; status[4 * b + 2] = 0; status[4 * b + 3] = 0; }
        return OSLAM_OK;
    }
    std::lock_guard<std::mutex> lock(h->mu);
    OSLAM_HIP_CHECK(hipSetDevice(h->device));
    oslam::StageLayout lay;
    const auto fPr = lay.add<oslam_loop_gba_problem_t>(np);
    const auto fPa = lay.add<int32_t>(N);
    const auto fKb = lay.add<uint8_t>(N);
    const auto fT = lay.add<float>(N * 16), fTg = lay.add<float>(N * 16), fP = lay.add<float>(M * 3), fPg = lay.add<float>(M * 3);
    const auto fPb = lay.add<uint8_t>(M), fBd = lay.add<uint8_t>(M);
    const auto fRf = lay.add<int32_t>(M);
    const auto fTo = lay.add<float>(N * 16);
    const auto fRe = lay.add<uint8_t>(N);
    const auto fPo = lay.add<float>(M * 3);
    const auto fSt = lay.add<int32_t>(np * 4);
    OSLAM_CHECK(h->io.grow(lay.total(), 4096));
    uint8_t *ph = h->io.h.bytes(), *pd = h->io.d.bytes();
    put(fPr, ph, (const oslam_loop_gba_problem_t*)pr.data()); put(fPa, ph, parent); put(fKb, ph, kf_in_ba); put(fT, ph, Tcw); put(fTg, ph, TcwGBA); put(fP, ph, P);
    put(fPg, ph, PosGBA); put(fPb, ph, pt_in_ba); put(fBd, ph, bad); put(fRf, ph, ref);
    put(fTo, ph, (const float*)Tcw_out); put(fRe, ph, (const uint8_t*)reached); put(fPo, ph, (const float*)P_out); put(fSt, ph, (const int32_t*)status);
    OSLAM_HIP_CHECK(hipMemcpyAsync(pd, ph, lay.total(), hipMemcpyHostToDevice, nullptr));
    OSLAM_CHECK(oslam_loop_update_after_gba_device(h, n_problems, at(fPr, pd), n_kf_total, at(fPa, pd), at(fKb, pd), at(fT, pd), at(fTg, pd), n_points_total, at(fP, pd),
                                                   at(fPg, pd), at(fPb, pd), at(fBd, pd), at(fRf, pd), at(fTo, pd), at(fRe, pd), at(fPo, pd), at(fSt, pd), nullptr));
    OSLAM_HIP_CHECK(hipMemcpyAsync(ph + fTo.off, pd + fTo.off, lay.total() - fTo.off, hipMemcpyDeviceToHost, nullptr));
    OSLAM_HIP_CHECK(hipStreamSynchronize(nullptr));
    get(fTo, ph, Tcw_out); get(fRe, ph, reached); get(fPo, ph, P_out); get(fSt, ph, status);
    return OSLAM_OK;
}

}  // extern "C"
