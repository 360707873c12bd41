// lba_win.inc — local bundle adjustment, ONE WORKGROUP PER WINDOW, the whole Levenberg-Marquardt schedule in one launch (included by lba.hip inside
// namespace oslam).  The layout of the batch-of-sequences driver: a step solves a few hundred independent windows (5-30 free keyframes, 1-3 k points,
// 4-13 k edges each), so the GPU is filled ACROSS windows (one CU each; the hardware dispatcher hands a finished workgroup's CU to the next window, so small
// windows do not wait for large ones) and a window never leaves its CU: no launch boundaries, no host polling, no inter-workgroup synchronisation.
// Reference: Optimizer::LocalBundleAdjustment src/Optimizer.cc:453-778 (g2o BlockSolver_6_3 + OptimizationAlgorithmLevenberg, SURVEY.md Appendix B).
//
// With 256 windows in flight a CU's share of the HBM bandwidth is ~30 GB/s (13 bytes per clock) against 64 fp64 operations per clock, and the per-edge
// blocks of the normal equations (B_e = Hpl: 144 bytes, W_e: 144 bytes, their (W_a, B_b) pairs: 288 bytes per pair, 4.4 pairs per edge in the driver's
// steady-state windows) would have to stream from HBM in every LM trial (measured: 3.3 ms per trial and window, as slow as the multi-launch layout).  So
// this kernel keeps NO per-edge block in memory: Jacobians are recomputed from the 21 bytes of edge input wherever they are needed (~500 operations per
// edge, cheaper than the 144 bytes they would replace), and the Schur complement is formed on chip:
//
//   lin     (per LM iteration) edges are numbered KEYFRAME-major and cut into chunks of <= 64 of one keyframe (pose, "free keyframe" test and the pose-block
//           reduction are wave-uniform, a wave reads consecutive edge records): chi2, robust sum, the pose part J_p^T W J_p / J_p^T W e summed per wave over
//           its run of chunks of a keyframe, then per keyframe in chunk order; the point part J_x^T W J_x / J_x^T W e by one thread per point in edge order;
//   schur   (per LM trial) points are cut into tiles of <= TE edges in free keyframes.  Per tile: (Hll + lambda I)^-1 of its points, then B_e and
//           W_e = B_e (Hll + lambda I)^-1 of its edges into LDS, then every 6x6 block of the reduced system — owned by one thread (or m threads when there are
//           fewer blocks than threads) with its 36 + 6 sums in registers — adds the W_a B_b^T products of the tile's pairs of that block, read from LDS
//           through a host-built (tile, block) pair list; the sums go to the LDS-resident reduced system (upper block triangle, packed) in a fixed order;
//   chol    blocked U^T U (6-wide panels, look-ahead on the next diagonal block) + register-resident back substitution, all in LDS;
//   update  landmark back substitution (B_e^T x_a = J_x^T W (J_p x_a), Jacobians recomputed), exponential map of the pose increments; eval: chi2 of the
//           trial state; LM control (uniform in every thread).
// All sums have a fixed order (no floating-point atomics): two runs give identical bits.

constexpr int kWinThreads = 512;
constexpr int kWinWaves = kWinThreads / 64;
constexpr int kWinLdsMax = 155 * 1024;   // dynamic LDS of a window's workgroup (the CU has 160 KB; ~3.5 KB of static LDS beside it)
constexpr int kWinGroupsMax = 4;         // passes over the tiles when a window has more 6x6 blocks with pairs than threads (<= 4 x 512 blocks: 63 free keyframes)
constexpr int kWinTileEdgesMax = 512;    // staged edges per tile (16-bit local indices in the pair list)
constexpr int kWinTilePointsMax = 128;
constexpr int kWinSplitMax = 32;         // threads per 6x6 block when the window has few blocks

struct LbaWin {
    // Edge numbering of this layout: KEYFRAME-major (sorted by keyframe, then point): LbaProblem::e_kf / e_pt / e_obs / e_info, chi2, level, erase follow it;
    // a keyframe's edges are cut into chunks of <= 64 consecutive ids, a point finds its edges through pt_edge.
    const int* chunk_kf;        // [nchunk] keyframe of the chunk
    const int* chunk_e0;        // [nchunk] first edge id of the chunk
    const int* chunk_n;         // [nchunk] edges in the chunk (1 .. 64)
    const int* kf_chunk0;       // [K + 1] first chunk of every keyframe
    const int* pt_edge;         // [E] edge ids grouped by point (LbaProblem::pt_start), ascending inside a point
    // Schur tiles: tile t = points tile_p0[t] .. tile_p0[t + 1] - 1; its staged edges (those in free keyframes, point-major, ascending keyframe inside a point)
    // are stg_edge[tile_s0[t] .. tile_s0[t + 1]).  The (W_a, B_b) pairs of a block inside a tile are NOT listed: while staging, every tile point gets a bit mask of
    // the free keyframes that see it and the index of its first staged edge; a block's thread scans the masks (a point contributes iff both bits are set; the edge
    // of keyframe block a is first + popcount(mask below bit a)).  ~100 bytes of lists per point less to build on the host and to upload, per window and call.
    const int* tile_p0;         // [ntile + 1]
    const int* tile_s0;         // [ntile + 1]
    const int* stg_edge;        // [staged edges]
    const int* thr_own;         // [ngroup][kWinThreads] block | sub << 16 | split << 24 of the thread in pass g of the Schur phase, -1 = none.  Threads are dealt to the
                                // blocks in proportion to their pair counts and ordered by load, so that the lanes of a wave walk lists of similar length; a window with
                                // more blocks than threads takes several passes over the tiles (the staging is then repeated)
    const int* blk_thr;         // [nblk] offset into blk_slots | slot count << 16 of the block (0 slots: a block without pairs)
    const int* blk_slots;       // the slots (pass * kWinThreads + thread) of every block in `sub` order
    double* HsG;                // reduced system [n][n + 1] in global memory when it does not fit LDS (hs_global), factored by the matrix-core solver
    double* chunkC;             // [nchunk][27] pose-part sums
    double* pairPart;           // [ngroup * kWinThreads][42] per-slot sums of the blocks
    int nchunk, npairs, nfree, nblk, ntile, ngroup, hs_global;
    int TE, TP;                 // tile capacities (staged edges, points)
    int hs_doubles;             // packed size of the reduced system incl. rhs column
    int region_doubles;         // LDS region shared by the reduced system and the tile buffers
};

// packed upper block-triangular storage of the augmented reduced system [n][n + 1]: block row b (rows 6b .. 6b+5) keeps columns 6b .. n; A(i, k) =
// Hs[rowoff(i) + k] for k >= 6 (i / 6)
__host__ __device__ inline int win_rowoff(int i, int n) {
    const int b = i / 6, Lb = n + 1 - 6 * b;
    return 6 * (b * (n + 1) - 3 * b * (b - 1)) + (i - 6 * b) * Lb - 6 * b;
}
__host__ __device__ inline int win_hs_doubles(int nfree) {
    const int n = 6 * nfree;
    return nfree == 0 ? 8 : win_rowoff(n - 1, n) + n + 1 + 7;   // + slack
}
// persistent part of the dynamic LDS (bytes): xp, Hpp, bp, T, R, Tn, blk, free_pose, rowoff
__host__ __device__ inline size_t win_persist_bytes(int K, int nfree) {
    const size_t n = 6 * (size_t)nfree;
    const size_t d = (n + 8) + 36 * (size_t)nfree + 6 * (size_t)nfree + 7 * (size_t)K + 9 * (size_t)K + 7 * (size_t)nfree;
    const size_t ints = (size_t)K + nfree + n + 8;
    return d * 8 + ((ints * 4 + 15) & ~(size_t)15) + 64;
}
// doubles of the tile buffers: W, B [TE][18], Dinv [TP][9], bl [TP][3], keyframe mask [TP] (64 bits), first staged edge [TP] and local point of every staged
// edge [TE] (ints)
__host__ __device__ inline size_t win_tile_doubles(int TE, int TP) { return (size_t)TE * 36 + (size_t)TP * 13 + ((size_t)TE + TP + 1) / 2 + 2; }

// The pairs of block (oa, ob) among the np points of the staged tile, taken by thread `sub` of `split`: every point whose mask has both bits, in point order.
// acc += W_a B_b^T (and bsv += W_a b_l for a diagonal block).  s_pmask / s_pbase / s_W / s_B / s_bl: the tile buffers in LDS.
__device__ __forceinline__ void win_tile_pairs(int np, int oa, int ob, int sub, int split, const unsigned long long* s_pmask, const int* s_pbase, const double* s_W, const double* s_B,
                                               const double* s_bl, double acc[36], double bsv[6]) {
#pragma clang fp contract(fast)
    const bool diag = oa == ob;
    const unsigned long long below_a = (1ull << oa) - 1ull, below_b = (1ull << ob) - 1ull;
    int ord = 0;
    for (int lp0 = 0; lp0 < np; lp0 += 64) {
        // this thread's hits among 64 tile points (the masks are read at wave-uniform addresses: LDS broadcasts)
        unsigned long long hits = 0;
        const int cnt = min(64, np - lp0);
        for (int i = 0; i < cnt; i++) {
            const unsigned long long m = s_pmask[lp0 + i];
            hits |= (unsigned long long)((m >> oa) & (m >> ob) & 1ull) << i;
        }
        while (hits) {
            const int i = __builtin_ctzll(hits);
            hits &= hits - 1;
            const int k = ord++;
            if (split > 1 && k % split != sub) continue;
            const int lp = lp0 + i;
            const unsigned long long m = s_pmask[lp];
            const int base = s_pbase[lp];
            const int li = base + __builtin_popcountll(m & below_a), lj = base + __builtin_popcountll(m & below_b);
            const double* Wa = s_W + li * 18;
            const double* Bb = s_B + lj * 18;
            double BD[18], B2[18];
#pragma unroll
            for (int q = 0; q < 18; q++) { BD[q] = Wa[q]; B2[q] = Bb[q]; }
            if (diag) {
                const double* blp = s_bl + lp * 3;
                const double l0 = blp[0], l1 = blp[1], l2 = blp[2];
#pragma unroll
                for (int q = 0; q < 6; q++) bsv[q] += BD[q * 3] * l0 + BD[q * 3 + 1] * l1 + BD[q * 3 + 2] * l2;
            }
#pragma unroll
            for (int q = 0; q < 6; q++)
#pragma unroll
                for (int j = 0; j < 6; j++)
                    acc[q * 6 + j] += BD[q * 3] * B2[j * 3] + BD[q * 3 + 1] * B2[j * 3 + 1] + BD[q * 3 + 2] * B2[j * 3 + 2];
        }
    }
}

// Blocked Cholesky U^T U (6-wide panels, look-ahead on the next diagonal block) of the packed LDS system + register-resident back substitution by one wavefront;
// x (LDS or global) receives the solution, or zeros when a pivot is not positive.  Fused multiply-adds allowed: the reference factors this matrix with Eigen's
// LDLT inside g2o, a different algorithm anyway.  Called by all kWinThreads threads of the workgroup; returns the same flag to every thread.
__device__ __forceinline__ bool win_chol_packed(double* Hs, const int* rowoff, int n, double* xp) {
#pragma clang fp contract(fast)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __shared__ int s_flag;
    __shared__ double s_Dg[36], s_rinv[6];
    bool ok2 = true;
    if (tid == 0) s_flag = 1;
    auto A = [&](int i, int k) -> double& { return Hs[rowoff[i] + k]; };
    auto factor_diag = [&](int j0) {   // one wavefront, every lane redundantly
        double Dg[36], rinv[6];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int k = 0; k < 6; k++) Dg[i * 6 + k] = k >= i ? A(j0 + i, j0 + k) : 0.0;
        bool good = true;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const double d = Dg[j * 6 + j];
            good = good && (d > 0) && (d < 1.7e308);
            const double r = rsqrt(d);
            rinv[j] = r;
            Dg[j * 6 + j] = d * r;
#pragma unroll
            for (int k = j + 1; k < 6; k++) Dg[j * 6 + k] *= r;
#pragma unroll
            for (int i = j + 1; i < 6; i++)
#pragma unroll
                for (int k = i; k < 6; k++) Dg[i * 6 + k] -= Dg[j * 6 + i] * Dg[j * 6 + k];
        }
        if (lane == 0) {
            if (!good) s_flag = 0;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                s_rinv[i] = rinv[i];
#pragma unroll
                for (int k = i; k < 6; k++) { s_Dg[i * 6 + k] = Dg[i * 6 + k]; A(j0 + i, j0 + k) = Dg[i * 6 + k]; }
            }
        }
    };
    auto scale_cols = [&](int j0) {   // row panel of block j0: one column (k > j0 + 5, incl. the rhs) per thread
        for (int k = j0 + 6 + tid; k <= n; k += kWinThreads) {
            double col[6];
#pragma unroll
            for (int i = 0; i < 6; i++) col[i] = A(j0 + i, k);
#pragma unroll
            for (int j = 0; j < 6; j++) {
                double sv = col[j];
#pragma unroll
                for (int i = 0; i < j; i++) sv -= s_Dg[i * 6 + j] * col[i];
                col[j] = sv * s_rinv[j];
            }
#pragma unroll
            for (int i = 0; i < 6; i++) A(j0 + i, k) = col[i];
        }
    };
    auto update_rows = [&](int j0, int i0, int kmin, int kend, auto nr_tag) {
        constexpr int NR = decltype(nr_tag)::value;
        double Pn[NR][6];
#pragma unroll
        for (int ii = 0; ii < NR; ii++)
#pragma unroll
            for (int r = 0; r < 6; r++) Pn[ii][r] = A(j0 + r, i0 + ii);
        for (int k = kmin + lane; k <= kend; k += 64) {
            double cpan[6], tv[NR];
#pragma unroll
            for (int r = 0; r < 6; r++) cpan[r] = A(j0 + r, k);
#pragma unroll
            for (int ii = 0; ii < NR; ii++) tv[ii] = A(i0 + ii, k);
#pragma unroll
            for (int ii = 0; ii < NR; ii++) {
                double sv = 0;
#pragma unroll
                for (int r = 0; r < 6; r++) sv += Pn[ii][r] * cpan[r];
                A(i0 + ii, k) = tv[ii] - sv;
            }
        }
    };
    __syncthreads();
    if (n > 0) {
    if (wv == 0) factor_diag(0);
    __syncthreads();
    scale_cols(0);
    __syncthreads();
    for (int j0 = 0; j0 + 6 < n; j0 += 6) {
        if (wv == 0) {   // look-ahead: the next diagonal block is updated and factored while the other waves apply the panel
            update_rows(j0, j0 + 6, j0 + 6, j0 + 11, std::integral_constant<int, 6>());
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            factor_diag(j0 + 6);
        } else {
            for (int i0 = j0 + 6 + 3 * (wv - 1); i0 < n; i0 += 3 * (kWinWaves - 1)) update_rows(j0, i0, max(i0, j0 + 12), n, std::integral_constant<int, 3>());
        }
        __syncthreads();
        scale_cols(j0 + 6);
        __syncthreads();
    }
    ok2 = s_flag != 0;
    // back substitution U x = y, column oriented (x_i = y_i / U_ii, then y_k -= U_ki x_i for k < i), one wavefront
    if (wv == 0 && ok2) {
        if (n <= 192) {   // y and 1 / U_ii in registers (lane l holds entries l, l + 64, l + 128), x_i by readlane, next column prefetched
            double y0 = 0, y1 = 0, y2 = 0, r0 = 0, r1 = 0, r2 = 0;
            if (lane < n) { y0 = A(lane, n); r0 = 1.0 / A(lane, lane); }
            if (lane + 64 < n) { y1 = A(lane + 64, n); r1 = 1.0 / A(lane + 64, lane + 64); }
            if (lane + 128 < n) { y2 = A(lane + 128, n); r2 = 1.0 / A(lane + 128, lane + 128); }
            auto bcast = [&](double v, int src) -> double {
                const unsigned long long u = (unsigned long long)__double_as_longlong(v);
                const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)u, src), hi = __builtin_amdgcn_readlane((int)(unsigned)(u >> 32), src);
                return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
            };
            const int row0 = min(lane, n - 1), row1 = min(lane + 64, n - 1), row2 = min(lane + 128, n - 1);
            const int o0 = rowoff[row0], o1 = rowoff[row1], o2 = rowoff[row2];
            double v0 = Hs[o0 + n - 1], v1 = Hs[o1 + n - 1], v2 = Hs[o2 + n - 1];
            auto run = [&](auto seg_tag, int ihi, int ilo) {
                constexpr int SG = decltype(seg_tag)::value;
                for (int i = ihi; i >= ilo; i--) {
                    const int inext = i > 0 ? i - 1 : 0;
                    const double w0 = Hs[o0 + inext];
                    double w1 = 0, w2 = 0;
                    if (SG >= 1) w1 = Hs[o1 + inext];
                    if (SG >= 2) w2 = Hs[o2 + inext];
                    const int src = i & 63;
                    const double xi = bcast(SG == 0 ? y0 : SG == 1 ? y1 : y2, src) * bcast(SG == 0 ? r0 : SG == 1 ? r1 : r2, src);
                    y0 -= (lane < i ? v0 : 0.0) * xi;
                    if (SG >= 1) y1 -= (lane + 64 < i ? v1 : 0.0) * xi;
                    if (SG >= 2) y2 -= (lane + 128 < i ? v2 : 0.0) * xi;
                    if (SG == 0) y0 = lane == src ? xi : y0;
                    if (SG == 1) y1 = lane == src ? xi : y1;
                    if (SG == 2) y2 = lane == src ? xi : y2;
                    v0 = w0; v1 = w1; v2 = w2;
                }
            };
            if (n > 128) run(std::integral_constant<int, 2>(), n - 1, 128);
            if (n > 64) run(std::integral_constant<int, 1>(), min(n - 1, 127), 64);
            if (n > 0) run(std::integral_constant<int, 0>(), min(n - 1, 63), 0);
            if (lane < n) xp[lane] = y0;
            if (lane + 64 < n) xp[lane + 64] = y1;
            if (lane + 128 < n) xp[lane + 128] = y2;
        } else {
            for (int i = lane; i < n; i += 64) xp[i] = A(i, n);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int i = n - 1; i >= 0; i--) {
                const double xi = xp[i] / A(i, i);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (int k = lane; k < i; k += 64) xp[k] -= A(k, i) * xi;
                if (lane == 0) xp[i] = xi;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    }
    if (!ok2) for (int i = tid; i < n; i += kWinThreads) xp[i] = 0;
    __syncthreads();
    return ok2;
}

__global__ __launch_bounds__(kWinThreads) void k_lba_win(const LbaProblem* probs, const LbaWin* wins, const int* order) {
    // The products J^T W J, B (Hll + lambda I)^-1, W B^T and the dense solve may use fused multiply-adds (the rest of the library is built
    // -ffp-contract=off): they feed normal equations whose solution is compared at 1e-4, and this kernel evaluates them several times per LM trial.  The
    // residuals, the robust kernel and the chi2 tests (se3_math.h: se3_map, edge_error, huber) and the LM control below keep one IEEE operation per operator.
#pragma clang fp contract(fast)
    const int wi = order[blockIdx.x];
    const LbaProblem& pr = probs[wi];
    const LbaWin& w = wins[wi];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int K = pr.K, P = pr.P, E = pr.E;
    const int nfree = w.nfree, n = 6 * nfree;
    extern __shared__ __align__(16) uint8_t dyn[];
    double* Hs = (double*)dyn;                       // region: the reduced system, or the tile buffers of the Schur phase
    double* s_W = Hs;                                //   [TE][18]
    double* s_B = s_W + (size_t)w.TE * 18;           //   [TE][18]
    double* s_Dinv = s_B + (size_t)w.TE * 18;        //   [TP][9]
    double* s_bl = s_Dinv + (size_t)w.TP * 9;        //   [TP][3]
    unsigned long long* s_pmask = (unsigned long long*)(s_bl + (size_t)w.TP * 3);   //   [TP] free keyframes (block indices) that see the tile point
    int* s_pbase = (int*)(s_pmask + w.TP);           //   [TP] first staged edge of the tile point
    int* s_ptl = s_pbase + w.TP;                     //   [TE] local point of a staged edge
    double* xp = Hs + w.region_doubles;
    double* Hpp = xp + n + 8;
    double* bp = Hpp + 36 * nfree;
    SE3* T = (SE3*)(bp + 6 * nfree);
    double* R = (double*)(T + K);
    SE3* Tn = (SE3*)(R + 9 * K);
    int* blk = (int*)(Tn + nfree);
    int* free_pose = blk + K;
    int* rowoff = free_pose + nfree;
    __shared__ double s_red[2][kWinWaves][2];
    __shared__ int s_stop;
    int phase = 0;
#ifdef OSLAM_LBA_PROFILE
    long long prof_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long tlast_ = wall_clock64();
#define WIN_STAMP(i) do { if (tid == 0) { const long long t__ = wall_clock64(); prof_[i] += t__ - tlast_; tlast_ = t__; } } while (0)
#else
#define WIN_STAMP(i) do { } while (0)
#endif

    const Cam cam = {(double)pr.K5[0], (double)pr.K5[1], (double)pr.K5[2], (double)pr.K5[3], (double)pr.K5[4]};
    const double dMono = (double)pr.delta_mono, dStereo = (double)pr.delta_stereo;

    // block-wide sum / max of two values in a fixed order; every thread gets the same result
    auto red2 = [&](double& a, double& b, bool is_max) {
        const double ra = is_max ? wmax(a) : wsum(a), rb = is_max ? wmax(b) : wsum(b);
        if (lane == 0) { s_red[phase][wv][0] = ra; s_red[phase][wv][1] = rb; }
        __syncthreads();
        double sa = s_red[phase][0][0], sb = s_red[phase][0][1];
        for (int q = 1; q < kWinWaves; q++) {
            if (is_max) { sa = fmax(sa, s_red[phase][q][0]); sb = fmax(sb, s_red[phase][q][1]); }
            else { sa += s_red[phase][q][0]; sb += s_red[phase][q][1]; }
        }
        a = sa; b = sb;
        phase ^= 1;
    };

    // ---- setup ----
    if (tid == 0) {
        int nb = 0;
        for (int a = 0; a < K; a++) {
            if (pr.fixed[a]) blk[a] = -1;
            else { free_pose[nb] = a; blk[a] = nb++; }
        }
    }
    for (int a = tid; a < K; a += kWinThreads) {
        T[a] = se3_from_T(pr.poses + a * 16);
        se3_R(T[a], R + 9 * a);
    }
    for (int i = tid; i < n; i += kWinThreads) rowoff[i] = win_rowoff(i, n);
    for (int i = tid; i < P * 3; i += kWinThreads) pr.Xa[i] = (double)pr.points[i];
    for (int e = tid; e < E; e += kWinThreads) { pr.level[e] = 0; pr.chi2[e] = 0; pr.erase[e] = 0; }
    __syncthreads();

    double* X = pr.Xa;    // current points
    double* Xn = pr.Xb;   // trial points
    int st_its0 = 0, st_its1 = 0, st_trials0 = 0, st_trials1 = 0;
    auto stopped = [&]() -> bool {   // g2o setForceStopFlag: one lane polls, the workgroup agrees
        if (!pr.stop) return false;
        __syncthreads();
        if (tid == 0) s_stop = *pr.stop;
        __syncthreads();
        return s_stop != 0;
    };
    const bool early = stopped();   // reference :655-657
    bool robust = pr.robust0 != 0;

    // trial / current pose of keyframe a
    auto pose_of = [&](int a, bool trial) -> const SE3& { const int ba = blk[a]; return (trial && ba >= 0) ? Tn[ba] : T[a]; };

    // Residual and Jacobians of edge e (keyframe a, at the CURRENT poses / points): er, the pose / point Jacobians, info and the robust weight.
    // Inlined at every use: what a caller does not read is not computed.
    auto edge_lin = [&](int e, int a, double* er, double* Jp, double* Jx, double& info, double& wgt, double& c2, bool& stereo) {
        const int p = pr.e_pt[e];
        const double Xw[3] = {X[p * 3], X[p * 3 + 1], X[p * 3 + 2]};
        const float ur = pr.e_obs[e * 3 + 2];
        stereo = !(ur < 0);
        const double ob[3] = {(double)pr.e_obs[e * 3], (double)pr.e_obs[e * 3 + 1], (double)ur};
        info = (double)pr.e_info[e];
        double pc[3];
        se3_map(T[a], Xw, pc);
        c2 = edge_error(cam, pc, ob, stereo, info, er);
        double r0 = c2;
        wgt = 1.0;
        if (robust) huber(c2, stereo ? dStereo : dMono, r0, wgt);
        jac_binary_rcp(cam, pc, R + 9 * a, stereo, Jp, Jx);
    };

    // chi2 of every active edge at the trial state; returns this thread's share of the (robust) sum
    auto eval_trial = [&](const double* Xp) -> double {
        double F = 0;
        for (int c = wv; c < w.nchunk; c += kWinWaves) {
            const int a = w.chunk_kf[c];
            const int e = w.chunk_e0[c] + lane;
            if (lane >= w.chunk_n[c] || pr.level[e] != 0) continue;
            const SE3& Tp = pose_of(a, true);
            const int p = pr.e_pt[e];
            const double Xw[3] = {Xp[p * 3], Xp[p * 3 + 1], Xp[p * 3 + 2]};
            const float ur = pr.e_obs[e * 3 + 2];
            const bool stereo = !(ur < 0);
            const double ob[3] = {(double)pr.e_obs[e * 3], (double)pr.e_obs[e * 3 + 1], (double)ur};
            double pc[3], er[3];
            se3_map(Tp, Xw, pc);
            const double c2 = edge_error(cam, pc, ob, stereo, (double)pr.e_info[e], er);
            pr.chi2[e] = c2;
            if (robust) { double r0, r1; huber(c2, stereo ? dStereo : dMono, r0, r1); F += r0; }
            else F += c2;
        }
        return F;
    };

    // contiguous run of chunks of every wave (so that a wave meets the chunks of a keyframe one after the other and sums them in registers)
    const int cpw = (w.nchunk + kWinWaves - 1) / kWinWaves;
    const int c_lo = min(w.nchunk, wv * cpw), c_hi = min(w.nchunk, c_lo + cpw);

    for (int stage = 0; stage < pr.nstages && !early; stage++) {
        const int iters = stage == 0 ? pr.iters0 : pr.iters1;
        double lambda = 0, ni = 2;
        bool ok = true;
        for (int iter = 0; iter < iters && !stopped() && ok; iter++) {
            // ================= linearisation, pose part: keyframe-major chunks =================
            double F0 = 0;
            WIN_STAMP(6);
            {
                double C[27];
#pragma unroll
                for (int k = 0; k < 27; k++) C[k] = 0;
                int seg0 = c_lo;   // first chunk of the current run of one keyframe
                for (int c = c_lo; c < c_hi; c++) {
                    const int a = w.chunk_kf[c];
                    const int ba = blk[a];
                    const int e = w.chunk_e0[c] + lane;
                    if (lane < w.chunk_n[c] && pr.level[e] == 0) {
                        double er[3], Jp[18], Jx[9], info, wgt, c2;
                        bool stereo;
                        edge_lin(e, a, er, Jp, Jx, info, wgt, c2, stereo);
                        pr.chi2[e] = c2;
                        double r0 = c2, r1;
                        if (robust) huber(c2, stereo ? dStereo : dMono, r0, r1);
                        F0 += r0;
                        if (ba >= 0) {
                            const double wi_ = wgt * info;
                            // mono edges carry a zero third row (J, e): the 3-row loops add exact zeros
                            int k = 0;
#pragma unroll
                            for (int i = 0; i < 6; i++) {
                                double sb = 0;
                                _Pragma("unroll") for (int d = 0; d < 3; d++) sb += Jp[d * 6 + i] * (info * er[d]);
                                C[21 + i] -= wgt * sb;
#pragma unroll
                                for (int j = i; j < 6; j++) {
                                    double sh = 0;
                                    _Pragma("unroll") for (int d = 0; d < 3; d++) sh += Jp[d * 6 + i] * wi_ * Jp[d * 6 + j];
                                    C[k++] += sh;
                                }
                            }
                        }
                    }
                    const bool last = c + 1 == c_hi || w.chunk_kf[c + 1] != a;   // wave-uniform
                    if (last) {
                        if (ba >= 0) {   // the run's 27 sums: lane k keeps sum k; the run's first chunk slot takes them, its other slots are zero
                            double mine = 0;
#pragma unroll
                            for (int k = 0; k < 27; k++) { const double sv = wsum(C[k]); mine = lane == k ? sv : mine; C[k] = 0; }
                            if (lane < 27) {
                                w.chunkC[(long long)seg0 * 27 + lane] = mine;
                                for (int c2 = seg0 + 1; c2 <= c; c2++) w.chunkC[(long long)c2 * 27 + lane] = 0;
                            }
                        }
                        seg0 = c + 1;
                    }
                }
            }
            // ================= linearisation, point part: one thread per point, its edges in order =================
            double m1 = 0;
            for (int p = tid; p < P; p += kWinThreads) {
                double hl[6] = {0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0};
                for (int q = pr.pt_start[p]; q < pr.pt_start[p + 1]; q++) {
                    const int e = w.pt_edge[q];
                    if (pr.level[e] != 0) continue;
                    double er[3], Jp[18], Jx[9], info, wgt, c2;
                    bool stereo;
                    edge_lin(e, pr.e_kf[e], er, Jp, Jx, info, wgt, c2, stereo);
                    const double wi_ = wgt * info;
                    int k = 0;
#pragma unroll
                    for (int i = 0; i < 3; i++) {
                        double sb = 0;
                        _Pragma("unroll") for (int d = 0; d < 3; d++) sb += Jx[d * 3 + i] * (info * er[d]);
                        bl[i] -= wgt * sb;
#pragma unroll
                        for (int j = i; j < 3; j++) {
                            double sh = 0;
                            _Pragma("unroll") for (int d = 0; d < 3; d++) sh += Jx[d * 3 + i] * wi_ * Jx[d * 3 + j];
                            hl[k++] += sh;
                        }
                    }
                }
                double* H = pr.Hll + (long long)p * 9;
                H[0] = hl[0]; H[1] = hl[1]; H[2] = hl[2]; H[3] = hl[1]; H[4] = hl[3]; H[5] = hl[4]; H[6] = hl[2]; H[7] = hl[4]; H[8] = hl[5];
                pr.bl[p * 3] = bl[0]; pr.bl[p * 3 + 1] = bl[1]; pr.bl[p * 3 + 2] = bl[2];
                m1 = fmax(m1, fmax(fabs(hl[0]), fmax(fabs(hl[3]), fabs(hl[5]))));
            }
            __syncthreads();
            WIN_STAMP(0);
            // pose blocks: chunk slots in chunk order (upper triangle + rhs -> full 6x6 and b_p in LDS)
            for (int it = tid; it < nfree * 27; it += kWinThreads) {
                const int ba = it / 27, k = it - ba * 27;
                const int a = free_pose[ba];
                double sv = 0;
                for (int c = w.kf_chunk0[a]; c < w.kf_chunk0[a + 1]; c++) sv += w.chunkC[(long long)c * 27 + k];
                if (k >= 21) bp[ba * 6 + (k - 21)] = sv;
                else {
                    int i = 0, rem = k;
                    while (rem >= 6 - i) { rem -= 6 - i; i++; }
                    const int j = i + rem;
                    Hpp[ba * 36 + i * 6 + j] = sv; Hpp[ba * 36 + j * 6 + i] = sv;
                }
            }
            double dummy = 0;
            red2(F0, dummy, false);     // (barrier inside: Hpp / bp are complete for everybody)
            double currentChi = F0;
            if (iter == 0) {   // computeLambdaInit over pose and point diagonals
                double m2 = 0;
                for (int it = tid; it < nfree * 6; it += kWinThreads) m2 = fmax(m2, fabs(Hpp[(it / 6) * 36 + (it % 6) * 7]));
                red2(m1, m2, true);
                lambda = 1e-5 * fmax(m1, m2);
                ni = 2;
            }

            double rho = 0;
            int qmax = 0;
            WIN_STAMP(1);
            do {
                // ================= Schur complement on chip: tiles of points, one thread (or `split` threads) per 6x6 block =================
                for (int grp = 0; grp < w.ngroup; grp++) {
                    const int own = w.thr_own[grp * kWinThreads + tid];
                    const bool owner = own >= 0;
                    const int tb = own & 0xFFFF, sub = (own >> 16) & 0xFF, split = owner ? (own >> 24) & 0xFF : 1;
                    int oa = 0, ob = 0;
                    if (owner) { int rem = tb; while (rem >= nfree - oa) { rem -= nfree - oa; oa++; } ob = oa + rem; }
                    double acc[36], bsv[6];
#pragma unroll
                    for (int i = 0; i < 36; i++) acc[i] = 0;
#pragma unroll
                    for (int i = 0; i < 6; i++) bsv[i] = 0;
                    for (int t = 0; t < w.ntile; t++) {
                        const int p0 = w.tile_p0[t], np = w.tile_p0[t + 1] - p0;
                        const int s0 = w.tile_s0[t], ns = w.tile_s0[t + 1] - s0;
                        // (1) (Hll + lambda I)^-1 and b_l of the tile's points
                        for (int lp = tid; lp < np; lp += kWinThreads) {
                            const int p = p0 + lp;
                            s_pmask[lp] = 0;
                            double D[9], Di[9];
                            const double* H = pr.Hll + (long long)p * 9;
#pragma unroll
                            for (int i = 0; i < 9; i++) D[i] = H[i];
                            D[0] += lambda; D[4] += lambda; D[8] += lambda;
                            inv3(D, Di);
#pragma unroll
                            for (int i = 0; i < 9; i++) s_Dinv[lp * 9 + i] = Di[i];
#pragma unroll
                            for (int i = 0; i < 3; i++) s_bl[lp * 3 + i] = pr.bl[p * 3 + i];
                        }
                        __syncthreads();
                        // (2) B_e and W_e = B_e (Hll + lambda I)^-1 of the tile's edges in free keyframes
                        for (int l = tid; l < ns; l += kWinThreads) {
                            const int e = w.stg_edge[s0 + l];
                            double* Bo = s_B + l * 18;
                            double* Wo = s_W + l * 18;
                            const int lp = pr.e_pt[e] - p0;
                            s_ptl[l] = lp;
                            atomicOr(&s_pmask[lp], 1ull << blk[pr.e_kf[e]]);   // (integer: the result does not depend on the order)
                            if (l == 0 || pr.e_pt[w.stg_edge[s0 + l - 1]] - p0 != lp) s_pbase[lp] = l;
                            if (pr.level[e] != 0) {
#pragma unroll
                                for (int i = 0; i < 18; i++) { Bo[i] = 0; Wo[i] = 0; }
                                continue;
                            }
                            double er[3], Jp[18], Jx[9], info, wgt, c2;
                            bool stereo;
                            edge_lin(e, pr.e_kf[e], er, Jp, Jx, info, wgt, c2, stereo);
                            const double wi_ = wgt * info;
                            const double* Di = s_Dinv + lp * 9;
#pragma unroll
                            for (int i = 0; i < 6; i++) {
                                double b3[3];
#pragma unroll
                                for (int j = 0; j < 3; j++) {
                                    double sh = 0;
                                    _Pragma("unroll") for (int d = 0; d < 3; d++) sh += Jp[d * 6 + i] * wi_ * Jx[d * 3 + j];
                                    b3[j] = sh;
                                    Bo[i * 3 + j] = sh;
                                }
                                Wo[i * 3] = b3[0] * Di[0] + b3[1] * Di[3] + b3[2] * Di[6];
                                Wo[i * 3 + 1] = b3[0] * Di[1] + b3[1] * Di[4] + b3[2] * Di[7];
                                Wo[i * 3 + 2] = b3[0] * Di[2] + b3[1] * Di[5] + b3[2] * Di[8];
                            }
                        }
                        __syncthreads();
                        WIN_STAMP(2);
                        // (3) the tile's pairs of this thread's block
                        if (owner) win_tile_pairs(np, oa, ob, sub, split, s_pmask, s_pbase, s_W, s_B, s_bl, acc, bsv);
                        __syncthreads();   // the tile buffers are free again
                        WIN_STAMP(7);
                    }
                    // the blocks' sums: per-slot sums through memory
                    if (owner) {
                        double* o = w.pairPart + (long long)(grp * kWinThreads + tid) * 42;
#pragma unroll
                        for (int i = 0; i < 36; i++) o[i] = acc[i];
#pragma unroll
                        for (int i = 0; i < 6; i++) o[36 + i] = bsv[i];
                    }
                }
                {
                    // reduced system (LDS, packed; or global, full) = diag(Hpp + lambda I), rhs b_p, minus the blocks' sums added in slot order
                    const int ldg = n + 1;
                    if (w.hs_global) { for (long long i = tid; i < (long long)n * ldg; i += kWinThreads) w.HsG[i] = 0; }
                    else for (int i = tid; i < w.hs_doubles; i += kWinThreads) Hs[i] = 0;
                    __syncthreads();
                    for (int it = tid; it < w.nblk * 42; it += kWinThreads) {
                        const int t = it / 42, k = it - t * 42;
                        int ba = 0, rem = t;
                        while (rem >= nfree - ba) { rem -= nfree - ba; ba++; }
                        const int bb = ba + rem;
                        if (k >= 36 && ba != bb) continue;
                        double sv = 0;
                        const int bt = w.blk_thr[t], t0 = bt & 0xFFFF, tn = bt >> 16;
                        for (int s2 = 0; s2 < tn; s2++) sv += w.pairPart[(long long)w.blk_slots[t0 + s2] * 42 + k];
                        if (k < 36) {
                            const int i = k / 6, j = k - i * 6;
                            double v = -sv;
                            if (ba == bb) v += Hpp[ba * 36 + k] + (i == j ? lambda : 0.0);
                            if (w.hs_global) w.HsG[(long long)(6 * ba + i) * ldg + 6 * bb + j] = v;
                            else Hs[rowoff[6 * ba + i] + 6 * bb + j] = v;
                        } else {
                            const double v = bp[ba * 6 + (k - 36)] - sv;
                            if (w.hs_global) w.HsG[(long long)(6 * ba + (k - 36)) * ldg + n] = v;
                            else Hs[rowoff[6 * ba + (k - 36)] + n] = v;
                        }
                    }
                    __syncthreads();
                }
                WIN_STAMP(3);
                // ================= blocked Cholesky U^T U in LDS (fused multiply-adds allowed: the reference factors this matrix with Eigen's LDLT) =================
                bool ok2 = true;
                if (w.hs_global) {   // the system is in global memory (L2): matrix-core Cholesky (16-wide panels through LDS, v_mfma_f64_16x16x4_f64 trailing updates)
                    const int pw = ((n + 1 + kMB - 1) / kMB + 1) * kMB;
                    ok2 = chol_mfma_dev(w.HsG, n, xp, Hs, Hs + (size_t)kMB * pw);
                } else ok2 = win_chol_packed(Hs, rowoff, n, xp);
                WIN_STAMP(4);
                // ================= landmarks: x_l = (Hll + lambda I)^-1 (b_l - sum_a B_a^T x_a), B_a^T x_a = J_x^T W (J_p x_a); trial state =================
                double sc = 0;
                for (int p = tid; p < P; p += kWinThreads) {
                    double cl[3] = {pr.bl[p * 3], pr.bl[p * 3 + 1], pr.bl[p * 3 + 2]};
                    double xo[3] = {0, 0, 0};
                    if (ok2) {
                        for (int q = pr.pt_start[p]; q < pr.pt_start[p + 1]; q++) {
                            const int e = w.pt_edge[q];
                            if (pr.level[e] != 0) continue;
                            const int a = pr.e_kf[e];
                            const int ba = blk[a];
                            if (ba < 0) continue;
                            double er[3], Jp[18], Jx[9], info, wgt, c2;
                            bool stereo;
                            edge_lin(e, a, er, Jp, Jx, info, wgt, c2, stereo);
                            const double wi_ = wgt * info;
                            const double* xa = xp + 6 * ba;
                            // (B^T x)_j = sum_i (sum_d Jp[d][i] wi Jx[d][j]) x_i: the products in B's own order, so the rounding is that of the stored-block form
#pragma unroll
                            for (int j = 0; j < 3; j++) {
                                double sv = 0;
#pragma unroll
                                for (int i = 0; i < 6; i++) {
                                    double sh = 0;
                                    _Pragma("unroll") for (int d = 0; d < 3; d++) sh += Jp[d * 6 + i] * wi_ * Jx[d * 3 + j];
                                    sv += sh * xa[i];
                                }
                                cl[j] -= sv;
                            }
                        }
                        double D[9], Di[9];
                        const double* H = pr.Hll + (long long)p * 9;
#pragma unroll
                        for (int i = 0; i < 9; i++) D[i] = H[i];
                        D[0] += lambda; D[4] += lambda; D[8] += lambda;
                        inv3(D, Di);
#pragma unroll
                        for (int i = 0; i < 3; i++) xo[i] = Di[i * 3] * cl[0] + Di[i * 3 + 1] * cl[1] + Di[i * 3 + 2] * cl[2];
                    }
#pragma unroll
                    for (int i = 0; i < 3; i++) {
                        Xn[p * 3 + i] = X[p * 3 + i] + xo[i];
                        sc += xo[i] * (lambda * xo[i] + pr.bl[p * 3 + i]);   // computeScale, landmark part
                    }
                }
                for (int ba = tid; ba < nfree; ba += kWinThreads) {
                    double xa[6];
                    for (int i = 0; i < 6; i++) { xa[i] = xp[6 * ba + i]; sc += xa[i] * (lambda * xa[i] + bp[ba * 6 + i]); }
                    Tn[ba] = se3_mul(se3_exp(xa), T[free_pose[ba]]);
                }
                __syncthreads();
                WIN_STAMP(5);
                double F1 = eval_trial(Xn);
                red2(F1, sc, false);
                {
#pragma clang fp contract(off)
                double tempChi = F1;
                if (!ok2) tempChi = 1.7976931348623157e308;
                rho = (currentChi - tempChi) / (sc + 1e-3);
                const bool finite = (tempChi - tempChi) == 0;
                if (rho > 0 && finite) {
                    double alpha = 1. - (2 * rho - 1) * (2 * rho - 1) * (2 * rho - 1);
                    alpha = fmin(alpha, 2. / 3.);
                    lambda *= fmax(1. / 3., alpha);
                    ni = 2;
                    currentChi = tempChi;
                    for (int ba = tid; ba < nfree; ba += kWinThreads) { const int a = free_pose[ba]; T[a] = Tn[ba]; se3_R(T[a], R + 9 * a); }
                    { double* t_ = X; X = Xn; Xn = t_; }
                } else {
                    lambda *= ni;
                    ni *= 2;
                }
                }
                __syncthreads();
                WIN_STAMP(6);
                qmax++;
                if (stage == 0) st_trials0++; else st_trials1++;
            } while (rho < 0 && qmax < 10 && !stopped());
            if (stage == 0) st_its0++; else st_its1++;
            if (qmax == 10 || rho == 0) ok = false;
        }
        if (stage == 0 && pr.nstages > 1) {
            if (stopped()) break;   // bDoMore = false (:664-666)
            // gate observations, drop the robust kernel (:672-702)
            for (int e = tid; e < E; e += kWinThreads) {
                const int a = pr.e_kf[e], p = pr.e_pt[e];
                const bool stereo = !(pr.e_obs[e * 3 + 2] < 0);
                const double Xw[3] = {X[p * 3], X[p * 3 + 1], X[p * 3 + 2]};
                double pc[3];
                se3_map(T[a], Xw, pc);
                if (pr.chi2[e] > (stereo ? 7.815 : 5.991) || !(pc[2] > 0.0)) pr.level[e] = 1;
            }
            robust = false;
            __syncthreads();
        }
    }
    __syncthreads();
    // ---- outputs (:711-777) ----
    if (!early) {
        for (int e = tid; e < E; e += kWinThreads) {
            const int a = pr.e_kf[e], p = pr.e_pt[e];
            const bool stereo = !(pr.e_obs[e * 3 + 2] < 0);
            const double Xw[3] = {X[p * 3], X[p * 3 + 1], X[p * 3 + 2]};
            double pc[3];
            se3_map(T[a], Xw, pc);
            pr.erase[e] = (pr.chi2[e] > (stereo ? 7.815 : 5.991) || !(pc[2] > 0.0)) ? 1 : 0;
        }
    }
    for (int a = tid; a < K; a += kWinThreads) {
        if (pr.fixed[a] != 1 && !early) se3_to_T(T[a], pr.poses_out + a * 16);
        else for (int i = 0; i < 16; i++) pr.poses_out[a * 16 + i] = pr.poses[a * 16 + i];
    }
    for (int i = tid; i < P * 3; i += kWinThreads) pr.points_out[i] = early ? pr.points[i] : (float)X[i];
#ifdef OSLAM_LBA_PROFILE
    if (tid == 0) for (int i = 0; i < 8; i++) pr.stats[8 + i] = (int)(prof_[i] / 100);   // 100 MHz wall clock: microseconds
#endif
    if (tid == 0) { pr.stats[0] = st_its0; pr.stats[1] = st_trials0; pr.stats[2] = st_its1; pr.stats[3] = st_trials1; }
}


// ==========================================================================================================================================================
// The same on-chip Schur complement for the WIDE layout (every LM trial of all windows as whole-GPU launches): `nwg` workgroups per window share its tiles
// (workgroup g takes tiles g, g + nwg, ...), stage B_e from the stored Hpl blocks (one coalesced read per trial instead of the 288 bytes per PAIR the
// pair-gather kernel of rounds 1-4 pulled from HBM: 4-6 pairs per edge in the driver's windows) and leave per-workgroup block sums; k_w_schur_sum adds them in
// workgroup / slot order into the reduced system.  Short kernels: the windows of a call spread over the whole GPU and the other handles' kernels interleave.
// ==========================================================================================================================================================
__global__ __launch_bounds__(kWinThreads) void k_w_schur_tiles(const LbaProblem* probs, const LbaWide* ws) {
#pragma clang fp contract(fast)
    const LbaProblem& pr = probs[blockIdx.y];
    const LbaWide& w = ws[blockIdx.y];
    const LbaCtrl* ct = w.ct;
    if (ct->done) return;
    const int g = blockIdx.x;
    if (g >= w.nwg) return;
    const int tid = threadIdx.x;
    const int nfree = ct->nfree;
    const double lambda = ct->lambda;
    extern __shared__ __align__(16) uint8_t dyn[];
    double* s_W = (double*)dyn;
    double* s_B = s_W + (size_t)w.TE * 18;
    double* s_Dinv = s_B + (size_t)w.TE * 18;
    double* s_bl = s_Dinv + (size_t)w.TP * 9;
    unsigned long long* s_pmask = (unsigned long long*)(s_bl + (size_t)w.TP * 3);
    int* s_pbase = (int*)(s_pmask + w.TP);
    int* s_ptl = s_pbase + w.TP;
    for (int grp = 0; grp < w.ngroup; grp++) {
        const int own = w.thr_own[grp * kWinThreads + tid];
        const bool owner = own >= 0;
        const int tb = own & 0xFFFF, sub = (own >> 16) & 0xFF, split = owner ? (own >> 24) & 0xFF : 1;
        int oa = 0, ob = 0;
        if (owner) { int rem = tb; while (rem >= nfree - oa) { rem -= nfree - oa; oa++; } ob = oa + rem; }
        double acc[36], bsv[6];
#pragma unroll
        for (int i = 0; i < 36; i++) acc[i] = 0;
#pragma unroll
        for (int i = 0; i < 6; i++) bsv[i] = 0;
        for (int t = g; t < w.ntile; t += w.nwg) {
            const int p0 = w.tile_p0[t], np = w.tile_p0[t + 1] - p0;
            const int s0 = w.tile_s0[t], ns = w.tile_s0[t + 1] - s0;
            for (int lp = tid; lp < np; lp += kWinThreads) {
                const int p = p0 + lp;
                s_pmask[lp] = 0;
                double D[9], Di[9];
                const double* H = pr.Hll + (long long)p * 9;
#pragma unroll
                for (int i = 0; i < 9; i++) D[i] = H[i];
                D[0] += lambda; D[4] += lambda; D[8] += lambda;
                inv3(D, Di);
#pragma unroll
                for (int i = 0; i < 9; i++) s_Dinv[lp * 9 + i] = Di[i];
#pragma unroll
                for (int i = 0; i < 3; i++) s_bl[lp * 3 + i] = pr.bl[p * 3 + i];
            }
            __syncthreads();
            for (int l = tid; l < ns; l += kWinThreads) {
                const int e = w.stg_edge[s0 + l];
                double* Bo = s_B + l * 18;
                double* Wo = s_W + l * 18;
                const int lp = pr.e_pt[e] - p0;
                s_ptl[l] = lp;
                atomicOr(&s_pmask[lp], 1ull << w.blk[pr.e_kf[e]]);
                if (l == 0 || pr.e_pt[w.stg_edge[s0 + l - 1]] - p0 != lp) s_pbase[lp] = l;
                if (pr.level[e] != 0) {
#pragma unroll
                    for (int i = 0; i < 18; i++) { Bo[i] = 0; Wo[i] = 0; }
                    continue;
                }
                const double* Bg = pr.Hpl + (long long)e * 18;
                const double* Di = s_Dinv + lp * 9;
#pragma unroll
                for (int i = 0; i < 6; i++) {
                    const double b0 = Bg[i * 3], b1 = Bg[i * 3 + 1], b2 = Bg[i * 3 + 2];
                    Bo[i * 3] = b0; Bo[i * 3 + 1] = b1; Bo[i * 3 + 2] = b2;
                    Wo[i * 3] = b0 * Di[0] + b1 * Di[3] + b2 * Di[6];
                    Wo[i * 3 + 1] = b0 * Di[1] + b1 * Di[4] + b2 * Di[7];
                    Wo[i * 3 + 2] = b0 * Di[2] + b1 * Di[5] + b2 * Di[8];
                }
            }
            __syncthreads();
            if (owner) win_tile_pairs(np, oa, ob, sub, split, s_pmask, s_pbase, s_W, s_B, s_bl, acc, bsv);
            __syncthreads();
        }
        if (owner) {
            double* o = w.parts + ((long long)g * w.ngroup * kWinThreads + grp * kWinThreads + tid) * 42;
#pragma unroll
            for (int i = 0; i < 36; i++) o[i] = acc[i];
#pragma unroll
            for (int i = 0; i < 6; i++) o[36 + i] = bsv[i];
        }
    }
}

// reduced system [n][n + 1] in global memory = diag(Hpp + lambda I), rhs b_p, minus the block sums of all workgroups in (workgroup, slot) order
__global__ __launch_bounds__(256) void k_w_schur_sum(const LbaProblem* probs, const LbaWide* ws) {
    const LbaProblem& pr = probs[blockIdx.y];
    const LbaWide& w = ws[blockIdx.y];
    const LbaCtrl* ct = w.ct;
    if (ct->done) return;
    const int nfree = ct->nfree, n = ct->n, ld = n + 1;
    const int it = blockIdx.x * 256 + threadIdx.x;
    if (it >= w.nblk * 42 || nfree == 0) return;
    const double lambda = ct->lambda;
    const int t = it / 42, k = it - t * 42;
    int ba = 0, rem = t;
    while (rem >= nfree - ba) { rem -= nfree - ba; ba++; }
    const int bb = ba + rem;
    if (k >= 36 && ba != bb) return;
    const int bt = w.blk_thr[t], t0 = bt & 0xFFFF, tn = bt >> 16;
    double sv = 0;
    for (int g = 0; g < w.nwg; g++)
        for (int s2 = 0; s2 < tn; s2++) sv += w.parts[((long long)g * w.ngroup * kWinThreads + w.blk_slots[t0 + s2]) * 42 + k];
    const int a = w.free_pose[ba];
    if (k < 36) {
        const int i = k / 6, j = k - i * 6;
        double v = -sv;
        if (ba == bb) v += pr.Hpp[a * 36 + k] + (i == j ? lambda : 0.0);
        pr.Hs[(size_t)(6 * ba + i) * ld + 6 * bb + j] = v;
    } else pr.Hs[(size_t)(6 * ba + (k - 36)) * ld + n] = pr.bp[a * 6 + (k - 36)] - sv;
}

// reduced systems of 133 .. ~190 unknowns (23-31 free keyframes): the packed LDS solver of the window kernel as a kernel of the wide layout (k_w_chol<true>
// holds the full square and stops at 132; beyond ~190 the matrix cores take over in global memory)
constexpr int kCholPackedN = 192;
constexpr int kCholPackedLds = 159 * 1024;
__global__ __launch_bounds__(kWinThreads) void k_w_chol_packed(const LbaProblem* probs, const LbaWide* ws) {
    const LbaProblem& pr = probs[blockIdx.y];
    const LbaWide& w = ws[blockIdx.y];
    LbaCtrl* ct = w.ct;
    if (ct->done) return;
    const int tid = threadIdx.x;
    const int n = ct->n, ld = n + 1;
    if (n > kCholPackedN) return;   // (a larger window of the same call is factored by k_w_chol_mfma, launched right behind this kernel)
    extern __shared__ __align__(16) uint8_t dyn[];
    double* Hs = (double*)dyn;
    const int hsd = win_hs_doubles(ct->nfree);
    int* rowoff = (int*)(Hs + hsd);
    double* xs = (double*)(rowoff + ((n + 1) & ~1) + 2);
    for (int i = tid; i < n; i += kWinThreads) rowoff[i] = win_rowoff(i, n);
    __syncthreads();
    for (int i = 0; i < n; i++) {
        const int k0 = 6 * (i / 6);
        for (int k = k0 + tid; k <= n; k += kWinThreads) Hs[rowoff[i] + k] = pr.Hs[(size_t)i * ld + k];
    }
    __syncthreads();
    const bool ok2 = win_chol_packed(Hs, rowoff, n, xs);
    for (int i = tid; i < n; i += kWinThreads) pr.xp[i] = xs[i];
    if (tid == 0) ct->ok2 = ok2 ? 1 : 0;
}

// ==========================================================================================================================================================
// Reduced camera system of 133 .. 186 unknowns (23-31 free keyframes: the bench's steady-state windows) by MATRIX CORES with the system resident in LDS.
// k_w_chol_packed above needs n / 6 = 27 panels at n = 162, each a chain of two workgroup barriers, a serial 6x6 factor and LDS-bound scalar row updates
// (134 us per launch, 0.5 % of the fp64 peak: rocprofv3, profiles/r04_lba_win_prof_40windows_kernel_stats_v0.csv).  Here: right-looking blocked Cholesky
// U^T U with 16-wide panels (11 panels at n = 162); per panel the 16x16 diagonal block is factored by wavefront 0, one thread per column solves the row panel
// U12 = U11^-T A12 in registers, and the trailing update A22 -= U12^T U12 runs on v_mfma_f64_16x16x4_f64 with BOTH operands read straight from the LDS image
// (the row panel is part of it: no staging copy), a wavefront owning a strip of tiles of one tile row so that the A operand is fetched once per strip.
// The image is the upper triangle packed by 16-row blocks: block row B keeps columns 16 B .. n (column n = right-hand side); A(i, k) = Hs[off(i) + k] for
// k >= 16 (i / 16): 152 KB at n = 186.  Back substitution as in win_chol_packed (register-resident, one wavefront).
// ==========================================================================================================================================================
constexpr int kCholLdsMfmaN = 186;
__host__ __device__ inline int chol16_rowoff(int i, int n) {
    const int B = i >> 4, r = i & 15;
    return 16 * (B * (n + 1) - 8 * B * (B - 1)) + r * (n + 1 - 16 * B) - 16 * B;
}
__host__ __device__ inline int chol16_doubles(int n) {
    const int NB = (n + 15) / 16;
    return 16 * (NB * (n + 1) - 8 * NB * (NB - 1)) + 16;
}
__host__ __device__ inline size_t chol16_lds_bytes(int n) { return ((size_t)chol16_doubles(n) + (size_t)n + 16) * 8 + (((size_t)n * 4 + 15) & ~(size_t)15) + 64; }

__global__ __launch_bounds__(kWinThreads) void k_w_chol_lds_mfma(const LbaProblem* probs, const LbaWide* ws, int min_n) {
#pragma clang fp contract(fast)
    const LbaProblem& pr = probs[blockIdx.y];
    const LbaWide& w = ws[blockIdx.y];
    LbaCtrl* ct = w.ct;
    if (ct->done) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = ct->n, ld = n + 1;
    if (n > kCholLdsMfmaN || n < min_n) return;   // (other windows of the call: the smaller LDS kernel / the global-memory matrix-core kernel, launched beside this one)
    extern __shared__ __align__(16) uint8_t dyn[];
    double* Hs = (double*)dyn;
    double* xs = Hs + chol16_doubles(n);
    int* rowoff = (int*)(xs + n + 16);
    __shared__ double s_D[kMB][kMB + 1];
    __shared__ int s_ok;
#ifdef OSLAM_LBA_PROFILE
    long long tw_ = wall_clock64();
#define CL_STAMP(i) do { if (tid == 0) { const long long t_ = wall_clock64(); pr.stats[8 + (i)] += (int)(t_ - tw_); tw_ = t_; } } while (0)
    // (inside the trailing phase: stats[13] / [14] = wavefront 0's tile (0, 0) / its factor, stats[15] = the strips of wavefront 1)
    long long ts_ = 0;
#define CL_SUB_BEGIN() do { ts_ = wall_clock64(); } while (0)
#define CL_SUB_STAMP(t, i) do { if (tid == (t)) { const long long t_ = wall_clock64(); pr.stats[(i)] += (int)(t_ - ts_); ts_ = t_; } } while (0)
#else
#define CL_STAMP(i) do { } while (0)
#define CL_SUB_BEGIN() do { } while (0)
#define CL_SUB_STAMP(t, i) do { } while (0)
#endif
    for (int i = tid; i < n; i += kWinThreads) rowoff[i] = chol16_rowoff(i, n);
    if (tid == 0) s_ok = 1;
    __syncthreads();
    {   // The image, block row by block row: thread (r = tid >> 5, cl = tid & 31) copies row 16 B + r, columns 16 B + cl, + 32, ...; the loads of FOUR block rows
        // (up to 24 per thread) are requested before the first LDS store (round 4 copied row by row with one dependent round trip per 64 columns: 12 us).
        // (the source pointer in a register and every load unconditional — lanes outside the image read its first entry and never store it: as written before,
        // each of the 24 loads sat in its own branch behind a scalar reload of pr.Hs and a wait for it: found in the ISA)
        const int r = tid >> 5, cl = tid & 31, NBr = (n + 15) >> 4;
        const double* __restrict__ gH = pr.Hs;
        for (int B0 = 0; B0 < NBr; B0 += 4) {
            double v[4][6];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int B = B0 + u, i = 16 * B + r, LB = n + 1 - 16 * B;
                const bool rowok = B < NBr && i < n;
                const size_t base = rowok ? (size_t)i * ld + 16 * B : 0;
#pragma unroll
                for (int q = 0; q < 6; q++) {
                    const int c = cl + 32 * q;
                    v[u][q] = gH[(rowok && c < LB) ? base + c : 0];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int B = B0 + u, i = 16 * B + r, LB = n + 1 - 16 * B;
                if (B < NBr && i < n) {
                    const int o = rowoff[i] + 16 * B;
#pragma unroll
                    for (int q = 0; q < 6; q++) { const int c = cl + 32 * q; if (c < LB) Hs[o + c] = v[u][q]; }
                }
            }
        }
    }
    __syncthreads();
    CL_STAMP(0);
    auto A = [&](int i, int k) -> double& { return Hs[rowoff[i] + k]; };
    // Diagonal block of the panel at j0 (called by wavefront 0), in registers: lane k (mod 16) holds COLUMN k of the block (padded to 16x16 with the identity).  Step j: the pivot
    // comes from lane j by readlane, every lane scales its entry of row j, and row j's entries U(j, i) — one readlane each — update the rows below.  No
    // LDS round trip inside the 16 steps (the LDS form took 8 us per block: rocprof phase stamps).  Then V = U^-1 the same way (back substitution on the
    // identity, column k in lane k), written to LDS for the row-panel product. ----
    // (always_inline: as an out-of-line function the closure reached Hs / s_D through FLAT loads of a captured pointer — two dependent flat loads per entry with
    // a full wait each, 16 in a row before the first step of the factor: found in the ISA, tools/chol_lds_phase_prof.py: trailing phase 4.8 us per panel)
    auto factor_block = [&](int j0, int nb, int Lb, int ro_panel) __attribute__((always_inline)) {   // (chol16_aug, lba.hip: factor and inverse of the block in one pass over [A | I])
        const int hh = lane >> 5, cc = lane & 31;
        double R[8];
#pragma unroll
        for (int sI = 0; sI < 8; sI++) {
            const int i = 2 * sI + hh;
            // (branch-free: all eight LDS reads are issued before the first wait; lanes outside the block's upper triangle read the block's first entry and drop it)
            const bool in_blk = cc < kMB && i < nb && cc < nb && cc >= i;
            const double a = Hs[in_blk ? ro_panel + i * Lb + j0 + cc : ro_panel + j0];
            const double idn = ((cc < kMB ? cc : cc - kMB) == i) ? 1.0 : 0.0;
            R[sI] = in_blk ? a : idn;
        }
        const bool good = chol16_aug(R, lane);
        if (!good && lane == 0) s_ok = 0;
#pragma unroll
        for (int sI = 0; sI < 8; sI++) {
            const int i = 2 * sI + hh;
            // lanes cc >= 16 hold U^-T[i][k], k = cc - 16: V = U11^-1 (upper triangular), V[k][i] = U^-T[i][k].  It goes to s_D for this panel's row-panel product
            // and INTO THE IMAGE in place of U11 (nothing reads U11 again): the blocked back substitution multiplies by V instead of substituting through U11
            if (cc >= kMB) {
                const int k = cc - kMB;
                s_D[k][i] = R[sI];
                if (i < nb && k < nb && i >= k) Hs[ro_panel + k * Lb + j0 + i] = R[sI];
            }
        }
    };
    if (wv == 0 && n > 0) factor_block(0, min(kMB, n), n + 1, rowoff[0]);
    for (int j0 = 0; j0 < n; j0 += kMB) {
        const int nb = min(kMB, n - j0), c0 = j0 + nb, m = n - c0;   // m trailing rows; trailing columns c0 .. n (incl. the rhs)
        const int Lb = n + 1 - j0, ro_panel = rowoff[j0];            // rows j0 .. j0 + 15 are ONE 16-row block of the image: consecutive rows are Lb doubles apart
        // ---- 1. (the diagonal block of this panel was factored ahead: by the prologue or during the previous panel's trailing update) ----
        __syncthreads();
        CL_STAMP(1);
        // ---- 2. row panel U12 = U11^-T A12 = V^T A12 by MFMA, one wavefront per 16-column tile, in place (a tile's 16 rows are read before they are written) ----
        {
            const int Tp = (m + 1 + kMB - 1) / kMB;
            for (int t = wv; t < Tp; t += kWinWaves) {
                const int col = c0 + kMB * t + (lane & 15);
                const bool cv = col <= n;
                v4f64 acc = (v4f64){0.0, 0.0, 0.0, 0.0};
                // (all eight operands are requested before the first matrix instruction — unconditional loads from clamped addresses, zeroed by a select: with the
                // loads inside the conditional every MFMA waited for an LDS round trip of its own: ISA)
                double aop[kMB / 4], bop[kMB / 4];
#pragma unroll
                for (int sx = 0; sx < kMB / 4; sx++) {
                    const int kk = 4 * sx + (lane >> 4);
                    const bool on = cv && kk < nb;
                    aop[sx] = s_D[kk][lane & 15];                                            // A[i][k] = V[k][i]
                    const double b = Hs[ro_panel + (on ? kk * Lb + col : j0)];               // B[k][j] = A12[k][col]
                    bop[sx] = on ? b : 0.0;
                }
#pragma unroll
                for (int sx = 0; sx < kMB / 4; sx++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[sx], bop[sx], acc, 0, 0, 0);
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const int r = (lane >> 4) + 4 * g;
                    if (cv && r < nb) Hs[ro_panel + r * Lb + col] = acc[g];
                }
            }
        }
        __syncthreads();
        CL_STAMP(2);
        // ---- 3. trailing update by MFMA with LOOK-AHEAD.  Tile (ti, tk), ti <= tk, covers rows c0 + 16 ti .. and columns c0 + 16 tk ..  c0 is a multiple of
        // 16 whenever there is a trailing block (every panel before the last is full), so a tile row is one 16-row block of the image: offsets by arithmetic.
        // Wavefront 0 updates tile (0, 0) — the NEXT panel's diagonal block — and factors it at once (16 dependent steps + the inverse: 5 us, the longest
        // serial piece of a panel) while wavefronts 1..7 update all other tiles in strips of up to 4 tiles of one tile row (shared A operand), dealt round
        // robin.  Nobody else touches tile (0, 0) or s_D during this phase (the row panel above was the last reader of this panel's V). ----
        if (m > 0) {
            const int Tm = (m + kMB - 1) / kMB, Tc = (m + 1 + kMB - 1) / kMB;   // tile rows; tile columns incl. the rhs column
            auto strip = [&](int ti, int tfirst, int ntl) {   // tiles (ti, ti + tfirst .. ti + tfirst + ntl - 1), ntl <= 4
                const int Bi = (c0 >> 4) + ti;                                   // 16-row block of this tile row
                const int LB = n + 1 - 16 * Bi;
                const int ro_row = 16 * (Bi * (n + 1) - 8 * Bi * (Bi - 1)) - 16 * Bi;   // chol16_rowoff(16 Bi, n)
                const int i_col = c0 + kMB * ti + (lane & 15);      // the column of U12 this lane feeds as A operand = a ROW index of the trailing block
                double aop[kMB / 4];
#pragma unroll
                for (int sx = 0; sx < kMB / 4; sx++) aop[sx] = i_col < n ? Hs[ro_panel + (4 * sx + (lane >> 4)) * Lb + i_col] : 0.0;   // (a panel with a trailing block is full: 16 rows)
                v4f64 acc[4];
                int kcol[4];
                double cin[4][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    acc[u] = (v4f64){0.0, 0.0, 0.0, 0.0};
                    kcol[u] = c0 + kMB * (ti + tfirst + u) + (lane & 15);   // this lane's column in tile u
                }
                // The B operands of ALL the strip's tiles are requested before the first matrix instruction, unconditionally (a column past the right-hand side reads
                // the right-hand side: its products land in columns that are never stored).  With the load inside the conditional every one of the 16 MFMAs of a strip
                // waited for an LDS round trip of its own (ISA; tools/chol_lds_phase_prof.py: 1.4 us per tile and wavefront).
                double bop[kMB / 4][4];
#pragma unroll
                for (int sx = 0; sx < kMB / 4; sx++) {
                    const int ro = ro_panel + (4 * sx + (lane >> 4)) * Lb;
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        if (u < ntl) bop[sx][u] = Hs[ro + min(kcol[u], n)];   // (wave-uniform)
                }
                // C / D layout of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 g; the C values are requested before the MFMAs run
#pragma unroll
                for (int u = 0; u < 4; u++)
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        const int rr = (lane >> 4) + 4 * g;
                        if (u < ntl) cin[u][g] = Hs[ro_row + rr * LB + min(kcol[u], n)];
                    }
#pragma unroll
                for (int sx = 0; sx < kMB / 4; sx++) {
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        if (u < ntl) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[sx], bop[sx][u], acc[u], 0, 0, 0);   // (wave-uniform)
                }
                // (every difference is in a register before the first store: the stores sit in branches, and a C value that arrived behind an earlier store made the
                // compiler wait for ALL outstanding LDS operations — the previous store included — in front of every single one of them: ISA)
                double dif[4][4];
#pragma unroll
                for (int u = 0; u < 4; u++)
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        dif[u][g] = u < ntl ? cin[u][g] - acc[u][g] : 0.0;
                        asm volatile("" : "+v"(dif[u][g]));
                    }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (u >= ntl || kcol[u] > n) continue;
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        const int rr = (lane >> 4) + 4 * g;
                        if (c0 + kMB * ti + rr < n) Hs[ro_row + rr * LB + kcol[u]] = dif[u][g];
                    }
                }
            };
            // A strip whose four tiles lie inside the image (no partial last tile column, no partial last tile row) needs no clamps and no guards: three lane bases,
            // the tile / row-group steps as constant or per-panel offsets.  The general form above spends ~800 instructions per strip, mostly address arithmetic
            // and exec-mask bookkeeping, for 16 matrix instructions (ISA; 2.35 us per strip: tools/chol_lds_phase_prof.py).
            auto strip_full = [&](int ti, int tfirst) __attribute__((always_inline)) {
                const int Bi = (c0 >> 4) + ti;
                const int LB = n + 1 - 16 * Bi;
                const int ro_row = 16 * (Bi * (n + 1) - 8 * Bi * (Bi - 1)) - 16 * Bi;
                const int lq = lane >> 4, ll = lane & 15;
                const double* pa = Hs + (ro_panel + lq * Lb + c0 + kMB * ti + ll);               // A operand (+ 4 sx Lb)
                const double* pb = Hs + (ro_panel + lq * Lb + c0 + kMB * (ti + tfirst) + ll);    // B operands (+ 4 sx Lb + 16 u)
                double* pc = Hs + (ro_row + lq * LB + c0 + kMB * (ti + tfirst) + ll);            // C tiles (+ 4 g LB + 16 u)
                double aop[kMB / 4], bop[kMB / 4][4], cin[4][4];
#pragma unroll
                for (int sx = 0; sx < kMB / 4; sx++) aop[sx] = pa[4 * sx * Lb];
#pragma unroll
                for (int sx = 0; sx < kMB / 4; sx++)
#pragma unroll
                    for (int u = 0; u < 4; u++) bop[sx][u] = pb[4 * sx * Lb + kMB * u];
#pragma unroll
                for (int u = 0; u < 4; u++)
#pragma unroll
                    for (int g = 0; g < 4; g++) cin[u][g] = pc[4 * g * LB + kMB * u];
                v4f64 acc[4];
#pragma unroll
                for (int u = 0; u < 4; u++) acc[u] = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int sx = 0; sx < kMB / 4; sx++)
#pragma unroll
                    for (int u = 0; u < 4; u++) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[sx], bop[sx][u], acc[u], 0, 0, 0);
#pragma unroll
                for (int u = 0; u < 4; u++)
#pragma unroll
                    for (int g = 0; g < 4; g++) pc[4 * g * LB + kMB * u] = cin[u][g] - acc[u][g];
            };
            if (wv == 0) {
                CL_SUB_BEGIN();
                strip(0, 0, 1);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                CL_SUB_STAMP(0, 13);
                __builtin_amdgcn_s_setprio(3);   // the panel's critical path: ahead of the SIMD's other wavefront (which is in the MFMA strips)
                factor_block(c0, min(kMB, n - c0), n + 1 - c0, rowoff[c0]);
                __builtin_amdgcn_s_setprio(0);
                CL_SUB_STAMP(0, 14);
            } else {
                CL_SUB_BEGIN();
                int sidx = 0;
                for (int ti = 0; ti < Tm; ti++) {
                    const int ntile_row = Tc - ti, t_begin = ti == 0 ? 1 : 0;   // (tile (0, 0) is wavefront 0's)
                    for (int t0 = t_begin; t0 < ntile_row; t0 += 4, sidx++) {
                        if (sidx % (kWinWaves - 1) != wv - 1) continue;
                        const int ntl = min(4, ntile_row - t0);
                        if (ntl == 4 && c0 + kMB * (ti + t0 + 3) + kMB - 1 <= n && c0 + kMB * ti + kMB - 1 < n) strip_full(ti, t0);
                        else strip(ti, t0, ntl);
                    }
                }
                CL_SUB_STAMP(64, 15);
            }
        }
        __syncthreads();
        CL_STAMP(3);
    }
    const bool ok2 = s_ok != 0;
    // ---- back substitution U x = y (y = column n of the image), blocked (round 5): the diagonal blocks of the image hold V_B = U_BB^-1, so for B = last .. 0:
    // x_B = V_B y_B (16 dot products, one wavefront), then y_r -= U(r, block B) x_B for the rows above (one thread per row, 16 multiply-adds).  Two workgroup
    // barriers per 16 unknowns; the round-4 form (one wavefront, one unknown per step: 156 dependent steps) took 14 us at n = 156. ----
    if (ok2 && n > 0) {
        for (int i = tid; i < n; i += kWinThreads) xs[i] = A(i, n);
        __syncthreads();
        for (int B = ((n + 15) >> 4) - 1; B >= 0; B--) {
            const int j0 = 16 * B, nb = min(kMB, n - j0), LB = n + 1 - j0, ro = rowoff[j0];
            if (wv == 0) {
                double acc = 0;
                if (lane < nb) {   // V[lane][k], k >= lane (the block's entries below the diagonal are not V: masked); all 32 LDS reads in flight
                    double vr[kMB], yk[kMB];
#pragma unroll
                    for (int k = 0; k < kMB; k++) {
                        const bool on = k >= lane && k < nb;
                        vr[k] = on ? Hs[ro + lane * LB + j0 + k] : 0.0;
                        yk[k] = on ? xs[j0 + k] : 0.0;
                    }
#pragma unroll
                    for (int k = 0; k < kMB; k++) acc += vr[k] * yk[k];
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();   // (every lane has read y_B)
                if (lane < nb) xs[j0 + lane] = acc;
            }
            __syncthreads();
            for (int r = tid; r < j0; r += kWinThreads) {
                const int o = rowoff[r] + j0;
                double ur[kMB], xc[kMB];
#pragma unroll
                for (int c = 0; c < kMB; c++) { ur[c] = c < nb ? Hs[o + c] : 0.0; xc[c] = c < nb ? xs[j0 + c] : 0.0; }
                double sv = 0;
#pragma unroll
                for (int c = 0; c < kMB; c++) sv += ur[c] * xc[c];
                xs[r] -= sv;
            }
            __syncthreads();
        }
        for (int i = tid; i < n; i += kWinThreads) pr.xp[i] = xs[i];
    }
    CL_STAMP(4);
    if (!ok2) for (int i = tid; i < n; i += kWinThreads) pr.xp[i] = 0;
    if (tid == 0) ct->ok2 = ok2 ? 1 : 0;
}
