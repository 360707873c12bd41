// One keyframe in LDS for the windowed searches that run one workgroup per problem (sim3_match.hip, sim3_project.hip): keypoint xy, octave, the 32-byte
// descriptors and the 64 x 48 cell table in KeyFrame::GetFeaturesInArea's visiting order (cell column, then cell row, then keypoint index), and the
// cv::Mat product both files round alike.  Device code only; the including file owns the LDS block and says where the arrays lie.
#pragma once
#include "common.h"

namespace oslam {
namespace kf_stage {

constexpr int kGridCols = 64, kGridRows = 48;   // reference include/Frame.h:43-44 (KeyFrame copies the Frame's grid, src/KeyFrame.cc:33-55)
constexpr int kGridCells = kGridCols * kGridRows;
constexpr int kThreads = 1024;                  // threads of the staging workgroup
constexpr int kMaxKps = 2400;                   // LDS budget: 51 bytes per keypoint (the staged arrays and 8 bytes of the including kernel's) and the cell table

struct Grid { float minX, minY, invW, invH; };   // mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv

struct Staged {
    uint32_t* desc;    // [ncap][8]
    float2* xy;        // [ncap]
    int* cell;         // [kGridCells + 1] end of every cell in items
    uint16_t* items;   // [ncap] keypoints sorted by cell (ix major, iy minor), index order inside a cell
    int8_t* oct;       // [ncap]
};

// cv::Mat 3x3 * 3x1 + 3x1 as matcher.hip restates it (gemm_row): the three products summed in float from left to right, the `+ c` in double, rounded once
__device__ __forceinline__ float gemm_row(const float* a, const float* x, float cc) {
    const float t0 = a[0] * x[0] + a[1] * x[1] + a[2] * x[2];
    return (float)((double)t0 + (double)cc);
}

// The keyframe (N keypoints at kps, descriptors at desc8) into LDS: xy, octave, descriptors, and mGrid (src/Frame.cc:455-470: cell = round((x - mnMinX) * inv),
// push_back in index order).  s_wtot: kThreads / 64 ints of LDS.  Begins and ends with a barrier.
__device__ inline void stage_target(const Staged& s, const oslam_keypoint_t* kps, const uint8_t* desc8, int N, const Grid& g, int* s_wtot) {
    const int tid = threadIdx.x;
    const uint32_t* gdesc = (const uint32_t*)desc8;
    __syncthreads();   // the readers of the keyframe staged before are done
    for (int i = tid; i <= kGridCells; i += kThreads) s.cell[i] = 0;
    __syncthreads();
    for (int i = tid; i < N; i += kThreads) {
        const oslam_keypoint_t kp = kps[i];
        s.xy[i] = make_float2(kp.x, kp.y);
        s.oct[i] = (int8_t)min(max(kp.octave, -2), 127);   // (the level gate compares with levels 0 .. 15: -2 and 127 stand for everything beyond)
        const int px = (int)roundf((kp.x - g.minX) * g.invW);
        const int py = (int)roundf((kp.y - g.minY) * g.invH);
        if (px >= 0 && px < kGridCols && py >= 0 && py < kGridRows) atomicAdd(&s.cell[px * kGridRows + py], 1);
    }
    for (int i = tid; i < N * 8; i += kThreads) s.desc[i] = gdesc[i];
    __syncthreads();
    {   // exclusive scan of the cell counts, kCellsPer per thread
        constexpr int kCellsPer = kGridCells / kThreads;
        static_assert(kCellsPer * kThreads == kGridCells, "the cell scan gives every thread the same number of cells");
        const int lane = tid & 63, wv = tid >> 6;
        const int base = tid * kCellsPer;
        int cc[kCellsPer];
        int incl = 0;
#pragma unroll
        for (int k = 0; k < kCellsPer; k++) { cc[k] = s.cell[base + k]; incl += cc[k]; }
        const int local = incl;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (lane == 63) s_wtot[wv] = incl;
        __syncthreads();
        int start = incl - local;
        for (int i = 0; i < wv; i++) start += s_wtot[i];
#pragma unroll
        for (int k = 0; k < kCellsPer; k++) { s.cell[base + k] = start; start += cc[k]; }
    }
    __syncthreads();
    // scatter with the cell starts as cursors (afterwards cell[c] = end of cell c = start of c + 1), then restore index order inside every cell
    for (int i = tid; i < N; i += kThreads) {
        const float2 p = s.xy[i];
        const int px = (int)roundf((p.x - g.minX) * g.invW);
        const int py = (int)roundf((p.y - g.minY) * g.invH);
        if (px >= 0 && px < kGridCols && py >= 0 && py < kGridRows) {
            const int pos = atomicAdd(&s.cell[px * kGridRows + py], 1);
            s.items[pos] = (uint16_t)i;
        }
    }
    __syncthreads();
    for (int cell = tid; cell < kGridCells; cell += kThreads) {
        const int st = cell > 0 ? s.cell[cell - 1] : 0, en = s.cell[cell];
        for (int q = st + 1; q < en; q++) {   // insertion sort, cells hold a handful of points
            const uint16_t v = s.items[q];
            int p = q - 1;
            while (p >= st && s.items[p] > v) { s.items[p + 1] = s.items[p]; p--; }
            s.items[p + 1] = v;
        }
    }
    __syncthreads();
}

}  // namespace kf_stage
}  // namespace oslam
