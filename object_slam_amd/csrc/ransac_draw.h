// The counter-based generator and the swap-with-back draw of the RANSAC solvers (include/oslam_hip.h, "PnP solver", normalisation 1): the same text for
// the kernels and for the host functions oslam_pnp_draw / oslam_sim3_draw, so that a caller can reproduce every sample of every iteration.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace oslam {

// A 32-bit hash of (seed, iteration, draw).
__host__ __device__ inline uint32_t ransac_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}
__host__ __device__ inline uint32_t ransac_hash(uint32_t seed, int iteration, int draw) {
    return ransac_mix(ransac_mix(seed + 0x9E3779B9u * (uint32_t)(iteration + 1)) ^ (0x85EBCA6Bu * (uint32_t)(draw + 1)));
}
// K indices of 0 .. N - 1 (N >= K) without replacement by the swap-with-back rule (src/PnPsolver.cc:188-201, src/Sim3Solver.cc:163-177), without the
// list: position p of the list holds p unless an earlier draw moved the back element there.
template <int K>
__host__ __device__ inline void ransac_draw(uint32_t seed, int iteration, int N, int (&idx)[K]) {
    int pos[K], val[K];
    for (int k = 0; k < K; k++) {
        const int size = N - k;
        const int randi = (int)(((uint64_t)ransac_hash(seed, iteration, k) * (uint64_t)size) >> 32);
        int at = randi, back = size - 1;
        for (int j = k - 1; j >= 0; j--) if (pos[j] == randi) { at = val[j]; break; }
        for (int j = k - 1; j >= 0; j--) if (pos[j] == size - 1) { back = val[j]; break; }
        idx[k] = at;
        pos[k] = randi; val[k] = back;
    }
}

}  // namespace oslam
