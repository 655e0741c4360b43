// device_f64_sum.h — the deterministic f64 block sums of the streaming loss kernels (depth_loss.hip, normal_loss.hip; the pattern of
// exposure.hip): each lane adds its pixels in index order, a lane-exchange butterfly inside the wave, the block's waves in wave order
// through LDS, one f64 row per block in a context slot; one block then adds the rows in index order (depth_loss.hip's final kernels).
#pragma once
#include "device_math.h"

namespace bh {

constexpr int DL_WG = 256;
constexpr int DL_WAVES = DL_WG / 64;
// the grid depends on H W alone and is capped at 4 blocks per CU: a 1080p frame is two passes of the capped grid
constexpr uint32_t DL_MAX_BLOCKS = 1024;
constexpr int DL_ROW = 4;            // f64 words per block row (the loss uses 2, the metrics 4)

BH_DEV double dl_wave_sum(double x) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, 64);   // every lane adds the same pairs in the same order
    return x;
}

// the block's K sums -> row blockIdx.x of partials (the columns behind K stay unwritten and unread)
template <int K>
BH_DEV void dl_block_store(const double (&s)[K], double (*wave_rows)[DL_ROW], double* __restrict__ partials) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double r = dl_wave_sum(s[k]);
        if (lane == 0) wave_rows[wave][k] = r;
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)K) {
        double r = wave_rows[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < DL_WAVES; ++w) r += wave_rows[w][threadIdx.x];
        partials[(size_t)blockIdx.x * DL_ROW + threadIdx.x] = r;
    }
}

}  // namespace bh
