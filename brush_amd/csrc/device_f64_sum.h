// device_f64_sum.h — the deterministic f64 pieces of the streaming kernels (depth_loss.hip, normal_loss.hip, distortion.hip, exposure.hip,
// bilagrid.hip, project.hip's pose pass, intrinsics.hip): each lane adds its items in index order, a lane-exchange butterfly inside the wave, the
// block's waves in wave order through LDS, one f64 row per block in a context slot; one block then adds the rows in index order
// (depth_loss.hip's final kernels, dl_final_rows12 here).  And the f64 Adam step of the per-view tables' elements.
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

// the block's K sums -> row blockIdx.x of partials, rows of STRIDE words (the columns behind K stay unwritten and unread)
template <int K, int STRIDE = DL_ROW, int WAVES = DL_WAVES>
BH_DEV void dl_block_store(const double (&s)[K], double (*wave_rows)[STRIDE], double* __restrict__ partials) {
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
        for (int w = 1; w < WAVES; ++w) r += wave_rows[w][threadIdx.x];
        partials[(size_t)blockIdx.x * STRIDE + threadIdx.x] = r;
    }
}

// R partial rows of 12 -> 12 totals, by one block of DL_FINAL_CHUNKS * 12 = 1020 lanes: lane (chunk, k) adds entry k of its run of
// consecutive rows in index order, lane k then adds the runs in order and gets the total (the other lanes get 0).  The pass waits on
// memory, one dependent f64 add per row: at 1 M splats / 1080p (3400 rows of the pose pass) 16 runs took 64 us, five times K18.
// UNROLL: of the loop over the runs (its callers were compiled with different ones, and keep them)
// dl_final_rows<K, CHUNKS, UNROLL>: the same for rows of K by CHUNKS * K lanes (the intrinsics pass: 4 columns, 256 runs)
constexpr int DL_FINAL_CHUNKS = 85;
template <int K, int CHUNKS, int UNROLL>
BH_DEV double dl_final_rows(uint32_t rows, const double* __restrict__ partials, double (*runs)[K]) {
    const uint32_t chunk = threadIdx.x / (uint32_t)K, k = threadIdx.x % (uint32_t)K;
    const uint32_t per = (rows + CHUNKS - 1) / CHUNKS;
    const uint32_t r0 = chunk * per < rows ? chunk * per : rows;
    const uint32_t r1 = r0 + per < rows ? r0 + per : rows;
    double s = 0.0;
    uint32_t r = r0;
    for (; r + 4 <= r1; r += 4) {   // four loads in flight, the adds in index order
        const double a0 = partials[(size_t)r * K + k], a1 = partials[(size_t)(r + 1) * K + k];
        const double a2 = partials[(size_t)(r + 2) * K + k], a3 = partials[(size_t)(r + 3) * K + k];
        s += a0; s += a1; s += a2; s += a3;
    }
    for (; r < r1; ++r) s += partials[(size_t)r * K + k];
    runs[chunk][k] = s;
    __syncthreads();
    double total = 0.0;
    if (threadIdx.x < K) {
        total = runs[0][threadIdx.x];
#pragma unroll UNROLL
        for (int i = 1; i < CHUNKS; ++i) total += runs[i][threadIdx.x];
    }
    return total;
}
template <int UNROLL>
BH_DEV double dl_final_rows12(uint32_t rows, const double* __restrict__ partials, double (*runs)[12]) {
    return dl_final_rows<12, DL_FINAL_CHUNKS, UNROLL>(rows, partials, runs);
}

// One Adam step of an element in f64 on the unrounded gradient sum g, at step count tn >= 1: returns the new parameter; a, b are the
// new moments, unrounded (the caller stores them in its own type)
BH_DEV float adam_step_f64(double g, float param, double m1, double m2, double tn, double lr, double beta1, double beta2, double eps, double& a, double& b) {
    a = beta1 * m1 + (1.0 - beta1) * g;
    b = beta2 * m2 + (1.0 - beta2) * g * g;
    const double ah = a / (1.0 - pow(beta1, tn));
    const double bh = b / (1.0 - pow(beta2, tn));
    return (float)((double)param - lr * ah / (sqrt(bh) + eps));
}

}  // namespace bh
