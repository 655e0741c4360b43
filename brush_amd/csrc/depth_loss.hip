// depth_loss.hip — depth supervision (include/brush_hip_depth_loss.h): the fused depth loss of an expected-depth
// map against a target, and the held-out depth metrics.  Streaming kernels: a pixel is 8 B read and 4 B written, no blending;
// the time is bandwidth plus launch latency.  The sums are f64 with a fixed order (the pattern of exposure.hip): each lane adds
// its pixels in index order, a lane-exchange butterfly inside the wave, the block's waves in wave order through LDS, one f64
// row per block in a context slot, and one block adds the rows in index order.  No float atomics: two calls give the same bits.
#include <cmath>

#include "context.h"
#include "device_f64_sum.h"

namespace bh {

namespace {

constexpr int DL_FINAL_WG = 256;     // the final block: lane i adds rows i, i + 256, ... in index order, then the lanes in lane order

struct DepthLossArgs {
    uint64_t pixels;
    uint32_t kind;
    float scale, offset;
    float c;   // weight / (H W), rounded once on the host
};

// t = fmaf(scale, gt, offset); valid: gt finite, t > 0, E > 0
BH_DEV bool dl_target(const DepthLossArgs& a, float e, float g, float& t) {
    t = __builtin_fmaf(a.scale, g, a.offset);
    return is_finite_f32(g) && t > 0.0f && e > 0.0f;
}

template <uint32_t KIND, bool GRAD>
__global__ __launch_bounds__(DL_WG) void depth_loss_kernel(DepthLossArgs a, const float* __restrict__ depth, const float* __restrict__ gt,
                                                           float* __restrict__ v_depth, double* __restrict__ partials) {
    __shared__ double wave_rows[DL_WAVES][DL_ROW];
    double s[2] = {0.0, 0.0};
    const uint64_t stride = (uint64_t)gridDim.x * DL_WG;
    for (uint64_t p = (uint64_t)blockIdx.x * DL_WG + threadIdx.x; p < a.pixels; p += stride) {
        const float e = depth[p];
        float t;
        const bool valid = dl_target(a, e, gt[p], t);
        float l = 0.0f, v = 0.0f;
        if (valid) {
            if (KIND == BH_DEPTH_LOSS_L1) {
                const float d = e - t;
                l = __builtin_fabsf(d);
                v = d > 0.0f ? a.c : (d < 0.0f ? -a.c : 0.0f);
            } else {
                const float d = 1.0f / e - t;
                l = __builtin_fabsf(d);
                const float sc = d > 0.0f ? a.c : (d < 0.0f ? -a.c : 0.0f);
                v = d == 0.0f ? 0.0f : -sc / (e * e);   // (a zero stays +0, as an invalid pixel's)
            }
            s[0] += (double)l;
            s[1] += 1.0;
        }
        if (GRAD) v_depth[p] = v;
    }
    dl_block_store<2>(s, wave_rows, partials);
}

__global__ __launch_bounds__(DL_WG) void depth_metrics_kernel(DepthLossArgs a, const float* __restrict__ depth, const float* __restrict__ gt,
                                                              double* __restrict__ partials) {
    __shared__ double wave_rows[DL_WAVES][DL_ROW];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const uint64_t stride = (uint64_t)gridDim.x * DL_WG;
    for (uint64_t p = (uint64_t)blockIdx.x * DL_WG + threadIdx.x; p < a.pixels; p += stride) {
        const float e = depth[p];
        float t;
        if (!dl_target(a, e, gt[p], t)) continue;
        const float zt = a.kind == BH_DEPTH_LOSS_DISPARITY ? 1.0f / t : t;
        const double ed = (double)e, zd = (double)zt, d = ed - zd;
        const double ratio = fmax(ed / zd, zd / ed);
        s[0] += fabs(d) / zd;
        s[1] = fma(d, d, s[1]);
        s[2] += ratio < 1.25 ? 1.0 : 0.0;
        s[3] += 1.0;
    }
    dl_block_store<4>(s, wave_rows, partials);
}

// one block: column k of the rows, added in a fixed order.  Returns the total in every lane.
BH_DEV double dl_final_column(uint32_t rows, const double* __restrict__ partials, int k, double* lanes) {
    double s = 0.0;
    for (uint32_t r = threadIdx.x; r < rows; r += DL_FINAL_WG) s += partials[(size_t)r * DL_ROW + k];
    __syncthreads();   // (the previous column's lanes[] has been read)
    lanes[threadIdx.x] = s;
    __syncthreads();
    double total = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < DL_FINAL_WG; ++i) total += lanes[i];
    return total;   // (lane 0's is the sum)
}

__global__ __launch_bounds__(DL_FINAL_WG) void depth_loss_final_kernel(uint32_t rows, const double* __restrict__ partials, float c, float* __restrict__ loss,
                                                                       float* __restrict__ accum, float* __restrict__ accum_host) {
    __shared__ double lanes[DL_FINAL_WG];
    const double sum = dl_final_column(rows, partials, 0, lanes);
    const double cnt = dl_final_column(rows, partials, 1, lanes);
    if (threadIdx.x == 0) {
        const float l = (float)((double)c * sum);
        loss[0] = l;
        loss[1] = (float)cnt;
        if (accum) {   // the train step: its loss grows in place, in f32, and travels to the pinned word the host reads
            const float total = accum[0] + l;
            accum[0] = total;
            if (accum_host) accum_host[0] = total;
        }
    }
}

__global__ __launch_bounds__(DL_FINAL_WG) void depth_metrics_final_kernel(uint32_t rows, const double* __restrict__ partials, float* __restrict__ metrics) {
    __shared__ double lanes[DL_FINAL_WG];
    const double ar = dl_final_column(rows, partials, 0, lanes);
    const double se = dl_final_column(rows, partials, 1, lanes);
    const double in = dl_final_column(rows, partials, 2, lanes);
    const double cnt = dl_final_column(rows, partials, 3, lanes);
    if (threadIdx.x == 0) {
        const bool any = cnt > 0.0;
        metrics[0] = any ? (float)(ar / cnt) : 0.0f;
        metrics[1] = any ? (float)sqrt(se / cnt) : 0.0f;
        metrics[2] = any ? (float)(in / cnt) : 0.0f;
        metrics[3] = (float)cnt;
    }
}

DepthLossArgs dl_args(const BhDepthTarget& t) {
    DepthLossArgs a;
    a.pixels = (uint64_t)t.h * t.w;
    a.kind = t.kind;
    a.scale = t.scale;
    a.offset = t.offset;
    a.c = (float)((double)t.weight / (double)a.pixels);
    return a;
}

int check_target(bh_ctx* ctx, const BhDepthTarget* t, const char* who) {
    if (!t || !t->gt) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": null argument");
    if (t->h == 0 || t->w == 0) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": a depth map of zero size");
    if (t->kind > BH_DEPTH_LOSS_DISPARITY) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": unknown depth loss kind");
    return 0;
}

}  // namespace

double* loss_partials(bh_ctx* ctx, uint64_t pixels, uint32_t* blocks) {
    const uint64_t want = (pixels + DL_WG - 1) / DL_WG;
    *blocks = (uint32_t)(want < DL_MAX_BLOCKS ? want : DL_MAX_BLOCKS);
    return (double*)ensure(ctx, SLOT_PIXEL_LOSS, (size_t)DL_MAX_BLOCKS * DL_ROW * 8);
}

int launch_loss_pair_final(bh_ctx* ctx, uint32_t rows, const double* partials, float c, float* loss, float* accum, float* accum_host) {
    hipLaunchKernelGGL(depth_loss_final_kernel, dim3(1), dim3(DL_FINAL_WG), 0, ctx->stream, rows, partials, c, loss, accum, accum_host);
    BH_LAUNCH_CHECK(ctx, "depth_loss_final_kernel");
    return 0;
}

int launch_depth_loss(bh_ctx* ctx, const float* depth, const BhDepthTarget& t, float* loss, float* v_depth, float* accum, float* accum_host) {
    const DepthLossArgs a = dl_args(t);
    uint32_t blocks = 0;
    double* partials = loss_partials(ctx, a.pixels, &blocks);
    if (!partials) return BH_ERR_OOM;
    const dim3 grid(blocks), block(DL_WG);
#define BH_DL(K, G) hipLaunchKernelGGL((depth_loss_kernel<K, G>), grid, block, 0, ctx->stream, a, depth, t.gt, v_depth, partials)
    if (t.kind == BH_DEPTH_LOSS_L1) { if (v_depth) BH_DL(BH_DEPTH_LOSS_L1, true); else BH_DL(BH_DEPTH_LOSS_L1, false); }
    else { if (v_depth) BH_DL(BH_DEPTH_LOSS_DISPARITY, true); else BH_DL(BH_DEPTH_LOSS_DISPARITY, false); }
#undef BH_DL
    BH_LAUNCH_CHECK(ctx, "depth_loss_kernel");
    return launch_loss_pair_final(ctx, grid.x, partials, a.c, loss, accum, accum_host);
}

}  // namespace bh

using namespace bh;

extern "C" {

int bh_depth_loss_value_and_grad(bh_ctx* ctx, const float* depth, const BhDepthTarget* target, float* loss, float* v_depth) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!depth || !loss) return set_error(ctx, BH_ERR_INVALID_ARG, "depth_loss_value_and_grad: null argument");
    BH_TRY(check_target(ctx, target, "depth_loss_value_and_grad"));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    if (!(target->weight > 0.0f)) {   // no term: all +0, no pixel is looked at
        BH_HIP(ctx, hipMemsetAsync(loss, 0, 8, ctx->stream));
        if (v_depth) BH_HIP(ctx, hipMemsetAsync(v_depth, 0, (size_t)target->h * target->w * 4, ctx->stream));
        return 0;
    }
    ProfScope ps(ctx, "DepthLoss");
    return launch_depth_loss(ctx, depth, *target, loss, v_depth, nullptr, nullptr);
}

int bh_train_set_depth(bh_ctx* ctx, const BhDepthTarget* target) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    ctx->terms.depth_attached = target != nullptr;
    ctx->terms.depth_target = target ? *target : BhDepthTarget{};
    return 0;
}

int bh_eval_depth_metrics(bh_ctx* ctx, const float* depth, const BhDepthTarget* target, float* metrics) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!depth || !metrics) return set_error(ctx, BH_ERR_INVALID_ARG, "eval_depth_metrics: null argument");
    BH_TRY(check_target(ctx, target, "eval_depth_metrics"));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    const DepthLossArgs a = dl_args(*target);
    uint32_t rows = 0;
    double* partials = loss_partials(ctx, a.pixels, &rows);
    if (!partials) return BH_ERR_OOM;
    ProfScope ps(ctx, "DepthMetrics");
    hipLaunchKernelGGL(depth_metrics_kernel, dim3(rows), dim3(DL_WG), 0, ctx->stream, a, depth, target->gt, partials);
    BH_LAUNCH_CHECK(ctx, "depth_metrics_kernel");
    hipLaunchKernelGGL(depth_metrics_final_kernel, dim3(1), dim3(DL_FINAL_WG), 0, ctx->stream, rows, partials, metrics);
    BH_LAUNCH_CHECK(ctx, "depth_metrics_final_kernel");
    return 0;
}

}  // extern "C"
