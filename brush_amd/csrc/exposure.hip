// exposure.hip — per-view exposure compensation (brush_hip_exposure.h): the affine colour transform of a view on
// the rasterizer's image, its backward, and Adam on the twelve parameters of the view, all on the device.  Three kernels, all
// streaming or tiny: the point is to stay at HBM speed and to keep the order of the f64 reduction fixed.  The table itself — a
// bh_exposure is a ParamTable of rows of 12 with f64 moments — and every entry point that only manages it are param_table.h's, shared
// with bilagrid.hip and envmap.hip; the f64 reductions and the Adam step are device_f64_sum.h's.
#include "../../include/brush_hip_exposure.h"
#include "device_f64_sum.h"
#include "param_table.h"

namespace bh {

constexpr int EXP_WG = 256;
constexpr int EXP_WAVES = EXP_WG / 64;
// apply: grid-stride over pixels, at most 8 blocks of 256 per CU
constexpr uint32_t EXP_APPLY_MAX_BLOCKS = 2048;
// backward: the grid depends on H W alone and is capped at 4 blocks per CU (24 f64 accumulators per lane, 4 waves per SIMD):
// a 1080p frame is 7.9 passes of the capped grid, so the per-lane f64 sums amortise the block reduction behind them
constexpr uint32_t EXP_BWD_MAX_BLOCKS = 1024;

// y = A x + b on rgb, alpha passes through.  m is the table row: every lane reads the same twelve words through a read-only
// pointer, which the compiler turns into scalar loads (the row changes on the device, so it cannot be a by-value argument).
__global__ __launch_bounds__(EXP_WG) void exposure_apply_kernel(const float* __restrict__ m, const float4* img, float4* out, uint64_t pixels) {
    float a[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) a[k] = m[k];
    const uint64_t stride = (uint64_t)gridDim.x * EXP_WG;
    for (uint64_t p = (uint64_t)blockIdx.x * EXP_WG + threadIdx.x; p < pixels; p += stride) {
        const float4 x = img[p];
        float4 y;
        y.x = fmaf(a[0], x.x, fmaf(a[1], x.y, fmaf(a[2], x.z, a[3])));
        y.y = fmaf(a[4], x.x, fmaf(a[5], x.y, fmaf(a[6], x.z, a[7])));
        y.z = fmaf(a[8], x.x, fmaf(a[9], x.y, fmaf(a[10], x.z, a[11])));
        y.w = x.w;
        out[p] = y;
    }
}

// v = A^T v' on rgb (alpha passes through; v_img may be v_exposed: a lane reads its pixel before it writes it), and the block's
// share of v_m: each lane keeps twelve f64 sums over its pixels (f32 x f32 is exact in f64, so a term costs one rounding, the
// add's), then a lane-exchange butterfly inside the wave, the block's waves in wave order through LDS, one f64 row per block.
__global__ __launch_bounds__(EXP_WG) void exposure_backward_kernel(const float* __restrict__ m, const float4* __restrict__ x_img, const float4* v_exposed,
                                                                   float4* v_img, uint64_t pixels, double* __restrict__ partials) {
    __shared__ double wave_rows[EXP_WAVES][12];
    float a[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) a[k] = m[k];
    double s[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) s[k] = 0.0;
    const uint64_t stride = (uint64_t)gridDim.x * EXP_WG;
    for (uint64_t p = (uint64_t)blockIdx.x * EXP_WG + threadIdx.x; p < pixels; p += stride) {
        const float4 x = x_img[p];
        const float4 g = v_exposed[p];
        float4 v;
        v.x = fmaf(a[0], g.x, fmaf(a[4], g.y, a[8] * g.z));
        v.y = fmaf(a[1], g.x, fmaf(a[5], g.y, a[9] * g.z));
        v.z = fmaf(a[2], g.x, fmaf(a[6], g.y, a[10] * g.z));
        v.w = g.w;
        v_img[p] = v;
        const double x0 = x.x, x1 = x.y, x2 = x.z;
        const double g0 = g.x, g1 = g.y, g2 = g.z;
        s[0] = fma(g0, x0, s[0]); s[1] = fma(g0, x1, s[1]); s[2] = fma(g0, x2, s[2]); s[3] += g0;
        s[4] = fma(g1, x0, s[4]); s[5] = fma(g1, x1, s[5]); s[6] = fma(g1, x2, s[6]); s[7] += g1;
        s[8] = fma(g2, x0, s[8]); s[9] = fma(g2, x1, s[9]); s[10] = fma(g2, x2, s[10]); s[11] += g2;
    }
    dl_block_store<12, 12, EXP_WAVES>(s, wave_rows, partials);
}

// one block: the rows' twelve totals (dl_final_rows12), lane k writes grad[k] and — update — steps param[k] by Adam in f64 on the
// unrounded sum.  rows == 0: twelve zeros, and still a step.
__global__ __launch_bounds__(DL_FINAL_CHUNKS * 12) void exposure_final_kernel(uint32_t rows, const double* __restrict__ partials, float* __restrict__ grad,
                                                                              float* __restrict__ param, double* __restrict__ m1, double* __restrict__ m2,
                                                                              uint32_t* t, int update, double lr, double beta1, double beta2, double eps) {
    __shared__ double runs[DL_FINAL_CHUNKS][12];
    const double g = dl_final_rows12<4>(rows, partials, runs);
    if (threadIdx.x < 12) {
        const uint32_t tn = *t + 1u;   // (all twelve lanes read the count before lane 0 of the same wave writes it)
        grad[threadIdx.x] = (float)g;
        if (update) {
            double a, b;
            param[threadIdx.x] = adam_step_f64(g, param[threadIdx.x], m1[threadIdx.x], m2[threadIdx.x], (double)tn, lr, beta1, beta2, eps, a, b);
            m1[threadIdx.x] = a;
            m2[threadIdx.x] = b;
            if (threadIdx.x == 0) *t = tn;
        }
    }
}

static uint32_t grid_for(uint64_t pixels, uint32_t cap) {
    const uint64_t blocks = (pixels + EXP_WG - 1) / EXP_WG;
    return (uint32_t)(blocks < cap ? blocks : cap);
}

int launch_exposure_apply(bh_ctx* ctx, const bh_exposure* tab, uint32_t view, const float* img, uint32_t h, uint32_t w, float* out) {
    const uint64_t pixels = (uint64_t)h * w;
    if (pixels == 0) return 0;
    hipLaunchKernelGGL(exposure_apply_kernel, dim3(grid_for(pixels, EXP_APPLY_MAX_BLOCKS)), dim3(EXP_WG), 0, ctx->stream,
                       tab->param + (size_t)(view - 1) * 12, reinterpret_cast<const float4*>(img), reinterpret_cast<float4*>(out), pixels);
    BH_LAUNCH_CHECK(ctx, "exposure_apply_kernel");
    return 0;
}

int launch_exposure_backward(bh_ctx* ctx, bh_exposure* tab, uint32_t view, const float* img, const float* v_exposed, uint32_t h, uint32_t w,
                             float* v_img, bool update) {
    const uint64_t pixels = (uint64_t)h * w;
    const uint32_t rows = grid_for(pixels, EXP_BWD_MAX_BLOCKS);
    auto* partials = (double*)ensure(ctx, SLOT_EXPOSURE, (size_t)EXP_BWD_MAX_BLOCKS * 12 * 8);
    if (!partials) return BH_ERR_OOM;
    const size_t row = (size_t)(view - 1);
    if (rows > 0) {
        hipLaunchKernelGGL(exposure_backward_kernel, dim3(rows), dim3(EXP_WG), 0, ctx->stream, tab->param + row * 12,
                           reinterpret_cast<const float4*>(img), reinterpret_cast<const float4*>(v_exposed), reinterpret_cast<float4*>(v_img), pixels,
                           partials);
        BH_LAUNCH_CHECK(ctx, "exposure_backward_kernel");
    }
    hipLaunchKernelGGL(exposure_final_kernel, dim3(1), dim3(DL_FINAL_CHUNKS * 12), 0, ctx->stream, rows, partials, tab->grad + row * 12,
                       tab->param + row * 12, static_cast<double*>(tab->m1) + row * 12, static_cast<double*>(tab->m2) + row * 12, tab->t + row,
                       update ? 1 : 0, tab->lr, tab->beta1, tab->beta2, tab->eps);
    BH_LAUNCH_CHECK(ctx, "exposure_final_kernel");
    return 0;
}

}  // namespace bh

using namespace bh;

extern "C" {

int bh_exposure_create(bh_ctx* ctx, uint32_t n_views, bh_exposure** table) {
    BH_TRY(param_table_create_args(ctx, table, n_views, "exposure_create"));
    bh_exposure* tab = new bh_exposure;
    BH_TRY(param_table_create(ctx, tab, n_views, 12, 0, &COLOUR_IDENTITY, "exposure_create"));
    *table = tab;
    return 0;
}

int bh_exposure_destroy(bh_ctx* ctx, bh_exposure* table) { return param_table_destroy(ctx, PT_EXPOSURE, table, "exposure_destroy"); }

int bh_exposure_set_params(bh_ctx* ctx, bh_exposure* table, uint32_t first_view, uint32_t count, const float* host) {
    return param_table_set_params(ctx, PT_EXPOSURE, table, first_view, count, host, "exposure_set_params");
}

int bh_exposure_get_params(bh_ctx* ctx, bh_exposure* table, uint32_t first_view, uint32_t count, float* host) {
    return param_table_get_rows(ctx, PT_EXPOSURE, table, &ParamTable::param, first_view, count, host, "exposure_get_params");
}

int bh_exposure_get_grad(bh_ctx* ctx, bh_exposure* table, uint32_t first_view, uint32_t count, float* host) {
    return param_table_get_rows(ctx, PT_EXPOSURE, table, &ParamTable::grad, first_view, count, host, "exposure_get_grad");
}

int bh_exposure_get_state(bh_ctx* ctx, bh_exposure* table, uint32_t view, double* m1, double* m2, uint32_t* t) {
    return param_table_get_state(ctx, PT_EXPOSURE, table, view, m1, m2, t, "exposure_get_state");
}

int bh_exposure_set_state(bh_ctx* ctx, bh_exposure* table, uint32_t view, const double* m1, const double* m2, uint32_t t) {
    return param_table_set_state(ctx, PT_EXPOSURE, table, view, m1, m2, t, "exposure_set_state");
}

int bh_exposure_set_adam(bh_ctx* ctx, bh_exposure* table, double lr, double beta1, double beta2, double eps) {
    return param_table_set_adam(ctx, PT_EXPOSURE, table, lr, beta1, beta2, eps, "exposure_set_adam");
}

int bh_exposure_apply(bh_ctx* ctx, bh_exposure* table, uint32_t view, const float* img_hwc4, uint32_t h, uint32_t w, float* out_hwc4) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!img_hwc4 || !out_hwc4) return set_error(ctx, BH_ERR_INVALID_ARG, "exposure_apply: null argument");
    BH_TRY(check_image(ctx, h, w, /*below_2_31=*/false, "exposure_apply"));   // (the kernels count pixels in 64 bits)
    BH_TRY(check_rows(ctx, PT_EXPOSURE, table, view, 1, "exposure_apply"));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return launch_exposure_apply(ctx, table, view, img_hwc4, h, w, out_hwc4);
}

int bh_exposure_backward(bh_ctx* ctx, bh_exposure* table, uint32_t view, const float* img_hwc4, const float* v_exposed, uint32_t h, uint32_t w,
                         float* v_img, int update) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!img_hwc4 || !v_exposed || !v_img) return set_error(ctx, BH_ERR_INVALID_ARG, "exposure_backward: null argument");
    BH_TRY(check_image(ctx, h, w, /*below_2_31=*/false, "exposure_backward"));
    BH_TRY(check_rows(ctx, PT_EXPOSURE, table, view, 1, "exposure_backward"));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return launch_exposure_backward(ctx, table, view, img_hwc4, v_exposed, h, w, v_img, update != 0);
}

int bh_train_set_exposure(bh_ctx* ctx, bh_exposure* table) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    BH_TRY(param_table_attachable(ctx, PT_EXPOSURE, table, "train_set_exposure"));
    ctx->terms.exposure = table;
    return 0;
}

}  // extern "C"
