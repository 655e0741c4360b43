// exposure.hip — per-view exposure compensation (brush_hip_exposure.h): the affine colour transform of a view on
// the rasterizer's image, its backward, and Adam on the twelve parameters of the view, all on the device.  Three kernels, all
// streaming or tiny: the point is to stay at HBM speed and to keep the order of the f64 reduction fixed.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/brush_hip_exposure.h"
#include "context.h"

struct bh_exposure {
    uint32_t n_views = 0;
    void* mem = nullptr;          // one allocation: m1 | m2 | param | grad | t
    double* m1 = nullptr;         // [V,12]
    double* m2 = nullptr;         // [V,12]
    float* param = nullptr;       // [V,12]
    float* grad = nullptr;        // [V,12]
    uint32_t* t = nullptr;        // [V]
    double lr = 1e-3, beta1 = 0.9, beta2 = 0.999, eps = 1e-8;   // passed to the update by value
};

namespace bh {

constexpr int EXP_WG = 256;
constexpr int EXP_WAVES = EXP_WG / 64;
// apply: grid-stride over pixels, at most 8 blocks of 256 per CU
constexpr uint32_t EXP_APPLY_MAX_BLOCKS = 2048;
// backward: the grid depends on H W alone and is capped at 4 blocks per CU (24 f64 accumulators per lane, 4 waves per SIMD):
// a 1080p frame is 7.9 passes of the capped grid, so the per-lane f64 sums amortise the block reduction behind them
constexpr uint32_t EXP_BWD_MAX_BLOCKS = 1024;
// exposure_final_kernel: 85 runs of consecutive rows x 12 entries = 1020 lanes (the shape of pose_grad_final_kernel)
constexpr int EXP_FINAL_CHUNKS = 85;

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

BH_DEV double exposure_wave_sum(double x) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, 64);   // every lane adds the same pairs in the same order
    return x;
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
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const double r = exposure_wave_sum(s[k]);
        if (lane == 0) wave_rows[wave][k] = r;
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        double r = wave_rows[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < EXP_WAVES; ++w) r += wave_rows[w][threadIdx.x];
        partials[(size_t)blockIdx.x * 12 + threadIdx.x] = r;
    }
}

// one block: lane (chunk, k) adds entry k of its run of consecutive rows in index order, lane k then adds the runs in order,
// writes grad[k] and — update — steps param[k] by Adam in f64 on the unrounded sum.  rows == 0: twelve zeros, and still a step.
__global__ __launch_bounds__(EXP_FINAL_CHUNKS * 12) void exposure_final_kernel(uint32_t rows, const double* __restrict__ partials, float* __restrict__ grad,
                                                                               float* __restrict__ param, double* __restrict__ m1, double* __restrict__ m2,
                                                                               uint32_t* t, int update, double lr, double beta1, double beta2, double eps) {
    __shared__ double runs[EXP_FINAL_CHUNKS][12];
    const uint32_t chunk = threadIdx.x / 12u, k = threadIdx.x % 12u;
    const uint32_t per = (rows + EXP_FINAL_CHUNKS - 1) / EXP_FINAL_CHUNKS;
    const uint32_t r0 = chunk * per < rows ? chunk * per : rows;
    const uint32_t r1 = r0 + per < rows ? r0 + per : rows;
    double s = 0.0;
    uint32_t r = r0;
    for (; r + 4 <= r1; r += 4) {   // four loads in flight, the adds in index order
        const double a0 = partials[(size_t)r * 12 + k], a1 = partials[(size_t)(r + 1) * 12 + k];
        const double a2 = partials[(size_t)(r + 2) * 12 + k], a3 = partials[(size_t)(r + 3) * 12 + k];
        s += a0; s += a1; s += a2; s += a3;
    }
    for (; r < r1; ++r) s += partials[(size_t)r * 12 + k];
    runs[chunk][k] = s;
    __syncthreads();
    if (threadIdx.x < 12) {
        const uint32_t tn = *t + 1u;   // (all twelve lanes read the count before lane 0 of the same wave writes it)
        double g = runs[0][threadIdx.x];
#pragma unroll 4
        for (int i = 1; i < EXP_FINAL_CHUNKS; ++i) g += runs[i][threadIdx.x];
        grad[threadIdx.x] = (float)g;
        if (update) {
            const double a = beta1 * m1[threadIdx.x] + (1.0 - beta1) * g;
            const double b = beta2 * m2[threadIdx.x] + (1.0 - beta2) * g * g;
            const double ah = a / (1.0 - pow(beta1, (double)tn));
            const double bh = b / (1.0 - pow(beta2, (double)tn));
            param[threadIdx.x] = (float)((double)param[threadIdx.x] - lr * ah / (sqrt(bh) + eps));
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
    hipLaunchKernelGGL(exposure_final_kernel, dim3(1), dim3(EXP_FINAL_CHUNKS * 12), 0, ctx->stream, rows, partials, tab->grad + row * 12,
                       tab->param + row * 12, tab->m1 + row * 12, tab->m2 + row * 12, tab->t + row, update ? 1 : 0, tab->lr, tab->beta1, tab->beta2,
                       tab->eps);
    BH_LAUNCH_CHECK(ctx, "exposure_final_kernel");
    return 0;
}

uint32_t exposure_views(const bh_exposure* tab) { return tab->n_views; }

static void exposure_free(bh_exposure* tab) {
    if (tab->mem) (void)hipFree(tab->mem);
    delete tab;
}

void exposure_free_all(bh_ctx* ctx) {
    for (bh_exposure* tab : ctx->exposures) exposure_free(tab);
    ctx->exposures.clear();
    ctx->exposure = nullptr;
}

// the table is one of this ctx's and the views first .. first + count - 1 are rows of it
static int check_rows(bh_ctx* ctx, const bh_exposure* tab, uint32_t first, uint32_t count, const char* who) {
    if (!tab || std::find(ctx->exposures.begin(), ctx->exposures.end(), tab) == ctx->exposures.end())
        return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": not an exposure table of this context");
    if (first == 0 || count == 0 || first > tab->n_views || count > tab->n_views - first + 1)
        return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": view out of range (views are numbered 1 .. n_views)");
    return 0;
}

static int read_back(bh_ctx* ctx, void* host, const void* dev, size_t bytes) {
    BH_HIP(ctx, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    BH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    deliver_pending_loss(ctx);
    return 0;
}

}  // namespace bh

using namespace bh;

extern "C" {

int bh_exposure_create(bh_ctx* ctx, uint32_t n_views, bh_exposure** table) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!table) return set_error(ctx, BH_ERR_INVALID_ARG, "exposure_create: null argument");
    *table = nullptr;
    if (n_views == 0 || n_views > (1u << 24)) return set_error(ctx, BH_ERR_INVALID_ARG, "exposure_create: n_views must be 1 .. 2^24");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    const size_t v = n_views, bytes = v * 12 * 8 * 2 + v * 12 * 4 * 2 + v * 4;
    void* mem = nullptr;
    BH_HIP(ctx, hipMalloc(&mem, bytes));
    auto* tab = new bh_exposure;
    tab->n_views = n_views;
    tab->mem = mem;
    tab->m1 = static_cast<double*>(mem);
    tab->m2 = tab->m1 + v * 12;
    tab->param = reinterpret_cast<float*>(tab->m2 + v * 12);
    tab->grad = tab->param + v * 12;
    tab->t = reinterpret_cast<uint32_t*>(tab->grad + v * 12);
    std::vector<float> ident(v * 12, 0.0f);
    for (size_t i = 0; i < v; ++i) ident[i * 12 + 0] = ident[i * 12 + 5] = ident[i * 12 + 10] = 1.0f;
    hipError_t e = hipMemsetAsync(mem, 0, bytes, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(tab->param, ident.data(), v * 12 * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (the staging vector dies here)
    if (e != hipSuccess) {
        exposure_free(tab);
        return check_hip(ctx, e, "exposure_create");
    }
    deliver_pending_loss(ctx);
    ctx->exposures.push_back(tab);
    *table = tab;
    return 0;
}

int bh_exposure_destroy(bh_ctx* ctx, bh_exposure* table) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    auto it = std::find(ctx->exposures.begin(), ctx->exposures.end(), table);
    if (!table || it == ctx->exposures.end()) return set_error(ctx, BH_ERR_INVALID_ARG, "exposure_destroy: not an exposure table of this context");
    if (ctx->exposure == table) ctx->exposure = nullptr;   // an attached table is detached first
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);   // kernels queued on the table have run
    deliver_pending_loss(ctx);
    ctx->exposures.erase(it);
    exposure_free(table);
    return 0;
}

int bh_exposure_set_params(bh_ctx* ctx, bh_exposure* table, uint32_t first_view, uint32_t count, const float* host) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!host) return set_error(ctx, BH_ERR_INVALID_ARG, "exposure_set_params: null argument");
    BH_TRY(check_rows(ctx, table, first_view, count, "exposure_set_params"));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    BH_HIP(ctx, hipMemcpyAsync(table->param + (size_t)(first_view - 1) * 12, host, (size_t)count * 48, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

int bh_exposure_get_params(bh_ctx* ctx, bh_exposure* table, uint32_t first_view, uint32_t count, float* host) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!host) return set_error(ctx, BH_ERR_INVALID_ARG, "exposure_get_params: null argument");
    BH_TRY(check_rows(ctx, table, first_view, count, "exposure_get_params"));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return read_back(ctx, host, table->param + (size_t)(first_view - 1) * 12, (size_t)count * 48);
}

int bh_exposure_get_grad(bh_ctx* ctx, bh_exposure* table, uint32_t first_view, uint32_t count, float* host) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!host) return set_error(ctx, BH_ERR_INVALID_ARG, "exposure_get_grad: null argument");
    BH_TRY(check_rows(ctx, table, first_view, count, "exposure_get_grad"));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return read_back(ctx, host, table->grad + (size_t)(first_view - 1) * 12, (size_t)count * 48);
}

int bh_exposure_get_state(bh_ctx* ctx, bh_exposure* table, uint32_t view, double* m1, double* m2, uint32_t* t) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!m1 || !m2 || !t) return set_error(ctx, BH_ERR_INVALID_ARG, "exposure_get_state: null argument");
    BH_TRY(check_rows(ctx, table, view, 1, "exposure_get_state"));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    const size_t row = view - 1;
    BH_HIP(ctx, hipMemcpyAsync(m1, table->m1 + row * 12, 96, hipMemcpyDeviceToHost, ctx->stream));
    BH_HIP(ctx, hipMemcpyAsync(m2, table->m2 + row * 12, 96, hipMemcpyDeviceToHost, ctx->stream));
    return read_back(ctx, t, table->t + row, 4);
}

int bh_exposure_set_state(bh_ctx* ctx, bh_exposure* table, uint32_t view, const double* m1, const double* m2, uint32_t t) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!m1 || !m2) return set_error(ctx, BH_ERR_INVALID_ARG, "exposure_set_state: null argument");
    BH_TRY(check_rows(ctx, table, view, 1, "exposure_set_state"));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    const size_t row = view - 1;
    BH_HIP(ctx, hipMemcpyAsync(table->m1 + row * 12, m1, 96, hipMemcpyHostToDevice, ctx->stream));
    BH_HIP(ctx, hipMemcpyAsync(table->m2 + row * 12, m2, 96, hipMemcpyHostToDevice, ctx->stream));
    BH_HIP(ctx, hipMemcpyAsync(table->t + row, &t, 4, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

int bh_exposure_set_adam(bh_ctx* ctx, bh_exposure* table, double lr, double beta1, double beta2, double eps) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    BH_TRY(check_rows(ctx, table, 1, 1, "exposure_set_adam"));
    if (!(lr >= 0.0) || !std::isfinite(lr) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps > 0.0) || !std::isfinite(eps))
        return set_error(ctx, BH_ERR_INVALID_ARG, "exposure_set_adam: needs lr >= 0, 0 <= beta < 1 and eps > 0, all finite");
    table->lr = lr;
    table->beta1 = beta1;
    table->beta2 = beta2;
    table->eps = eps;
    return 0;
}

int bh_exposure_apply(bh_ctx* ctx, bh_exposure* table, uint32_t view, const float* img_hwc4, uint32_t h, uint32_t w, float* out_hwc4) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!img_hwc4 || !out_hwc4) return set_error(ctx, BH_ERR_INVALID_ARG, "exposure_apply: null argument");
    if (h == 0 || w == 0) return set_error(ctx, BH_ERR_INVALID_ARG, "exposure_apply: an image of zero size");
    BH_TRY(check_rows(ctx, table, view, 1, "exposure_apply"));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return launch_exposure_apply(ctx, table, view, img_hwc4, h, w, out_hwc4);
}

int bh_exposure_backward(bh_ctx* ctx, bh_exposure* table, uint32_t view, const float* img_hwc4, const float* v_exposed, uint32_t h, uint32_t w,
                         float* v_img, int update) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!img_hwc4 || !v_exposed || !v_img) return set_error(ctx, BH_ERR_INVALID_ARG, "exposure_backward: null argument");
    if (h == 0 || w == 0) return set_error(ctx, BH_ERR_INVALID_ARG, "exposure_backward: an image of zero size");
    BH_TRY(check_rows(ctx, table, view, 1, "exposure_backward"));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return launch_exposure_backward(ctx, table, view, img_hwc4, v_exposed, h, w, v_img, update != 0);
}

int bh_train_set_exposure(bh_ctx* ctx, bh_exposure* table) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (table && std::find(ctx->exposures.begin(), ctx->exposures.end(), table) == ctx->exposures.end())
        return set_error(ctx, BH_ERR_INVALID_ARG, "train_set_exposure: not an exposure table of this context");
    ctx->exposure = table;
    return 0;
}

}  // extern "C"
