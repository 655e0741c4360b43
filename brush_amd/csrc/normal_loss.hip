// normal_loss.hip — the normal-consistency regulariser (include/brush_hip_normal_loss.h): ONE streaming kernel per
// frame, one thread per pixel, in place of depth -> normal, a loss pass and the depth -> normal backward with their two [H,W,3]
// intermediates (u and its cotangent).
//
// A pixel evaluates five stencils of device_depth_normal.h: its own (the loss term and v_normal) and its four neighbours' (the gather
// of v_depth, in the order of normal.hip's depth_to_normal_backward_kernel), each cotangent formed on the fly from the neighbour's N
// and alpha.  The 13-pixel depth diamond and the 5-pixel N / alpha cross go through the caches, not LDS: consecutive lanes hold
// consecutive pixels, so the left / right taps are the same lines the wave has just loaded, and the rows above and below are the lines
// the blocks one image row away load at the same time (L2).  An LDS tile would need a two-pixel halo on a 256 x 1 strip
// (five rows staged for one row of results), or 2-D blocks whose rows no longer coalesce; the unique bytes per pixel (4 depth + 12 N +
// 16 image, 16 written) are what HBM sees either way.  The f64 sums are depth_loss.hip's (device_f64_sum.h: lane, wave butterfly, waves
// in order through LDS, one row per block in a context slot) and its final block adds the rows in index order.  No float atomics.
#include "context.h"
#include "device_depth_normal.h"
#include "device_f64_sum.h"

namespace bh {

namespace {

struct NormalLossArgs {
    PinholeK k;
    uint64_t pixels;
    float c;   // weight / (H W), rounded once on the host
};

// d loss / d (the depth of neighbour `which` of the stencil at (x, y)), the cotangent of u formed from N and alpha at (x, y)
BH_DEV float nl_neighbour(const NormalLossArgs& a, const float* __restrict__ depth, const float* __restrict__ normal, const float* __restrict__ image,
                          uint32_t x, uint32_t y, int which) {
    const Stencil s = depth_stencil(a.k, depth, x, y);
    if (!s.valid) return 0.0f;
    const float len = length(s.c);
    if (len == 0.0f) return 0.0f;
    const float inv = 1.0f / len;
    const Vec3A u = scale(s.c, inv);
    const size_t q = (size_t)x + (size_t)y * a.k.w;
    const float m = -(a.c * image[q * 4 + 3]);
    const Vec3A v = v3(m * normal[q * 3], m * normal[q * 3 + 1], m * normal[q * 3 + 2]);
    return stencil_chain(s, inv, u, v, which);
}

template <bool ACCUMULATE>
__global__ __launch_bounds__(DL_WG) void normal_consistency_kernel(NormalLossArgs a, const float* __restrict__ normal, const float* __restrict__ depth,
                                                                   const float* __restrict__ image, float* __restrict__ v_normal, float* __restrict__ v_depth,
                                                                   double* __restrict__ partials) {
    __shared__ double wave_rows[DL_WAVES][DL_ROW];
    double s[2] = {0.0, 0.0};   // sum of l, valid count
    const uint64_t stride = (uint64_t)gridDim.x * DL_WG;
    for (uint64_t p = (uint64_t)blockIdx.x * DL_WG + threadIdx.x; p < a.pixels; p += stride) {
        const uint32_t x = (uint32_t)(p % a.k.w), y = (uint32_t)(p / a.k.w);
        const Stencil st = depth_stencil(a.k, depth, x, y);
        float ox = 0.0f, oy = 0.0f, oz = 0.0f;
        if (st.valid) {
            const float len = length(st.c);
            const float inv = len == 0.0f ? 0.0f : 1.0f / len;
            const float ux = st.c.x * inv, uy = st.c.y * inv, uz = st.c.z * inv;
            const float al = image[p * 4 + 3];
            const float nx = normal[p * 3], ny = normal[p * 3 + 1], nz = normal[p * 3 + 2];
            const float d = __builtin_fmaf(nz, uz, __builtin_fmaf(ny, uy, nx * ux));
            const float l = al * (1.0f - d);
            const float m = -(a.c * al);
            ox = m * ux; oy = m * uy; oz = m * uz;
            s[0] += (double)l;
            s[1] += 1.0;
        }
        v_normal[p * 3] = ox;
        v_normal[p * 3 + 1] = oy;
        v_normal[p * 3 + 2] = oz;
        // the gather: pixel (x, y) is the right neighbour of the stencil at x-1, the left one of x+1, the lower one of y-1 and the
        // upper one of y+1 (its own stencil does not read its own depth)
        float g = 0.0f;
        if (x >= 1u) g += nl_neighbour(a, depth, normal, image, x - 1u, y, 1);
        if (x + 1u < a.k.w) g += nl_neighbour(a, depth, normal, image, x + 1u, y, 0);
        if (y >= 1u) g += nl_neighbour(a, depth, normal, image, x, y - 1u, 3);
        if (y + 1u < a.k.h) g += nl_neighbour(a, depth, normal, image, x, y + 1u, 2);
        v_depth[p] = ACCUMULATE ? v_depth[p] + g : g;
    }
    dl_block_store<2>(s, wave_rows, partials);
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

}  // namespace

int launch_normal_loss(bh_ctx* ctx, const BhCamera& cam, const float* normal, const float* depth, const float* image, uint32_t h, uint32_t w, float weight,
                       bool accumulate_v_depth, float* loss, float* v_normal, float* v_depth, float* accum, float* accum_host) {
    NormalLossArgs a;
    a.k.fx = cam.fx; a.k.fy = cam.fy; a.k.cx = cam.cx; a.k.cy = cam.cy;
    a.k.w = w; a.k.h = h;
    a.pixels = (uint64_t)h * w;
    a.c = (float)((double)weight / (double)a.pixels);
    uint32_t blocks = 0;
    double* partials = loss_partials(ctx, a.pixels, &blocks);
    if (!partials) return BH_ERR_OOM;
    const dim3 grid(blocks), block(DL_WG);
    if (accumulate_v_depth) hipLaunchKernelGGL(normal_consistency_kernel<true>, grid, block, 0, ctx->stream, a, normal, depth, image, v_normal, v_depth, partials);
    else hipLaunchKernelGGL(normal_consistency_kernel<false>, grid, block, 0, ctx->stream, a, normal, depth, image, v_normal, v_depth, partials);
    BH_LAUNCH_CHECK(ctx, "normal_consistency_kernel");
    // loss = { f32(c * column 0), column 1 }: the depth loss's final block, rows added in the same fixed order
    return launch_loss_pair_final(ctx, grid.x, partials, a.c, loss, accum, accum_host);
}

}  // namespace bh

using namespace bh;

extern "C" {

int bh_normal_consistency_value_and_grad(bh_ctx* ctx, const BhCamera* cam, const float* normal, const float* depth, const float* image, uint32_t h, uint32_t w,
                                         float weight, uint32_t accumulate_v_depth, float* loss, float* v_normal, float* v_depth) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!cam || !normal || !depth || !image || !loss || !v_normal || !v_depth)
        return set_error(ctx, BH_ERR_INVALID_ARG, "normal_consistency_value_and_grad: null argument");
    if (h == 0 || w == 0) return set_error(ctx, BH_ERR_INVALID_ARG, "normal_consistency_value_and_grad: a map of zero size");
    if (cam->model != BH_CAMERA_PINHOLE) return set_error(ctx, BH_ERR_INVALID_ARG, "normal_consistency_value_and_grad: pinhole cameras only");
    const size_t pixels = (size_t)h * w;
    if (pixels > 0x7FFFFFFFull) return set_error(ctx, BH_ERR_INVALID_ARG, "normal_consistency_value_and_grad: more than 2^31 - 1 pixels");
    const struct { const void* p; size_t bytes; } in[3] = {{normal, pixels * 12}, {depth, pixels * 4}, {image, pixels * 16}};
    for (const auto& i : in)
        if (overlaps(v_normal, pixels * 12, i.p, i.bytes) || overlaps(v_depth, pixels * 4, i.p, i.bytes))
            return set_error(ctx, BH_ERR_INVALID_ARG, "normal_consistency_value_and_grad: v_normal and v_depth may not alias an input");
    if (overlaps(v_normal, pixels * 12, v_depth, pixels * 4) || overlaps(loss, 8, v_normal, pixels * 12) || overlaps(loss, 8, v_depth, pixels * 4))
        return set_error(ctx, BH_ERR_INVALID_ARG, "normal_consistency_value_and_grad: the outputs may not alias each other");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    if (!(weight > 0.0f)) {   // no term: all +0, no pixel is looked at
        BH_HIP(ctx, hipMemsetAsync(loss, 0, 8, ctx->stream));
        BH_HIP(ctx, hipMemsetAsync(v_normal, 0, pixels * 12, ctx->stream));
        if (!accumulate_v_depth) BH_HIP(ctx, hipMemsetAsync(v_depth, 0, pixels * 4, ctx->stream));
        return 0;
    }
    ProfScope ps(ctx, "NormalLoss");
    return launch_normal_loss(ctx, *cam, normal, depth, image, h, w, weight, accumulate_v_depth != 0, loss, v_normal, v_depth, nullptr, nullptr);
}

int bh_train_set_normal(bh_ctx* ctx, const BhNormalTermConfig* cfg) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    ctx->terms.normal_attached = cfg != nullptr;
    ctx->terms.normal_term = cfg ? *cfg : BhNormalTermConfig{};
    return 0;
}

}  // extern "C"
