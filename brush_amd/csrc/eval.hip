// eval.hip — held-out evaluation: PSNR and SSIM of a rendered view against its packed ground truth.
//
// Reference: eval_stats (brush-train/src/eval.rs:23-63), called per held-out view by run_eval
// (brush-process/src/train_stream.rs:506-566):
//   q    = round(render.rgb * 255) / 255                  f32, round half to even, true divide, NOT clamped
//   mse  = mean_{H,W,3} image_loss_eval(q, gt, l1 1, ssim 0)^2
//   psnr = ln(1 / mse) * 10 / ln 10                       f32 (+inf when mse == 0)
//   ssim = mean_{H,W,3} image_loss_eval(q, gt, l1 0, ssim 1)   the loss forward's SSIM map (device_ssim.h), no composite, no mask
//
// MI355X shape.  The reference quantises into a new tensor, permutes it to CHW, runs the loss forward twice (each writes a
// [3,H,W] map and blurs all five moments) and reduces both maps.  Here one launch reads every pixel once as a float4, quantises it
// on the way into LDS beside its GT byte, and computes the squared error and the SSIM value of all three channels in the block
// that owns its 16x16 tile: 20 bytes of HBM per pixel (image + GT), + 4 with the rgb8 copy, and 16 bytes per tile of partial sums.
// The per-pixel terms are the f32 values the loss maps would hold; every sum is f64 in a fixed order (lanes of a wave, waves of a
// block, then tiles in index order in a one-block second launch), so the result does not depend on scheduling.
#include "device_ssim.h"

namespace bh {

constexpr int EVAL_WG = LB * LB;
constexpr int EVAL_FINAL_WG = 1024;

struct EvalArgs {
    uint32_t h, w;
    Taps taps;
};

// lane 0 of every wave ends up with the wave's sum; the tree is fixed, so is the result
BH_DEV double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

BH_DEV uint32_t rgb8_channel(float k) { return (uint32_t)__builtin_fminf(__builtin_fmaxf(k, 0.0f), 255.0f); }   // into_rgb8: clamped

// one 16x16 tile of the image: partial[tile] = (sum of the squared L1 map, sum of the SSIM map) over its pixels and 3 channels
__global__ __launch_bounds__(EVAL_WG) void eval_tile_kernel(const float4* __restrict__ img, const uint32_t* __restrict__ gt,
                                                            uint32_t* __restrict__ rgb8, double2* __restrict__ partial, EvalArgs a) {
    __shared__ float s_tile[3][SH * SH * 2];   // per channel (quantised render, gt) pairs with a HALO apron, zero outside the image
    __shared__ float s_h[SH * LB * 5];         // one channel's horizontally blurred moments at a time (24.5 KB of LDS in all: 6 blocks per CU)
    __shared__ double s_red[2][EVAL_WG / 64];
    const int tx0 = blockIdx.x * LB, ty0 = blockIdx.y * LB;
    const int rank = threadIdx.x;
    const int lx = rank % LB, ly = rank / LB;
    for (int i = rank; i < SH * SH; i += EVAL_WG) {
        const int r = i / SH, q = i % SH;
        const int y = ty0 + r - HALO, x = tx0 + q - HALO;
        float pv[3] = {0.0f, 0.0f, 0.0f}, ge[3] = {0.0f, 0.0f, 0.0f};
        if (y >= 0 && x >= 0 && y < (int)a.h && x < (int)a.w) {
            const uint32_t p = (uint32_t)y * a.w + (uint32_t)x;
            const float4 v = img[p];
            const uint32_t g = gt[p];
            // eval.rs:39: (render_rgb * 255.0).round() / 255.0 — burn's round is half to even (rintf), the divide correctly rounded
            const float k0 = rintf(v.x * 255.0f), k1 = rintf(v.y * 255.0f), k2 = rintf(v.z * 255.0f);
            pv[0] = k0 / 255.0f;
            pv[1] = k1 / 255.0f;
            pv[2] = k2 / 255.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) ge[c] = gt_channel(g, (uint32_t)c);
            // the tile's own pixels (not its apron) leave the 8-bit copy save_to_disk / the viewer want
            if (rgb8 && r >= HALO && r < HALO + LB && q >= HALO && q < HALO + LB)
                rgb8[p] = rgb8_channel(k0) | (rgb8_channel(k1) << 8) | (rgb8_channel(k2) << 16) | 0xff000000u;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s_tile[c][i * 2] = pv[c];
            s_tile[c][i * 2 + 1] = ge[c];
        }
    }
    __syncthreads();
    const bool inside = tx0 + lx < (int)a.w && ty0 + ly < (int)a.h;
    double sq = 0.0, ss = 0.0;
    for (int c = 0; c < 3; ++c) {
        for (int r = ly; r < SH; r += LB) {
            float o[5];
            hblur5(s_tile[c], SH, r, lx + HALO, a.taps, o);
#pragma unroll
            for (int k = 0; k < 5; ++k) s_h[(r * LB + lx) * 5 + k] = o[k];
        }
        __syncthreads();
        if (inside) {
            float o[5];
            vblur<5>(s_h, LB, ly + HALO, lx, a.taps, o);
            const float val = ssim_clamped(o);
            const int ci = ((ly + HALO) * SH + lx + HALO) * 2;
            const float d = __builtin_fabsf(s_tile[c][ci] - s_tile[c][ci + 1]);
            // the two loss maps' values, as the loss forward forms them (l1_w * |d| + ssim_w * val)
            const float l1_map = 1.0f * d + 0.0f * val;
            const float ssim_map = 0.0f * d + 1.0f * val;
            sq += (double)(l1_map * l1_map);   // eval.rs:49: powi_scalar(2) of the f32 map
            ss += (double)ssim_map;
        }
        __syncthreads();   // (the next channel's horizontal pass overwrites s_h)
    }
    sq = wave_sum(sq);
    ss = wave_sum(ss);
    if ((rank & 63) == 0) {
        s_red[0][rank >> 6] = sq;
        s_red[1][rank >> 6] = ss;
    }
    __syncthreads();
    if (rank == 0) {
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int wv = 0; wv < EVAL_WG / 64; ++wv) {
            t0 += s_red[0][wv];
            t1 += s_red[1][wv];
        }
        partial[blockIdx.y * gridDim.x + blockIdx.x] = make_double2(t0, t1);
    }
}

// the tiles' partials in index order -> metrics[3] = mse, psnr, ssim
__global__ __launch_bounds__(EVAL_FINAL_WG) void eval_final_kernel(const double2* __restrict__ partial, uint32_t tiles, double count,
                                                                   float* __restrict__ metrics) {
    __shared__ double s_red[2][EVAL_FINAL_WG / 64];
    double sq = 0.0, ss = 0.0;
#pragma unroll 4
    for (uint32_t i = threadIdx.x; i < tiles; i += EVAL_FINAL_WG) {   // (unrolled: the loads are in flight together, the adds stay in order)
        const double2 v = partial[i];
        sq += v.x;
        ss += v.y;
    }
    sq = wave_sum(sq);
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) {
        s_red[0][threadIdx.x >> 6] = sq;
        s_red[1][threadIdx.x >> 6] = ss;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int wv = 0; wv < EVAL_FINAL_WG / 64; ++wv) {
            t0 += s_red[0][wv];
            t1 += s_red[1][wv];
        }
        const float mse = (float)(t0 / count);
        // eval.rs:52: mse.recip().log() * 10.0 / LN_10, in f32
        const float psnr = logf(1.0f / mse) * 10.0f / 2.30258509299404568402f;
        metrics[0] = mse;
        metrics[1] = psnr;
        metrics[2] = (float)(t1 / count);
    }
}

static int launch_eval_metrics(bh_ctx* ctx, const float* img_hwc4, const uint32_t* gt_packed, uint32_t h, uint32_t w, float* metrics,
                               uint32_t* rgb8) {
    const uint32_t tiles_x = (w + LB - 1) / LB, tiles_y = (h + LB - 1) / LB;
    const uint32_t tiles = tiles_x * tiles_y;
    auto* partial = (double2*)ensure(ctx, SLOT_EVAL, (size_t)tiles * sizeof(double2));
    if (!partial) return BH_ERR_OOM;
    EvalArgs a;
    a.h = h;
    a.w = w;
    a.taps = gauss_taps();
    ProfScope ps(ctx, "EvalMetrics");
    hipLaunchKernelGGL(eval_tile_kernel, dim3(tiles_x, tiles_y), dim3(EVAL_WG), 0, ctx->stream, reinterpret_cast<const float4*>(img_hwc4), gt_packed, rgb8,
                       partial, a);
    BH_LAUNCH_CHECK(ctx, "eval_tile_kernel");
    hipLaunchKernelGGL(eval_final_kernel, dim3(1), dim3(EVAL_FINAL_WG), 0, ctx->stream, partial, tiles, (double)h * (double)w * 3.0, metrics);
    BH_LAUNCH_CHECK(ctx, "eval_final_kernel");
    return 0;
}

}  // namespace bh

using namespace bh;

extern "C" {

int bh_eval_metrics(bh_ctx* ctx, const float* img_hwc4, const uint32_t* gt_packed, uint32_t h, uint32_t w, float* metrics, uint32_t* rgb8) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!img_hwc4 || !gt_packed || !metrics || h == 0 || w == 0) return set_error(ctx, BH_ERR_INVALID_ARG, "eval_metrics: bad argument");
    if (reinterpret_cast<uintptr_t>(img_hwc4) & 15u) return set_error(ctx, BH_ERR_INVALID_ARG, "eval_metrics: img_hwc4 must be 16-byte aligned");
    if (w > 65520 || h > 65520) return set_error(ctx, BH_ERR_UNSUPPORTED, "eval_metrics: images larger than 65520 px per side are not supported");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return launch_eval_metrics(ctx, img_hwc4, gt_packed, h, w, metrics, rgb8);
}

int bh_eval_view(bh_ctx* ctx, const BhCamera* cam, uint32_t n, uint32_t sh_degree, const float* transforms, const float* sh_coeffs,
                 const float* raw_opacities, const float* min_scale, uint32_t flags, const uint32_t* gt_packed, float* metrics, uint32_t* rgb8) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!cam || !gt_packed || !metrics) return set_error(ctx, BH_ERR_INVALID_ARG, "eval_view: null argument");
    if (flags & ~(uint32_t)BH_FLAG_MIP) return set_error(ctx, BH_ERR_INVALID_ARG, "eval_view: BH_FLAG_MIP is the only flag");
    if (cam->tile_row_begin != 0 || cam->tile_row_end != 0) return set_error(ctx, BH_ERR_INVALID_ARG, "eval_view: the whole image is scored (no tile-row window)");
    if (n > 0 && (!transforms || !sh_coeffs || !raw_opacities)) return set_error(ctx, BH_ERR_INVALID_ARG, "eval_view: null splat tensor");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    // gaussian_splats.rs:379-386: the renderer sees fold_min_scale(params) when the splats carry a floor
    const float* r_t = transforms;
    const float* r_o = raw_opacities;
    if (min_scale && n > 0) {
        auto* folded = (float*)ensure(ctx, SLOT_LOD_FOLDED, (size_t)n * 11 * 4);
        if (!folded) return BH_ERR_OOM;
        ProfScope ps(ctx, "FoldMinScale");
        BH_TRY(launch_fold_min_scale(ctx, transforms, raw_opacities, min_scale, n, folded, folded + (size_t)n * 10));
        r_t = folded;
        r_o = folded + (size_t)n * 10;
    }
    // eval.rs:36-37: render_splats(.., Vec3::ZERO, TextureMode::Float) — the f32 image (RasterPass::Backward), complete lists, background 0
    const float bg[3] = {0.0f, 0.0f, 0.0f};
    BhRenderOut ro;
    BH_TRY(bh_render_forward(ctx, cam, n, sh_degree, r_t, sh_coeffs, r_o, bg, BH_FLAG_BWD_INFO | flags, &ro));
    return launch_eval_metrics(ctx, ro.out_img, gt_packed, cam->img_h, cam->img_w, metrics, rgb8);
}

}  // extern "C"
