// loss.hip — fused L1 + SSIM image loss (forward loss map, backward dL/dpred) on a
// packed rgba8 ground truth, plus the small layout / reduction helpers of the
// train step.
//
// Reference: brush-loss/src/lib.rs:45-661 (kernels :181 forward, :371 backward).
// Arithmetic follows the reference tap-pair accumulation order exactly; the
// Gaussian taps are evaluated on the host like the reference's comptime table.
//
// MI355X notes: 16x16 tiles for BOTH passes (the reference shrinks its backward to
// 8x8 to fit Apple's 32 KiB threadgroup memory; a CU here has 160 KiB), all five
// blurred moments staged through LDS once, and the kernels address pred / grads
// through (pixel stride, channel stride) so the train step can read the
// rasterizer's [H,W,4] image and write v_output [H,W,4] directly — the reference's
// HWC<->CHW permutes (lib.rs:1076,1103) disappear.
#include "device_ssim.h"

namespace bh {

// ---------------------------------------------------------------------------
// forward (lib.rs:181-359).  loss_map is always [C,H,W].
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(LB * LB) void image_loss_forward_kernel(const float* __restrict__ pred, const uint32_t* __restrict__ gt,
                                                                    float* __restrict__ loss_map, LossArgs a) {
    const uint32_t c = blockIdx.z;
    const int ty0 = blockIdx.y * LB, tx0 = blockIdx.x * LB;
    const int lx = threadIdx.x, ly = threadIdx.y;
    const int py = ty0 + ly, pxx = tx0 + lx;
    const size_t hw = (size_t)a.h * a.w;
    if (c == 3) {  // alpha-match plane: |pred.a - gt.a| (lib.rs:203-214)
        if (pxx < (int)a.w && py < (int)a.h) {
            const uint32_t p = (uint32_t)py * a.w + (uint32_t)pxx;
            const float ga = gt_channel(gt[p], 3);
            float v = __builtin_fabsf(pred[(size_t)3 * a.ch_stride + (size_t)p * a.pix_stride] - ga);
            if (a.mask) v = v * ga;
            loss_map[3 * hw + p] = v;
        }
        return;
    }
    __shared__ float s_tile[SH * SH * 2];
    __shared__ float s_h[SH * LB * 5];
    const int rank = ly * LB + lx;
    for (int i = rank; i < SH * SH; i += LB * LB) {
        const int r = i / SH, q = i % SH;
        float pv, ge;
        sample_pg(pred, gt, a, c, ty0 + r - HALO, tx0 + q - HALO, pv, ge);
        s_tile[i * 2] = pv;
        s_tile[i * 2 + 1] = ge;
    }
    __syncthreads();
    for (int r = ly; r < SH; r += LB) {
        float o[5];
        hblur5(s_tile, SH, r, lx + HALO, a.taps, o);
#pragma unroll
        for (int k = 0; k < 5; ++k) s_h[(r * LB + lx) * 5 + k] = o[k];
    }
    __syncthreads();
    if (pxx < (int)a.w && py < (int)a.h) {
        float o[5];
        vblur<5>(s_h, LB, ly + HALO, lx, a.taps, o);
        const float val = ssim_clamped(o);
        const int ci = ((ly + HALO) * SH + lx + HALO) * 2;
        const float p1 = s_tile[ci], p2 = s_tile[ci + 1];
        float lv = a.l1_w * __builtin_fabsf(p1 - p2) + a.ssim_w * val;
        const uint32_t p = (uint32_t)py * a.w + (uint32_t)pxx;
        if (a.mask) lv = lv * gt_channel(gt[p], 3);
        loss_map[(size_t)c * hw + p] = lv;
    }
}

// ---------------------------------------------------------------------------
// backward (lib.rs:371-661).  dl_dmap [C,H,W] or NULL (= constant chain per plane).
// dl_dpred is addressed with (pix_stride, ch_stride) like pred.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(LB * LB) void image_loss_backward_kernel(const float* __restrict__ pred, const uint32_t* __restrict__ gt,
                                                                     const float* __restrict__ dl_dmap, float dl_rgb, float dl_alpha,
                                                                     float* __restrict__ dl_dpred, LossArgs a) {
    const uint32_t c = blockIdx.z;
    const int ty0 = blockIdx.y * LB, tx0 = blockIdx.x * LB;
    const int lx = threadIdx.x, ly = threadIdx.y;
    const int py = ty0 + ly, pxx = tx0 + lx;
    const size_t hw = (size_t)a.h * a.w;
    if (c == 3) {  // lib.rs:392-412
        if (pxx < (int)a.w && py < (int)a.h) {
            const uint32_t p = (uint32_t)py * a.w + (uint32_t)pxx;
            const float ga = gt_channel(gt[p], 3);
            const size_t idx = (size_t)3 * a.ch_stride + (size_t)p * a.pix_stride;
            const float diff = pred[idx] - ga;
            const float sign = diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : 0.0f);
            float chain = dl_dmap ? dl_dmap[3 * hw + p] : dl_alpha;
            if (a.mask) chain = chain * ga;
            dl_dpred[idx] = sign * chain;
        }
        return;
    }
    __shared__ float s_ext[EXT * EXT * 2];   // (pred, gt) with a 2*HALO apron
    __shared__ float s_h[EXT * SH * 5];      // horizontally blurred moments
    __shared__ float s_part[SH * SH * 3];    // chain * (dmu1, dsigma1, dsigma12)
    __shared__ float s_h2[SH * LB * 3];      // horizontally blurred partials
    const int rank = ly * LB + lx;
    for (int i = rank; i < EXT * EXT; i += LB * LB) {
        const int r = i / EXT, q = i % EXT;
        float pv, ge;
        sample_pg(pred, gt, a, c, ty0 + r - 2 * HALO, tx0 + q - 2 * HALO, pv, ge);
        s_ext[i * 2] = pv;
        s_ext[i * 2 + 1] = ge;
    }
    __syncthreads();
    for (int i = rank; i < EXT * SH; i += LB * LB) {
        const int r = i / SH, q = i % SH;
        float o[5];
        hblur5(s_ext, EXT, r, q + HALO, a.taps, o);
#pragma unroll
        for (int k = 0; k < 5; ++k) s_h[i * 5 + k] = o[k];
    }
    __syncthreads();
    for (int i = rank; i < SH * SH; i += LB * LB) {
        const int r = i / SH, q = i % SH;
        float o[5];
        vblur<5>(s_h, SH, r + HALO, q, a.taps, o);
        const float mu1 = o[0], mu2 = o[2];
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2;
        const float s1 = __builtin_fmaxf(0.0f, o[1] - mu1_sq), s2 = __builtin_fmaxf(0.0f, o[3] - mu2_sq);
        const float s12 = o[4] - mu1 * mu2;
        const float A = mu1_sq + mu2_sq + SSIM_C1;
        const float B = s1 + s2 + SSIM_C2;
        const float c_top = 2.0f * mu1 * mu2 + SSIM_C1;
        const float d_top = 2.0f * s12 + SSIM_C2;
        const float inv_ab = 1.0f / (A * B);
        const float cd = c_top * d_top * inv_ab;
        const bool clamped = cd < -1.0f || cd > 1.0f;
        const float dmu1 = clamped ? 0.0f : 2.0f * mu2 * inv_ab * (d_top - c_top) - 2.0f * mu1 * cd * (1.0f / A - 1.0f / B);
        const float ds1 = clamped ? 0.0f : -cd / B;
        const float ds12 = clamped ? 0.0f : 2.0f * c_top * inv_ab;
        const int gy = ty0 + r - HALO, gx = tx0 + q - HALO;
        float chain = 0.0f;
        if (gy >= 0 && gx >= 0 && gy < (int)a.h && gx < (int)a.w) {
            const uint32_t p = (uint32_t)gy * a.w + (uint32_t)gx;
            chain = dl_dmap ? dl_dmap[(size_t)c * hw + p] : dl_rgb;
            if (a.mask) chain = chain * gt_channel(gt[p], 3);
        }
        s_part[i * 3] = dmu1 * chain;
        s_part[i * 3 + 1] = ds1 * chain;
        s_part[i * 3 + 2] = ds12 * chain;
    }
    __syncthreads();
    for (int r = ly; r < SH; r += LB) {
        float a0 = 0, a1 = 0, a2 = 0;
        const int col = lx + HALO;
#pragma unroll
        for (int d = 1; d < 6; ++d) {
            const float wd = a.taps.w[5 - d];
            const float* l = &s_part[(r * SH + col - d) * 3];
            const float* rr = &s_part[(r * SH + col + d) * 3];
            a0 += (l[0] + rr[0]) * wd;
            a1 += (l[1] + rr[1]) * wd;
            a2 += (l[2] + rr[2]) * wd;
        }
        const float* cc = &s_part[(r * SH + col) * 3];
        a0 += cc[0] * a.taps.w[5];
        a1 += cc[1] * a.taps.w[5];
        a2 += cc[2] * a.taps.w[5];
        s_h2[(r * LB + lx) * 3] = a0;
        s_h2[(r * LB + lx) * 3 + 1] = a1;
        s_h2[(r * LB + lx) * 3 + 2] = a2;
    }
    __syncthreads();
    if (pxx < (int)a.w && py < (int)a.h) {
        float s[3];
        vblur<3>(s_h2, LB, ly + HALO, lx, a.taps, s);
        const int ci = ((ly + 2 * HALO) * EXT + lx + 2 * HALO) * 2;
        const float p1 = s_ext[ci], ge = s_ext[ci + 1];
        const float ssim_grad = s[0] + (2.0f * p1) * s[1] + ge * s[2];
        const float diff = p1 - ge;
        const float l1_sign = diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : 0.0f);
        const uint32_t p = (uint32_t)py * a.w + (uint32_t)pxx;
        float chain_c = dl_dmap ? dl_dmap[(size_t)c * hw + p] : dl_rgb;
        if (a.mask) chain_c = chain_c * gt_channel(gt[p], 3);
        dl_dpred[(size_t)c * a.ch_stride + (size_t)p * a.pix_stride] = a.ssim_w * ssim_grad + a.l1_w * l1_sign * chain_c;
    }
}

static LossArgs make_args(uint32_t h, uint32_t w, const BhLossConfig& cfg, uint32_t pix_stride, uint32_t ch_stride) {
    LossArgs a;
    a.h = h; a.w = w;
    a.l1_w = cfg.l1_weight; a.ssim_w = cfg.ssim_weight;
    a.bg[0] = cfg.bg[0]; a.bg[1] = cfg.bg[1]; a.bg[2] = cfg.bg[2];
    a.composite = cfg.composite_bg; a.mask = cfg.mask;
    a.pix_stride = pix_stride; a.ch_stride = ch_stride;
    a.taps = gauss_taps();
    return a;
}

static int launch_image_loss_forward_strided(bh_ctx* ctx, const float* pred, uint32_t pix_stride, uint32_t ch_stride, const uint32_t* gt,
                                      uint32_t channels, uint32_t h, uint32_t w, const BhLossConfig& cfg, float* loss_map) {
    if (channels != 3 && channels != 4) return set_error(ctx, BH_ERR_INVALID_ARG, "image loss: channels must be 3 or 4");
    const LossArgs a = make_args(h, w, cfg, pix_stride, ch_stride);
    const dim3 grid((w + LB - 1) / LB, (h + LB - 1) / LB, channels), block(LB, LB);
    hipLaunchKernelGGL(image_loss_forward_kernel, grid, block, 0, ctx->stream, pred, gt, loss_map, a);
    BH_LAUNCH_CHECK(ctx, "image_loss_forward_kernel");
    return 0;
}

static int launch_image_loss_backward_strided(bh_ctx* ctx, const float* pred, uint32_t pix_stride, uint32_t ch_stride, const uint32_t* gt,
                                       const float* dl_dmap, float dl_rgb, float dl_alpha, uint32_t channels, uint32_t h, uint32_t w,
                                       const BhLossConfig& cfg, float* dl_dpred) {
    if (channels != 3 && channels != 4) return set_error(ctx, BH_ERR_INVALID_ARG, "image loss: channels must be 3 or 4");
    const LossArgs a = make_args(h, w, cfg, pix_stride, ch_stride);
    const dim3 grid((w + LB - 1) / LB, (h + LB - 1) / LB, channels), block(LB, LB);
    hipLaunchKernelGGL(image_loss_backward_kernel, grid, block, 0, ctx->stream, pred, gt, dl_dmap, dl_rgb, dl_alpha, dl_dpred, a);
    BH_LAUNCH_CHECK(ctx, "image_loss_backward_kernel");
    return 0;
}

int launch_image_loss_forward(bh_ctx* ctx, const float* pred, const uint32_t* gt, uint32_t channels, uint32_t h, uint32_t w,
                              const BhLossConfig& cfg, float* loss_map) {
    return launch_image_loss_forward_strided(ctx, pred, 1, h * w, gt, channels, h, w, cfg, loss_map);
}

int launch_image_loss_backward(bh_ctx* ctx, const float* pred, const uint32_t* gt, const float* dl_dmap, float dl_const,
                               uint32_t channels, uint32_t h, uint32_t w, const BhLossConfig& cfg, float* dl_dpred) {
    return launch_image_loss_backward_strided(ctx, pred, 1, h * w, gt, dl_dmap, dl_const, dl_const, channels, h, w, cfg, dl_dpred);
}

}  // namespace bh
