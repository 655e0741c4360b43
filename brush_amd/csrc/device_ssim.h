// device_ssim.h — the SSIM arithmetic of the image-loss kernels (brush-loss/src/lib.rs:45-359), shared by the loss
// (loss.hip) and the held-out metrics (eval.hip) so that both compute the same SSIM map, bit for bit.  The library is
// built with -ffp-contract=off: every helper below is the reference's tap-pair accumulation order, one rounding per op.
#pragma once
#include <cmath>

#include "context.h"

namespace bh {

constexpr int LB = 16;          // block edge
constexpr int HALO = 5;
constexpr int SH = LB + 2 * HALO;   // 26
constexpr int EXT = LB + 4 * HALO;  // 36
constexpr float SSIM_C1 = 0.01f * 0.01f;
constexpr float SSIM_C2 = 0.03f * 0.03f;
constexpr float INV_255 = 1.0f / 255.0f;

struct Taps { float w[11]; };

// lib.rs:55-68
static Taps gauss_taps() {
    Taps g;
    const float sigma = 1.5f;
    float sum = 0.0f;
    for (int i = 0; i < 11; ++i) {
        const float x = (float)i - 5.0f;
        g.w[i] = expf(-x * x / (2.0f * sigma * sigma));
        sum += g.w[i];
    }
    for (int i = 0; i < 11; ++i) g.w[i] /= sum;
    return g;
}

struct LossArgs {
    uint32_t h, w;
    float l1_w, ssim_w;
    float bg[3];
    int composite, mask;
    // addressing of pred-like tensors: idx = c * ch_stride + (y * w + x) * pix_stride
    uint32_t pix_stride, ch_stride;
    Taps taps;
};

BH_DEV float gt_channel(uint32_t val, uint32_t c) { return (float)((val >> (c * 8u)) & 0xffu) * INV_255; }

// (pred, gt_eff) sample with zero padding (lib.rs:110-176)
BH_DEV void sample_pg(const float* __restrict__ pred, const uint32_t* __restrict__ gt, const LossArgs& a, uint32_t c,
                      int y, int x, float& pv, float& ge) {
    if (y < 0 || x < 0 || y >= (int)a.h || x >= (int)a.w) {
        pv = 0.0f;
        ge = 0.0f;
        return;
    }
    const uint32_t p = (uint32_t)y * a.w + (uint32_t)x;
    pv = pred[(size_t)c * a.ch_stride + (size_t)p * a.pix_stride];
    const uint32_t val = gt[p];
    const float gc = gt_channel(val, c), ga = gt_channel(val, 3);
    ge = a.composite ? gc + (1.0f - ga) * a.bg[c] : gc;
}

// horizontal 11-tap blur of the five moments at LDS tile position (row, col) of a
// tile with row pitch `pitch` holding interleaved (pred, gt) pairs
BH_DEV void hblur5(const float* tile, int pitch, int row, int col, const Taps& g, float o[5]) {
    float sx = 0, sx2 = 0, sy = 0, sy2 = 0, sxy = 0;
#pragma unroll
    for (int d = 1; d < 6; ++d) {
        const float wd = g.w[5 - d];
        const float xl = tile[(row * pitch + col - d) * 2], yl = tile[(row * pitch + col - d) * 2 + 1];
        const float xr = tile[(row * pitch + col + d) * 2], yr = tile[(row * pitch + col + d) * 2 + 1];
        sx += (xl + xr) * wd;
        sx2 += (xl * xl + xr * xr) * wd;
        sy += (yl + yr) * wd;
        sy2 += (yl * yl + yr * yr) * wd;
        sxy += (xl * yl + xr * yr) * wd;
    }
    const float xc = tile[(row * pitch + col) * 2], yc = tile[(row * pitch + col) * 2 + 1];
    const float wc = g.w[5];
    sx += xc * wc;
    sx2 += xc * xc * wc;
    sy += yc * wc;
    sy2 += yc * yc * wc;
    sxy += xc * yc * wc;
    o[0] = sx; o[1] = sx2; o[2] = sy; o[3] = sy2; o[4] = sxy;
}

// vertical 11-tap blur over a [rows][cols][K] LDS array
template <int K>
BH_DEV void vblur(const float* buf, int cols, int row, int col, const Taps& g, float o[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) o[k] = 0.0f;
#pragma unroll
    for (int d = 1; d < 6; ++d) {
        const float wd = g.w[5 - d];
        const float* t = &buf[((row - d) * cols + col) * K];
        const float* b = &buf[((row + d) * cols + col) * K];
#pragma unroll
        for (int k = 0; k < K; ++k) o[k] += (t[k] + b[k]) * wd;
    }
    const float* c = &buf[(row * cols + col) * K];
#pragma unroll
    for (int k = 0; k < K; ++k) o[k] += c[k] * g.w[5];
}

// the forward's SSIM value of one pixel from its five blurred moments (lib.rs:330-346), clamped to [-1, 1]
BH_DEV float ssim_clamped(const float o[5]) {
    const float mu1 = o[0], mu2 = o[2];
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2;
    const float s1 = __builtin_fmaxf(0.0f, o[1] - mu1_sq), s2 = __builtin_fmaxf(0.0f, o[3] - mu2_sq);
    const float s12 = o[4] - mu1 * mu2;
    const float A = mu1_sq + mu2_sq + SSIM_C1;
    const float B = s1 + s2 + SSIM_C2;
    const float c_top = 2.0f * mu1 * mu2 + SSIM_C1;
    const float d_top = 2.0f * s12 + SSIM_C2;
    const float raw = (c_top * d_top) / (A * B);
    return clampf(raw, -1.0f, 1.0f);
}

}  // namespace bh
