// lpips.hip — LPIPS (VGG16) perceptual distance of a rendered image to its packed ground truth, and its data gradient.
//
// Reference: LpipsModel::lpips (crates/lpips/src/lib.rs), used by SplatTrainer::step when lpips_loss_weight > 0
// (brush-train/src/train.rs:153, 265-273) on unpack_gt_rgb(gt_packed, composite_bg) (brush-loss/src/lib.rs:662-696):
//   x     = ((img * 2 - 1) - shift) / scale              shift (-0.030, -0.088, -0.188), scale (0.458, 0.448, 0.450), true divide
//   5 blocks of (2, 2, 3, 3, 3) conv3x3 (pad 1, bias) + ReLU, 64 / 128 / 256 / 512 / 512 channels; a 2x2 stride-2 max-pool (odd
//   sizes floor) in front of blocks 2..5
//   LPIPS = sum_b mean_{pixels} head_b . (n(a_b) - n(g_b))^2,   n(v) = v / (sqrt(sum_c v^2) + 1e-10),   head_b a bias-free 1x1 conv
//
// Numerics: exact f32.  The convs run on v_mfma_f32_32x32x2_f32 (f32 operands, f32 accumulate, one rounding per product: a
// k-ordered fmaf chain over k = (tap, channel)); no 16-bit operand anywhere.  The per-pixel norm / head terms are f32 like the
// reference's; the spatial and block sums are f64 in a fixed order (waves, blocks, then partials in index order in one block), so
// repeated calls are bit-identical and no float atomics are used.
//
// Layout: activations NHWC f32.  Every 3x3 conv is an implicit GEMM, M = pixels, N = Cout, K = 9 Cin in (tap, channel) order; the
// data gradient of a stride-1 pad-1 3x3 conv is the same GEMM over the gradient with W'[ci][co][2-ky][2-kx], so bh_lpips_create
// stores both packings and one kernel body serves both directions (epilogue: bias + ReLU, or the ReLU mask of the layer's input).
// conv1_1 (Cin 3) and the gradient into the image (Cout 3) are too thin for a 32x32 MFMA tile: they run on the VALU.
//
// Memory (f32 counts from the shapes, not measured; P_b the pixels of block b, P_1 = H W): value_and_grad keeps pred's 13 conv
// outputs (270 P_1) and its 4 pooled block inputs (30 P_1), GT's 5 block outputs (122 P_1), both normalised inputs (6 P_1) and a
// pair of P_1 x 64 scratch / gradient buffers (128 P_1): ~556 P_1 floats, 4.6 GB at 1920x1080 and 18.4 GB at 3840x2160.
// bh_lpips_forward keeps only the 5 block outputs of each image, the inputs and the pair: ~378 P_1 floats, 3.1 GB at 1080p.
#include "context.h"

#include <cmath>
#include <vector>

namespace bh {

constexpr int LP_LAYERS = 13;
constexpr int LP_BLOCKS = 5;
constexpr int LP_CIN[LP_LAYERS] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int LP_COUT[LP_LAYERS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int LP_BLOCK_OF[LP_LAYERS] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};
constexpr int LP_FIRST[LP_BLOCKS] = {0, 2, 4, 7, 10};
constexpr int LP_LAST[LP_BLOCKS] = {1, 3, 6, 9, 12};
constexpr int LP_CH[LP_BLOCKS] = {64, 128, 256, 512, 512};
constexpr float LP_SHIFT[3] = {-0.030f, -0.088f, -0.188f};
constexpr float LP_SCALE[3] = {0.458f, 0.448f, 0.450f};

constexpr int LP_WG = 256;   // every kernel here: 4 waves
constexpr int LP_BK = 32;    // K per LDS stage of the implicit GEMM: one tap, 32 channels

typedef float f32x16 __attribute__((ext_vector_type(16)));

}  // namespace bh

// the model: both packings of every conv, biases and heads (device), canonical layout documented in brush_hip_lpips.h
struct bh_lpips {
    int device = 0;
    float* mem = nullptr;
    float* fwd[bh::LP_LAYERS] = {};     // [9 Cin][Cout]: B[(tap Cin + ci) Cout + co] = W[co][ci][ky][kx], tap = 3 ky + kx
    float* dgrad[bh::LP_LAYERS] = {};   // [9 Cout][Cin]: B[(tap Cout + co) Cin + ci] = W[co][ci][2 - ky][2 - kx]
    float* bias[bh::LP_LAYERS] = {};
    float* head[bh::LP_BLOCKS] = {};
};

namespace bh {

// ---- input normalisation -----------------------------------------------------------------------------------------------------
BH_DEV float lp_norm_in(float v, int c) { return (v * 2.0f - 1.0f - LP_SHIFT[c]) / LP_SCALE[c]; }

__global__ __launch_bounds__(LP_WG) void lpips_input_pred(const float4* __restrict__ img, float* __restrict__ x, uint32_t P) {
    const uint32_t p = blockIdx.x * LP_WG + threadIdx.x;
    if (p >= P) return;
    const float4 v = img[p];
    x[p * 3 + 0] = lp_norm_in(v.x, 0);
    x[p * 3 + 1] = lp_norm_in(v.y, 1);
    x[p * 3 + 2] = lp_norm_in(v.z, 2);
}

// unpack_gt_rgb (brush-loss/src/lib.rs:662-696): byte * (1/255), optionally + (1 - a) * bg; then the same normalisation
__global__ __launch_bounds__(LP_WG) void lpips_input_gt(const uint32_t* __restrict__ gt, float* __restrict__ x, uint32_t P, int composite, float bg0,
                                                        float bg1, float bg2) {
    const uint32_t p = blockIdx.x * LP_WG + threadIdx.x;
    if (p >= P) return;
    const uint32_t val = gt[p];
    const float inv = 1.0f / 255.0f;
    float r = (float)(val & 0xffu) * inv, g = (float)((val >> 8) & 0xffu) * inv, b = (float)((val >> 16) & 0xffu) * inv;
    if (composite) {
        const float inv_a = 1.0f - (float)(val >> 24) * inv;
        r = r + inv_a * bg0;
        g = g + inv_a * bg1;
        b = b + inv_a * bg2;
    }
    x[p * 3 + 0] = lp_norm_in(r, 0);
    x[p * 3 + 1] = lp_norm_in(g, 1);
    x[p * 3 + 2] = lp_norm_in(b, 2);
}

// ---- conv1_1 forward (Cin 3): one pixel per thread, 64 accumulators, k = (tap, channel) in order --------------------------------
__global__ __launch_bounds__(LP_WG) void lpips_conv3x3_fwd_c3(const float* __restrict__ x, const float* __restrict__ B /*[27][64]*/,
                                                              const float* __restrict__ bias, float* __restrict__ out, int H, int W) {
    __shared__ float s_b[27 * 64];
    __shared__ float s_bias[64];
    for (int i = threadIdx.x; i < 27 * 64; i += LP_WG) s_b[i] = B[i];
    if (threadIdx.x < 64) s_bias[threadIdx.x] = bias[threadIdx.x];
    __syncthreads();
    const size_t p = (size_t)blockIdx.x * LP_WG + threadIdx.x;
    if (p >= (size_t)H * W) return;
    const int y = (int)(p / W), xx = (int)(p % W);
    float acc[64];
#pragma unroll
    for (int c = 0; c < 64; ++c) acc[c] = 0.0f;
    for (int tap = 0; tap < 9; ++tap) {
        const int yy = y + tap / 3 - 1, xs = xx + tap % 3 - 1;
        const bool in = yy >= 0 && yy < H && xs >= 0 && xs < W;
        for (int ci = 0; ci < 3; ++ci) {
            const float v = in ? x[((size_t)yy * W + xs) * 3 + ci] : 0.0f;
            const float* b = s_b + (tap * 3 + ci) * 64;
#pragma unroll
            for (int c = 0; c < 64; ++c) acc[c] = fmaf(v, b[c], acc[c]);
        }
    }
    float4* o = reinterpret_cast<float4*>(out + p * 64);
#pragma unroll
    for (int c = 0; c < 64; c += 4) {
        float4 r;
        r.x = fmaxf(acc[c] + s_bias[c], 0.0f);
        r.y = fmaxf(acc[c + 1] + s_bias[c + 1], 0.0f);
        r.z = fmaxf(acc[c + 2] + s_bias[c + 2], 0.0f);
        r.w = fmaxf(acc[c + 3] + s_bias[c + 3], 0.0f);
        o[c / 4] = r;
    }
}

// ---- conv1_1 data gradient (Cout' 3) chained into the image: v_output[p].rgb += 2 (dL/dx) / scale ------------------------------
__global__ __launch_bounds__(LP_WG) void lpips_conv3x3_dgrad_c3(const float* __restrict__ g /*[P][64]*/, const float* __restrict__ B /*[9*64][3]*/,
                                                                float* __restrict__ v_output, int H, int W) {
    __shared__ float s_b[9 * 64 * 3];
    for (int i = threadIdx.x; i < 9 * 64 * 3; i += LP_WG) s_b[i] = B[i];
    __syncthreads();
    const size_t p = (size_t)blockIdx.x * LP_WG + threadIdx.x;
    if (p >= (size_t)H * W) return;
    const int y = (int)(p / W), xx = (int)(p % W);
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    for (int tap = 0; tap < 9; ++tap) {
        const int yy = y + tap / 3 - 1, xs = xx + tap % 3 - 1;
        if (yy < 0 || yy >= H || xs < 0 || xs >= W) continue;   // (zero padding: the skipped products are exact zeros)
        const float4* src = reinterpret_cast<const float4*>(g + ((size_t)yy * W + xs) * 64);
        const float* b = s_b + tap * 64 * 3;
#pragma unroll 4
        for (int q = 0; q < 16; ++q) {
            const float4 v = src[q];
            const float* bb = b + q * 12;
            a0 = fmaf(v.x, bb[0], a0); a1 = fmaf(v.x, bb[1], a1); a2 = fmaf(v.x, bb[2], a2);
            a0 = fmaf(v.y, bb[3], a0); a1 = fmaf(v.y, bb[4], a1); a2 = fmaf(v.y, bb[5], a2);
            a0 = fmaf(v.z, bb[6], a0); a1 = fmaf(v.z, bb[7], a1); a2 = fmaf(v.z, bb[8], a2);
            a0 = fmaf(v.w, bb[9], a0); a1 = fmaf(v.w, bb[10], a1); a2 = fmaf(v.w, bb[11], a2);
        }
    }
    // x = ((v * 2 - 1) - shift) / scale: dL/dv = (dL/dx / scale) * 2, as autodiff forms it
    float* o = v_output + p * 4;
    o[0] = o[0] + (a0 / LP_SCALE[0]) * 2.0f;
    o[1] = o[1] + (a1 / LP_SCALE[1]) * 2.0f;
    o[2] = o[2] + (a2 / LP_SCALE[2]) * 2.0f;
}

// ---- the implicit-GEMM 3x3 conv on f32 MFMA ---------------------------------------------------------------------------------
// Block: 4 waves as 2 (M) x 2 (N), each wave WM x WN tiles of 32x32 (v_mfma_f32_32x32x2_f32), so BM = 64 WM pixels by BN = 64 WN
// output channels.  K steps of 32 (one tap, 32 input channels) through LDS, the next step's global loads in registers while the
// current one is multiplied.  LDS holds A as [k][m] and B as [k][n]: an MFMA operand read is 32 consecutive floats per half-wave.
// Fragment maps (32x32x2 f32): lane l holds A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]; D register r of lane l is
// D[row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][col = l & 31].
// DGRAD = false: out = relu(acc + bias[n]);  DGRAD = true: out = epi[m][n] > 0 ? acc : 0 (epi = the layer input's activation).
template <int WM, int WN, bool DGRAD>
BH_DEV void conv3x3_body(const float* __restrict__ in, const float* __restrict__ B, const float* __restrict__ epi, float* __restrict__ out, int H,
                         int W, int Cin, int Cout) {
    constexpr int BM = 64 * WM, BN = 64 * WN;
    constexpr int LDA = BM + 4, LDB = BN + 4;
    constexpr int A_LD = BM * LP_BK / 4 / LP_WG;   // float4 loads per thread per K step
    constexpr int B_LD = BN * LP_BK / 4 / LP_WG;
    __shared__ float s_a[LP_BK * LDA];
    __shared__ float s_b[LP_BK * LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = H * W;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    // this thread's A loads: pixel (idx >> 3) of the tile, channel quad (idx & 7)
    int py[A_LD], px[A_LD];
#pragma unroll
    for (int i = 0; i < A_LD; ++i) {
        const int m = m0 + ((tid + LP_WG * i) >> 3);
        py[i] = m < M ? m / W : -0x40000000;   // (a pixel past the end: every tap reads as padding)
        px[i] = m < M ? m % W : 0;
    }
    const int kq = tid & 7;
    const int csteps = Cin / LP_BK, nk = 9 * csteps;
    float4 ra[A_LD], rb[B_LD];
    auto load = [&](int ks) {
        const int tap = ks / csteps, c0 = (ks - tap * csteps) * LP_BK;
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
#pragma unroll
        for (int i = 0; i < A_LD; ++i) {
            const int yy = py[i] + dy, xx = px[i] + dx;
            if (yy >= 0 && yy < H && xx >= 0 && xx < W)
                ra[i] = *reinterpret_cast<const float4*>(in + ((size_t)yy * W + xx) * Cin + c0 + 4 * kq);
            else
                ra[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        const float* bk = B + (size_t)ks * LP_BK * Cout + n0;
#pragma unroll
        for (int i = 0; i < B_LD; ++i) {
            const int idx = tid + LP_WG * i;
            const int r = idx / (BN / 4), c4 = idx % (BN / 4);
            rb[i] = *reinterpret_cast<const float4*>(bk + (size_t)r * Cout + 4 * c4);
        }
    };
    f32x16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    const int wm0 = (wave & 1) * 32 * WM, wn0 = (wave >> 1) * 32 * WN;
    const int lr = lane & 31, lk = lane >> 5;
    load(0);
    for (int ks = 0; ks < nk; ++ks) {
#pragma unroll
        for (int i = 0; i < A_LD; ++i) {
            const int m = (tid + LP_WG * i) >> 3;
            s_a[(4 * kq + 0) * LDA + m] = ra[i].x;
            s_a[(4 * kq + 1) * LDA + m] = ra[i].y;
            s_a[(4 * kq + 2) * LDA + m] = ra[i].z;
            s_a[(4 * kq + 3) * LDA + m] = ra[i].w;
        }
#pragma unroll
        for (int i = 0; i < B_LD; ++i) {
            const int idx = tid + LP_WG * i;
            const int r = idx / (BN / 4), c4 = idx % (BN / 4);
            *reinterpret_cast<float4*>(&s_b[r * LDB + 4 * c4]) = rb[i];
        }
        __syncthreads();
        if (ks + 1 < nk) load(ks + 1);
#pragma unroll
        for (int kk = 0; kk < LP_BK / 2; ++kk) {
            float a[WM], b[WN];
#pragma unroll
            for (int i = 0; i < WM; ++i) a[i] = s_a[(2 * kk + lk) * LDA + wm0 + 32 * i + lr];
#pragma unroll
            for (int j = 0; j < WN; ++j) b[j] = s_b[(2 * kk + lk) * LDB + wn0 + 32 * j + lr];
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        const int n = n0 + wn0 + 32 * j + lr;
        const float bn = DGRAD ? 0.0f : epi[n];
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (m >= M) continue;
                const size_t o = (size_t)m * Cout + n;
                float v = acc[i][j][r];
                if (DGRAD) v = epi[o] > 0.0f ? v : 0.0f;
                else v = fmaxf(v + bn, 0.0f);
                out[o] = v;
            }
    }
}

template <int WM, int WN>
__global__ __launch_bounds__(LP_WG) void lpips_conv3x3_fwd(const float* __restrict__ in, const float* __restrict__ B, const float* __restrict__ bias,
                                                           float* __restrict__ out, int H, int W, int Cin, int Cout) {
    conv3x3_body<WM, WN, false>(in, B, bias, out, H, W, Cin, Cout);
}

template <int WM, int WN>
__global__ __launch_bounds__(LP_WG) void lpips_conv3x3_dgrad(const float* __restrict__ in, const float* __restrict__ B, const float* __restrict__ mask,
                                                             float* __restrict__ out, int H, int W, int Cin, int Cout) {
    conv3x3_body<WM, WN, true>(in, B, mask, out, H, W, Cin, Cout);
}

// ---- 2x2 stride-2 max-pool (floor): forward, and its backward as a gather (every input element written once) -------------------
// ties go to the first maximum of the window in row-major order (strict >), as torch's max_pool2d picks it
__global__ __launch_bounds__(LP_WG) void lpips_pool_fwd(const float4* __restrict__ in, float4* __restrict__ out, int H, int W, int C4) {
    const int Ho = H / 2, Wo = W / 2;
    const size_t i = (size_t)blockIdx.x * LP_WG + threadIdx.x;
    if (i >= (size_t)Ho * Wo * C4) return;
    const int c = (int)(i % C4);
    const size_t po = i / C4;
    const int oy = (int)(po / Wo), ox = (int)(po % Wo);
    const size_t p00 = ((size_t)(2 * oy) * W + 2 * ox) * C4 + c;
    float4 m = in[p00];
    const float4 v[3] = {in[p00 + C4], in[p00 + (size_t)W * C4], in[p00 + (size_t)W * C4 + C4]};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        m.x = v[k].x > m.x ? v[k].x : m.x;
        m.y = v[k].y > m.y ? v[k].y : m.y;
        m.z = v[k].z > m.z ? v[k].z : m.z;
        m.w = v[k].w > m.w ? v[k].w : m.w;
    }
    out[i] = m;
}

BH_DEV int argmax4(float a, float b, float c, float d) {
    int k = 0;
    float m = a;
    if (b > m) { m = b; k = 1; }
    if (c > m) { m = c; k = 2; }
    if (d > m) { k = 3; }
    return k;
}

__global__ __launch_bounds__(LP_WG) void lpips_pool_bwd(const float* __restrict__ act /*[H,W,C]*/, const float* __restrict__ g_out /*[Ho,Wo,C]*/,
                                                        float* __restrict__ g_in /*[H,W,C]*/, int H, int W, int C) {
    const int Ho = H / 2, Wo = W / 2;
    const size_t i = (size_t)blockIdx.x * LP_WG + threadIdx.x;
    if (i >= (size_t)H * W * C) return;
    const int c = (int)(i % C);
    const size_t p = i / C;
    const int y = (int)(p / W), x = (int)(p % W);
    const int oy = y >> 1, ox = x >> 1;
    float g = 0.0f;
    if (oy < Ho && ox < Wo) {
        const size_t p00 = ((size_t)(2 * oy) * W + 2 * ox) * C + c;
        const int k = argmax4(act[p00], act[p00 + C], act[p00 + (size_t)W * C], act[p00 + (size_t)W * C + C]);
        if (k == (y & 1) * 2 + (x & 1)) g = g_out[((size_t)oy * Wo + ox) * C + c];
    }
    g_in[i] = g;
}

// ---- per block: normalise, difference, head, spatial sum (f64 partials per workgroup), and the pred side's backward -----------
BH_DEV double lp_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// One pixel per group of LP_G lanes, each lane a float4 of channels every 4 LP_G: coalesced loads and stores of the NHWC rows.
// Channel sums are a fixed xor butterfly inside the group (every lane ends with the same value, the order does not depend on
// scheduling).
constexpr int LP_G = 16;
constexpr int LP_PIX = LP_WG / LP_G;   // pixels per workgroup of the head kernels

BH_DEV float lp_group_sum(float v) {
#pragma unroll
    for (int off = LP_G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, LP_G);
    return v;
}

BH_DEV float lp_sq4(float4 q) { return ((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w; }

BH_DEV void lp_norms(const float* pa, const float* pb, int C, int l, float& sa, float& sb) {
    float xa = 0.0f, xb = 0.0f;
    for (int c = 4 * l; c < C; c += 4 * LP_G) {
        xa = xa + lp_sq4(*reinterpret_cast<const float4*>(pa + c));
        xb = xb + lp_sq4(*reinterpret_cast<const float4*>(pb + c));
    }
    sa = lp_group_sum(xa);
    sb = lp_group_sum(xb);
}

__global__ __launch_bounds__(LP_WG) void lpips_head_fwd(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ head,
                                                        uint32_t P, int C, double* __restrict__ partial) {
    __shared__ double s_red[LP_PIX];
    const int g = threadIdx.x / LP_G, l = threadIdx.x % LP_G;
    const uint32_t p = blockIdx.x * LP_PIX + g;
    double v = 0.0;
    if (p < P) {   // (uniform over the group)
        const float* pa = a + (size_t)p * C;
        const float* pb = b + (size_t)p * C;
        float sa, sb;
        lp_norms(pa, pb, C, l, sa, sb);
        const float na = sqrtf(sa) + 1e-10f, nb = sqrtf(sb) + 1e-10f;
        float s = 0.0f;
        for (int c = 4 * l; c < C; c += 4 * LP_G) {
            const float4 qa = *reinterpret_cast<const float4*>(pa + c), qb = *reinterpret_cast<const float4*>(pb + c);
            const float4 h = *reinterpret_cast<const float4*>(head + c);
            const float d0 = qa.x / na - qb.x / nb, d1 = qa.y / na - qb.y / nb, d2 = qa.z / na - qb.z / nb, d3 = qa.w / na - qb.w / nb;
            s = s + (((h.x * (d0 * d0) + h.y * (d1 * d1)) + h.z * (d2 * d2)) + h.w * (d3 * d3));
        }
        v = (double)lp_group_sum(s);
    }
    if (l == 0) s_red[g] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < LP_PIX; ++i) t += s_red[i];
        partial[blockIdx.x] = t;
    }
}

// g[p][k] (+)= (a_k > 0) * dL/da_k of this block's term, scale = weight / P (the mean's factor)
__global__ __launch_bounds__(LP_WG) void lpips_head_bwd(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ head,
                                                        uint32_t P, int C, float scale, int accumulate, float* __restrict__ g) {
    const int gi = threadIdx.x / LP_G, l = threadIdx.x % LP_G;
    const uint32_t p = blockIdx.x * LP_PIX + gi;
    if (p >= P) return;   // (uniform over the group; no barrier below)
    const float* pa = a + (size_t)p * C;
    const float* pb = b + (size_t)p * C;
    float* pg = g + (size_t)p * C;
    float sa, sb;
    lp_norms(pa, pb, C, l, sa, sb);
    const float ra = sqrtf(sa);
    const float na = ra + 1e-10f, nb = sqrtf(sb) + 1e-10f;
    // u = a / na, du/da_k = e_k / na - a (a_k / ra) / na^2;  gu_c = scale * head_c * 2 d_c
    auto gu = [&](float x, float y, float h) { return (scale * h) * (2.0f * (x / na - y / nb)); };
    float t = 0.0f;
    for (int c = 4 * l; c < C; c += 4 * LP_G) {
        const float4 qa = *reinterpret_cast<const float4*>(pa + c), qb = *reinterpret_cast<const float4*>(pb + c);
        const float4 h = *reinterpret_cast<const float4*>(head + c);
        t = t + (((gu(qa.x, qb.x, h.x) * qa.x + gu(qa.y, qb.y, h.y) * qa.y) + gu(qa.z, qb.z, h.z) * qa.z) + gu(qa.w, qb.w, h.w) * qa.w);
    }
    t = lp_group_sum(t);
    // (sa == 0: a is all zero, every a_k is masked below; the term would be 0 / 0)
    const float coef = ra > 0.0f ? t / (na * na) / ra : 0.0f;
    auto ga = [&](float x, float y, float h) { return x > 0.0f ? gu(x, y, h) / na - coef * x : 0.0f; };
    for (int c = 4 * l; c < C; c += 4 * LP_G) {
        const float4 qa = *reinterpret_cast<const float4*>(pa + c), qb = *reinterpret_cast<const float4*>(pb + c);
        const float4 h = *reinterpret_cast<const float4*>(head + c);
        float4 r = make_float4(ga(qa.x, qb.x, h.x), ga(qa.y, qb.y, h.y), ga(qa.z, qb.z, h.z), ga(qa.w, qb.w, h.w));
        if (accumulate) {
            const float4 o = *reinterpret_cast<const float4*>(pg + c);
            r.x = o.x + r.x;
            r.y = o.y + r.y;
            r.z = o.z + r.z;
            r.w = o.w + r.w;
        }
        *reinterpret_cast<float4*>(pg + c) = r;
    }
}

// partials of the 5 blocks in index order (f64) -> value = sum_b S_b / P_b; with loss: loss = loss + value * weight (f32)
struct LpFinal {
    uint32_t off[LP_BLOCKS + 1];
    double pixels[LP_BLOCKS];
};
__global__ __launch_bounds__(LP_WG) void lpips_final(const double* __restrict__ partial, LpFinal f, float* __restrict__ value, float weight,
                                                     float* __restrict__ loss, float* __restrict__ loss_host) {
    __shared__ double s_red[LP_WG / 64];
    double total = 0.0;
    for (int bl = 0; bl < LP_BLOCKS; ++bl) {
        double v = 0.0;
        for (uint32_t i = f.off[bl] + threadIdx.x; i < f.off[bl + 1]; i += LP_WG) v += partial[i];
        v = lp_wave_sum(v);
        if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
        __syncthreads();
        total += ((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])) / f.pixels[bl];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float val = (float)total;
        if (value) value[0] = val;
        if (loss) {
            const float l = loss[0] + val * weight;
            loss[0] = l;
            if (loss_host) loss_host[0] = l;
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static inline uint32_t lp_grid(size_t n) { return (uint32_t)((n + LP_WG - 1) / LP_WG); }
static inline uint32_t lp_head_grid(size_t pixels) { return (uint32_t)((pixels + LP_PIX - 1) / LP_PIX); }

struct LpDims {
    int h[LP_BLOCKS], w[LP_BLOCKS];
    size_t P[LP_BLOCKS];
    LpDims(uint32_t H, uint32_t W) {
        for (int b = 0; b < LP_BLOCKS; ++b) {
            h[b] = b == 0 ? (int)H : h[b - 1] / 2;
            w[b] = b == 0 ? (int)W : w[b - 1] / 2;
            P[b] = (size_t)h[b] * w[b];
        }
    }
};

static int launch_conv(bh_ctx* ctx, const bh_lpips* m, int L, bool dgrad, const float* in, const float* epi, float* out, int H, int W) {
    // forward: Cin -> Cout with the fwd packing; data gradient: Cout -> Cin with the dgrad packing
    const int ci = dgrad ? LP_COUT[L] : LP_CIN[L], co = dgrad ? LP_CIN[L] : LP_COUT[L];
    const float* B = dgrad ? m->dgrad[L] : m->fwd[L];
    const int M = H * W;
    if (co == 64) {
        const dim3 grid((M + 255) / 256, co / 64);
        if (dgrad) hipLaunchKernelGGL((lpips_conv3x3_dgrad<4, 1>), grid, dim3(LP_WG), 0, ctx->stream, in, B, epi, out, H, W, ci, co);
        else hipLaunchKernelGGL((lpips_conv3x3_fwd<4, 1>), grid, dim3(LP_WG), 0, ctx->stream, in, B, epi, out, H, W, ci, co);
    } else {
        const dim3 grid((M + 127) / 128, co / 128);
        if (dgrad) hipLaunchKernelGGL((lpips_conv3x3_dgrad<2, 2>), grid, dim3(LP_WG), 0, ctx->stream, in, B, epi, out, H, W, ci, co);
        else hipLaunchKernelGGL((lpips_conv3x3_fwd<2, 2>), grid, dim3(LP_WG), 0, ctx->stream, in, B, epi, out, H, W, ci, co);
    }
    BH_LAUNCH_CHECK(ctx, dgrad ? "lpips_conv3x3_dgrad" : "lpips_conv3x3_fwd");
    return 0;
}

static int launch_pool_fwd(bh_ctx* ctx, const float* in, float* out, int H, int W, int C) {
    const size_t n = (size_t)(H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(lpips_pool_fwd, dim3(lp_grid(n)), dim3(LP_WG), 0, ctx->stream, reinterpret_cast<const float4*>(in), reinterpret_cast<float4*>(out), H,
                       W, C / 4);
    BH_LAUNCH_CHECK(ctx, "lpips_pool_fwd");
    return 0;
}

// One image through the network.  keep_all: every conv output to acts[L] and every pooled input to pooled[b] (pred, for the
// backward); else through the scratch pair, the block outputs only to outs[b].
struct LpImage {
    float* x0 = nullptr;
    float* acts[LP_LAYERS] = {};
    float* pooled[LP_BLOCKS] = {};
    float* outs[LP_BLOCKS] = {};
};

static int run_image(bh_ctx* ctx, const bh_lpips* m, const LpDims& d, LpImage& im, bool keep_all, float* scratch0, float* scratch1) {
    const float* cur = im.x0;
    for (int L = 0; L < LP_LAYERS; ++L) {
        const int b = LP_BLOCK_OF[L];
        const int H = d.h[b], W = d.w[b];
        if (L == LP_FIRST[b] && b > 0) {
            float* pooled = keep_all ? im.pooled[b] : (cur == scratch0 ? scratch1 : scratch0);
            BH_TRY(launch_pool_fwd(ctx, cur, pooled, d.h[b - 1], d.w[b - 1], LP_CIN[L]));
            cur = pooled;
        }
        float* out;
        if (keep_all) out = im.acts[L];
        else if (L == LP_LAST[b]) out = im.outs[b];
        else out = cur == scratch0 ? scratch1 : scratch0;
        if (L == 0) {
            hipLaunchKernelGGL(lpips_conv3x3_fwd_c3, dim3(lp_grid(d.P[0])), dim3(LP_WG), 0, ctx->stream, cur, m->fwd[0], m->bias[0], out, H, W);
            BH_LAUNCH_CHECK(ctx, "lpips_conv3x3_fwd_c3");
        } else {
            BH_TRY(launch_conv(ctx, m, L, false, cur, m->bias[L], out, H, W));
        }
        if (keep_all && L == LP_LAST[b]) im.outs[b] = out;
        cur = out;
    }
    return 0;
}

// The whole LPIPS term.  v_output == NULL: value only.  loss != NULL (train step): loss += value * weight.
static int lpips_run(bh_ctx* ctx, const bh_lpips* m, const float* img_hwc4, const uint32_t* gt_packed, uint32_t h, uint32_t w, const float* bg,
                     float weight, float* value, float* v_output, float* loss, float* loss_host) {
    const LpDims d(h, w);
    const bool grad = v_output != nullptr;
    const size_t P1 = d.P[0];
    // arena layout (floats), every piece a multiple of 4 floats
    auto r4 = [](size_t x) { return (x + 3) & ~(size_t)3; };
    size_t total = 2 * r4(P1 * 3) + 2 * P1 * 64;   // x0 pred, x0 gt, the scratch / gradient pair
    for (int b = 0; b < LP_BLOCKS; ++b) total += d.P[b] * LP_CH[b] * (grad ? 1 : 2);   // block outputs of gt (and pred, value only)
    if (grad) {
        for (int L = 0; L < LP_LAYERS; ++L) total += d.P[LP_BLOCK_OF[L]] * LP_COUT[L];   // pred's 13 conv outputs
        for (int b = 1; b < LP_BLOCKS; ++b) total += d.P[b] * LP_CH[b - 1];             // pred's pooled inputs
    }
    uint32_t part_off[LP_BLOCKS + 1];
    part_off[0] = 0;
    for (int b = 0; b < LP_BLOCKS; ++b) part_off[b + 1] = part_off[b] + lp_head_grid(d.P[b]);
    const size_t part_bytes = ((size_t)part_off[LP_BLOCKS] * 8 + 15) & ~(size_t)15;
    auto* base = (char*)ensure(ctx, SLOT_LPIPS, total * 4 + part_bytes + 16);
    if (!base) return BH_ERR_OOM;
    double* partial = reinterpret_cast<double*>(base);
    float* f = reinterpret_cast<float*>(base + part_bytes);
    auto take = [&](size_t n) { float* p = f; f += r4(n); return p; };
    LpImage pr, gi;
    pr.x0 = take(P1 * 3);
    gi.x0 = take(P1 * 3);
    float* s0 = take(P1 * 64);
    float* s1 = take(P1 * 64);
    for (int b = 0; b < LP_BLOCKS; ++b) {
        gi.outs[b] = take(d.P[b] * LP_CH[b]);
        if (!grad) pr.outs[b] = take(d.P[b] * LP_CH[b]);
    }
    if (grad) {
        for (int L = 0; L < LP_LAYERS; ++L) pr.acts[L] = take(d.P[LP_BLOCK_OF[L]] * LP_COUT[L]);
        for (int b = 1; b < LP_BLOCKS; ++b) pr.pooled[b] = take(d.P[b] * LP_CH[b - 1]);
    }

    ProfScope ps(ctx, grad ? "LpipsValueAndGrad" : "LpipsForward");
    hipLaunchKernelGGL(lpips_input_pred, dim3(lp_grid(P1)), dim3(LP_WG), 0, ctx->stream, reinterpret_cast<const float4*>(img_hwc4), pr.x0, (uint32_t)P1);
    BH_LAUNCH_CHECK(ctx, "lpips_input_pred");
    const int composite = bg ? 1 : 0;
    hipLaunchKernelGGL(lpips_input_gt, dim3(lp_grid(P1)), dim3(LP_WG), 0, ctx->stream, gt_packed, gi.x0, (uint32_t)P1, composite, bg ? bg[0] : 0.0f,
                       bg ? bg[1] : 0.0f, bg ? bg[2] : 0.0f);
    BH_LAUNCH_CHECK(ctx, "lpips_input_gt");
    BH_TRY(run_image(ctx, m, d, gi, false, s0, s1));
    BH_TRY(run_image(ctx, m, d, pr, grad, s0, s1));
    for (int b = 0; b < LP_BLOCKS; ++b) {
        hipLaunchKernelGGL(lpips_head_fwd, dim3(lp_head_grid(d.P[b])), dim3(LP_WG), 0, ctx->stream, pr.outs[b], gi.outs[b], m->head[b], (uint32_t)d.P[b],
                           LP_CH[b], partial + part_off[b]);
        BH_LAUNCH_CHECK(ctx, "lpips_head_fwd");
    }
    LpFinal fin;
    for (int b = 0; b <= LP_BLOCKS; ++b) fin.off[b] = part_off[b];
    for (int b = 0; b < LP_BLOCKS; ++b) fin.pixels[b] = (double)d.P[b];
    hipLaunchKernelGGL(lpips_final, dim3(1), dim3(LP_WG), 0, ctx->stream, partial, fin, value, weight, loss, loss_host);
    BH_LAUNCH_CHECK(ctx, "lpips_final");
    if (!grad) return 0;

    // backward of pred: cur holds dL/dz of layer L (its ReLU mask applied), the other buffer receives the next one
    auto head_bwd = [&](int b, bool acc, float* g) -> int {
        const float scale = (float)((double)weight / (double)d.P[b]);
        hipLaunchKernelGGL(lpips_head_bwd, dim3(lp_head_grid(d.P[b])), dim3(LP_WG), 0, ctx->stream, pr.outs[b], gi.outs[b], m->head[b], (uint32_t)d.P[b], LP_CH[b],
                           scale, acc ? 1 : 0, g);
        BH_LAUNCH_CHECK(ctx, "lpips_head_bwd");
        return 0;
    };
    float* cur = s0;
    float* other = s1;
    BH_TRY(head_bwd(LP_BLOCKS - 1, false, cur));
    for (int L = LP_LAYERS - 1; L >= 1; --L) {
        const int b = LP_BLOCK_OF[L];
        const bool first = L == LP_FIRST[b];
        const float* input_act = first ? pr.pooled[b] : pr.acts[L - 1];
        BH_TRY(launch_conv(ctx, m, L, true, cur, input_act, other, d.h[b], d.w[b]));
        std::swap(cur, other);
        if (first) {
            // dL/d(pooled) -> dL/d(block b-1 output) through the pool, then that block's own head term
            const size_t n = d.P[b - 1] * LP_CH[b - 1];
            hipLaunchKernelGGL(lpips_pool_bwd, dim3(lp_grid(n)), dim3(LP_WG), 0, ctx->stream, pr.acts[L - 1], cur, other, d.h[b - 1], d.w[b - 1], LP_CH[b - 1]);
            BH_LAUNCH_CHECK(ctx, "lpips_pool_bwd");
            std::swap(cur, other);
            BH_TRY(head_bwd(b - 1, true, cur));
        }
    }
    hipLaunchKernelGGL(lpips_conv3x3_dgrad_c3, dim3(lp_grid(P1)), dim3(LP_WG), 0, ctx->stream, cur, m->dgrad[0], v_output, d.h[0], d.w[0]);
    BH_LAUNCH_CHECK(ctx, "lpips_conv3x3_dgrad_c3");
    return 0;
}

static int lpips_check(bh_ctx* ctx, const bh_lpips* m, const float* img, const uint32_t* gt, uint32_t h, uint32_t w, const char* who) {
    if (!m || !img || !gt) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": null argument");
    if (h < 16 || w < 16) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": h and w must be >= 16 (block 5 needs a pixel)");
    if ((uint64_t)h * w > (1ull << 26)) return set_error(ctx, BH_ERR_UNSUPPORTED, std::string(who) + ": more than 2^26 pixels");
    if (reinterpret_cast<uintptr_t>(img) & 15u) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": img_hwc4 must be 16-byte aligned");
    if (m->device != ctx->device) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": the model lives on another device");
    return 0;
}

// the train step's term (train.hip): loss += weight * LPIPS, v_output.rgb += weight * dLPIPS/dimg
int lpips_train_term(bh_ctx* ctx, const float* img_hwc4, const uint32_t* gt_packed, uint32_t h, uint32_t w, const float* bg, float* v_output,
                     float* loss, float* loss_host) {
    const bh_lpips* m = ctx->terms.lpips;
    BH_TRY(lpips_check(ctx, m, img_hwc4, gt_packed, h, w, "train_step (LPIPS)"));
    return lpips_run(ctx, m, img_hwc4, gt_packed, h, w, bg, ctx->terms.lpips_weight, nullptr, v_output, loss, loss_host);
}

}  // namespace bh

using namespace bh;

extern "C" {

bh_lpips* bh_lpips_create(bh_ctx* ctx, const float* params, uint64_t count) {
    if (!ctx) return nullptr;
    if (!params) {
        set_error(ctx, BH_ERR_INVALID_ARG, "lpips_create: null params");
        return nullptr;
    }
    if (count != BH_LPIPS_PARAM_COUNT) {
        set_error(ctx, BH_ERR_INVALID_ARG, "lpips_create: expected " + std::to_string(BH_LPIPS_PARAM_COUNT) + " floats, got " + std::to_string(count));
        return nullptr;
    }
    // host repack: canonical order is per conv W [Cout][Cin][3][3] then bias [Cout], then the 5 heads [C]
    size_t dev_floats = 0;
    for (int L = 0; L < LP_LAYERS; ++L) dev_floats += 2 * (size_t)LP_COUT[L] * LP_CIN[L] * 9 + LP_COUT[L];
    for (int b = 0; b < LP_BLOCKS; ++b) dev_floats += LP_CH[b];
    std::vector<float> host(dev_floats);
    const float* src = params;
    size_t o = 0;
    size_t offs[LP_LAYERS][3], head_off[LP_BLOCKS];
    for (int L = 0; L < LP_LAYERS; ++L) {
        const int ci = LP_CIN[L], co = LP_COUT[L];
        const size_t nw = (size_t)co * ci * 9;
        float* fw = host.data() + o;
        float* dw = fw + nw;
        float* bs = dw + nw;
        offs[L][0] = o;
        offs[L][1] = o + nw;
        offs[L][2] = o + 2 * nw;
        for (int c = 0; c < co; ++c)
            for (int i = 0; i < ci; ++i)
                for (int t = 0; t < 9; ++t) {
                    const float v = src[((size_t)c * ci + i) * 9 + t];
                    fw[((size_t)t * ci + i) * co + c] = v;
                    dw[((size_t)(8 - t) * co + c) * ci + i] = v;   // tap' = 8 - tap: (2 - ky, 2 - kx)
                }
        src += nw;
        for (int c = 0; c < co; ++c) bs[c] = src[c];
        src += co;
        o += 2 * nw + co;
    }
    for (int b = 0; b < LP_BLOCKS; ++b) {
        head_off[b] = o;
        for (int c = 0; c < LP_CH[b]; ++c) host[o + c] = src[c];
        src += LP_CH[b];
        o += LP_CH[b];
    }
    if (hipSetDevice(ctx->device) != hipSuccess) {
        set_error(ctx, BH_ERR_HIP, "lpips_create: hipSetDevice failed");
        return nullptr;
    }
    auto* m = new bh_lpips();
    m->device = ctx->device;
    if (hipMalloc(&m->mem, dev_floats * 4) != hipSuccess) {
        delete m;
        set_error(ctx, BH_ERR_OOM, "lpips_create: out of device memory");
        return nullptr;
    }
    if (hipMemcpy(m->mem, host.data(), dev_floats * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(m->mem);
        delete m;
        set_error(ctx, BH_ERR_HIP, "lpips_create: upload failed");
        return nullptr;
    }
    for (int L = 0; L < LP_LAYERS; ++L) {
        m->fwd[L] = m->mem + offs[L][0];
        m->dgrad[L] = m->mem + offs[L][1];
        m->bias[L] = m->mem + offs[L][2];
    }
    for (int b = 0; b < LP_BLOCKS; ++b) m->head[b] = m->mem + head_off[b];
    return m;
}

void bh_lpips_destroy(bh_lpips* m) {
    if (!m) return;
    if (m->mem) {
        (void)hipSetDevice(m->device);
        (void)hipFree(m->mem);
    }
    delete m;
}

int bh_lpips_forward(bh_ctx* ctx, const bh_lpips* m, const float* img_hwc4, const uint32_t* gt_packed, uint32_t h, uint32_t w,
                     const float* composite_bg, float* value) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!value) return set_error(ctx, BH_ERR_INVALID_ARG, "lpips_forward: null value");
    BH_TRY(lpips_check(ctx, m, img_hwc4, gt_packed, h, w, "lpips_forward"));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return lpips_run(ctx, m, img_hwc4, gt_packed, h, w, composite_bg, 1.0f, value, nullptr, nullptr, nullptr);
}

int bh_lpips_value_and_grad(bh_ctx* ctx, const bh_lpips* m, const float* img_hwc4, const uint32_t* gt_packed, uint32_t h, uint32_t w,
                            const float* composite_bg, float weight, float* value, float* v_output) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!value || !v_output) return set_error(ctx, BH_ERR_INVALID_ARG, "lpips_value_and_grad: null value / v_output");
    BH_TRY(lpips_check(ctx, m, img_hwc4, gt_packed, h, w, "lpips_value_and_grad"));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return lpips_run(ctx, m, img_hwc4, gt_packed, h, w, composite_bg, weight, value, v_output, nullptr, nullptr);
}

int bh_train_set_lpips(bh_ctx* ctx, const bh_lpips* m, float weight) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!(weight >= 0.0f) || !std::isfinite(weight)) return set_error(ctx, BH_ERR_INVALID_ARG, "train_set_lpips: weight must be finite and >= 0");
    if (m && m->device != ctx->device) return set_error(ctx, BH_ERR_INVALID_ARG, "train_set_lpips: the model lives on another device");
    ctx->terms.lpips = m;
    ctx->terms.lpips_weight = m ? weight : 0.0f;
    return 0;
}

}  // extern "C"
