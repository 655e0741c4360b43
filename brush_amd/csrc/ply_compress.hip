// ply_compress.hip — splats -> SuperSplat / PlayCanvas "compressed.ply" (include/brush_hip_compressed_ply.h).
//
// The inverse of ply.hip's ply_decode_compressed_kernel (the reference's import.rs:407-600, quant.rs): rows in Morton order of a
// 1024^3 cell grid over the finite position box, each chunk of 256 file rows quantised against its own position / log-scale /
// colour ranges, the rotation as its smallest three, opacity as an absolute byte, SH bands as bytes.
//
// MI355X shape: the whole body is assembled on the device and crosses PCIe once, about 4x smaller than bh_splat_to_ply's.
//   cply_box_kernel       grid-stride min / max of the finite x y z, one partial per block (no atomics)
//   cply_box_final_kernel one block folds the partials into the box (min / max are exact: the result does not depend on order)
//   cply_keys_kernel      30-bit Morton key per splat
//   radix_argsort         stable, 30 bits (sort.hip): file row -> input row
//   cply_chunk_kernel<D>  one 256-thread block per chunk: gathers its rows through the order, reduces the 9 ranges with wave
//                         shuffles and LDS, writes the chunk row, 256 x 16 B of vertex words and the chunk's SH bytes, which are
//                         one contiguous span of the sh block, staged in LDS and stored as aligned 32-bit words
#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/brush_hip_compressed_ply.h"
#include "context.h"

namespace bh {

constexpr int CPLY_WG = 256;              // threads per block = rows per chunk (the format's 256)
constexpr uint32_t CPLY_BOX_BLOCKS = 1024;
constexpr float CPLY_SH_C0 = 0.2820948f;  // the reference's SH_C0 (sh.rs), the constant rgb_to_sh divides by

static const char* const kCplyChunkNames[18] = {"min_x", "min_y", "min_z", "max_x", "max_y", "max_z", "min_scale_x", "min_scale_y", "min_scale_z",
                                                "max_scale_x", "max_scale_y", "max_scale_z", "min_r", "min_g", "min_b", "max_r", "max_g", "max_b"};
static const char* const kCplyVertexNames[4] = {"packed_position", "packed_rotation", "packed_scale", "packed_color"};

// unorm(v, b): min(t, floor(v t + 0.5)), t = 2^b - 1; 0 for v < 0 or NaN
BH_DEV uint32_t cply_unorm(float v, uint32_t bits) {
    const float t = (float)((1u << bits) - 1u);
    if (!(v >= 0.0f)) return 0u;
    const float f = __builtin_floorf(v * t + 0.5f);
    return f >= t ? (1u << bits) - 1u : (uint32_t)f;
}
// norm01(x, lo, hi): 0 for a degenerate range, else (x - lo) / (hi - lo)
BH_DEV float cply_norm01(float x, float lo, float hi) {
    const float r = hi - lo;
    return r < 1e-5f ? 0.0f : (x - lo) / r;
}
BH_DEV uint32_t cply_part1by2(uint32_t x) {   // spread the low 10 bits of x to every third bit
    x &= 0x3FFu;
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}
BH_DEV uint32_t cply_cell(float x, float lo, float hi) {
    const float f = __builtin_floorf(1024.0f * cply_norm01(x, lo, hi));
    if (!(f >= 0.0f)) return 0u;   // NaN, -inf, below the box
    return f > 1023.0f ? 1023u : (uint32_t)f;
}
BH_DEV float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = __builtin_fminf(v, __shfl_xor(v, o, 64));
    return v;
}
BH_DEV float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = __builtin_fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// partial[b] = (min x y z, max x y z) over the finite coordinates of the rows block b visits (+inf / -inf: none)
__global__ __launch_bounds__(CPLY_WG) void cply_box_kernel(const float* __restrict__ transforms, uint32_t n, float* __restrict__ partial) {
    float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (uint32_t i = blockIdx.x * CPLY_WG + threadIdx.x; i < n; i += gridDim.x * CPLY_WG) {
        const float* t = transforms + (size_t)i * 10;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = t[k];
            if (is_finite_f32(v)) {
                mn[k] = __builtin_fminf(mn[k], v + 0.0f);
                mx[k] = __builtin_fmaxf(mx[k], v + 0.0f);
            }
        }
    }
    __shared__ float red[CPLY_WG / 64][6];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        mn[k] = wave_min(mn[k]);
        mx[k] = wave_max(mx[k]);
    }
    if (lane == 0)
        for (int k = 0; k < 3; ++k) { red[w][k] = mn[k]; red[w][3 + k] = mx[k]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = red[0][threadIdx.x];
        for (int j = 1; j < CPLY_WG / 64; ++j) v = threadIdx.x < 3 ? __builtin_fminf(v, red[j][threadIdx.x]) : __builtin_fmaxf(v, red[j][threadIdx.x]);
        partial[(size_t)blockIdx.x * 6 + threadIdx.x] = v;
    }
}

// box[0..5] = (lo x y z, hi x y z) from `blocks` partials; an axis with no finite value gets (0, 0)
__global__ __launch_bounds__(64) void cply_box_final_kernel(const float* __restrict__ partial, uint32_t blocks, float* __restrict__ box) {
    const uint32_t lane = threadIdx.x;
    float v[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = k < 3 ? __builtin_inff() : -__builtin_inff();
    for (uint32_t b = lane; b < blocks; b += 64)
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = k < 3 ? __builtin_fminf(v[k], partial[(size_t)b * 6 + k]) : __builtin_fmaxf(v[k], partial[(size_t)b * 6 + k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v[k] = wave_min(v[k]);
        v[3 + k] = wave_max(v[3 + k]);
    }
    if (lane < 3) {
        const bool empty = v[lane] == __builtin_inff();
        box[lane] = empty ? 0.0f : v[lane];
        box[3 + lane] = empty ? 0.0f : v[3 + lane];
    }
}

// key = part1by2(q_z) << 2 | part1by2(q_y) << 1 | part1by2(q_x)
__global__ __launch_bounds__(CPLY_WG) void cply_keys_kernel(const float* __restrict__ transforms, uint32_t n, const float* __restrict__ box,
                                                            uint32_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * CPLY_WG + threadIdx.x;
    if (i >= n) return;
    const float* t = transforms + (size_t)i * 10;
    const uint32_t qx = cply_cell(t[0], box[0], box[3]), qy = cply_cell(t[1], box[1], box[4]), qz = cply_cell(t[2], box[2], box[5]);
    keys[i] = (cply_part1by2(qz) << 2) | (cply_part1by2(qy) << 1) | cply_part1by2(qx);
}

// smallest-three rotation word of the (w, x, y, z) row q: the inverse of quant.rs::decode_quat
BH_DEV uint32_t cply_rotation(const float q[4]) {
    const float s = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    float a[4] = {1.0f, 0.0f, 0.0f, 0.0f};
    if (s != 0.0f && is_finite_f32(s)) {
        const float r = __builtin_sqrtf(s);
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = q[k] / r;
    }
    uint32_t L = 0;
    float best = __builtin_fabsf(a[0]);
#pragma unroll
    for (uint32_t k = 1; k < 4; ++k)
        if (__builtin_fabsf(a[k]) > best) { best = __builtin_fabsf(a[k]); L = k; }
    const float sgn = a[L] < 0.0f ? -1.0f : 1.0f;
    uint32_t word = L;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        if (k != L) word = (word << 10) | cply_unorm((sgn * a[k]) * 0.70710677f + 0.5f, 10);
    return word;
}

BH_DEV uint32_t cply_sh_byte(float v) {   // clamp(trunc((v / 8 + 0.5) * 256), 0, 255), NaN -> 0
    const float f = (v * 0.125f + 0.5f) * 256.0f;
    if (!(f > 0.0f)) return 0u;
    return f >= 255.0f ? 255u : (uint32_t)f;
}

// One block per chunk c: file rows [256c, min(256c + 256, n)), row r holds input splat order[r].
// body: chunk rows [C][18] f32 | vertex words [n][4] u32 | sh bytes [n][3K] u8, exactly as in the file
template <int D>
__global__ __launch_bounds__(CPLY_WG) void cply_chunk_kernel(const float* __restrict__ transforms, const float* __restrict__ sh,
                                                             const float* __restrict__ raw_opac, const uint32_t* __restrict__ order, uint32_t n,
                                                             uint32_t nchunks, uint8_t* __restrict__ body) {
    constexpr uint32_t C = (D + 1) * (D + 1), K = C - 1, SHB = 3 * K;
    constexpr uint32_t SH_WORDS = (CPLY_WG * SHB + 3) / 4;
    __shared__ float red[CPLY_WG / 64][18];
    __shared__ uint32_t sh_stage[SH_WORDS ? SH_WORDS : 1];
    const uint32_t c = blockIdx.x, t = threadIdx.x;
    const uint32_t w = t >> 6, lane = t & 63;
    const uint64_t r = (uint64_t)c * CPLY_WG + t;
    const bool live = r < n;
    const uint32_t src = live ? order[r] : 0u;
    float p[3] = {0, 0, 0}, q[4] = {1, 0, 0, 0}, s[3] = {0, 0, 0}, rgb[3] = {0, 0, 0}, o = 0.0f;
    if (live) {
        const float2* t2 = reinterpret_cast<const float2*>(transforms + (size_t)src * 10);   // 40-byte rows: 8-byte aligned
        const float2 a = t2[0], b = t2[1], cc = t2[2], d = t2[3], e = t2[4];
        p[0] = a.x; p[1] = a.y; p[2] = b.x;
        q[0] = b.y; q[1] = cc.x; q[2] = cc.y; q[3] = d.x;
        s[0] = d.y; s[1] = e.x; s[2] = e.y;
        o = raw_opac[src];
        const float* dc = sh + (size_t)src * C * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb[k] = dc[k] * CPLY_SH_C0 + 0.5f;
    }
    // the 9 ranges over the finite values of the chunk's rows (v + 0: -0 and +0 are one extreme)
    const float* vals[3] = {p, s, rgb};
    float lo[9], hi[9];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = vals[g][k];
            const bool ok = live && is_finite_f32(v);
            lo[g * 3 + k] = wave_min(ok ? v + 0.0f : __builtin_inff());
            hi[g * 3 + k] = wave_max(ok ? v + 0.0f : -__builtin_inff());
        }
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 9; ++k) { red[w][k] = lo[k]; red[w][9 + k] = hi[k]; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        float a = red[0][k], b = red[0][9 + k];
#pragma unroll
        for (int j = 1; j < CPLY_WG / 64; ++j) { a = __builtin_fminf(a, red[j][k]); b = __builtin_fmaxf(b, red[j][9 + k]); }
        const bool empty = a == __builtin_inff();   // no finite value: (0, 0)
        lo[k] = empty ? 0.0f : a;
        hi[k] = empty ? 0.0f : b;
    }
    // chunk row: min_x min_y min_z max_x max_y max_z | min_scale_* max_scale_* | min_r g b max_r g b
    if (t < 18) {
        const uint32_t g = t / 6, j = t % 6;
        reinterpret_cast<float*>(body)[(size_t)c * 18 + t] = j < 3 ? lo[g * 3 + j] : hi[g * 3 + (j - 3)];
    }
    if (live) {
        const uint32_t ppos = (cply_unorm(cply_norm01(p[0], lo[0], hi[0]), 11) << 21) | (cply_unorm(cply_norm01(p[1], lo[1], hi[1]), 10) << 11) |
                              cply_unorm(cply_norm01(p[2], lo[2], hi[2]), 11);
        const uint32_t pscl = (cply_unorm(cply_norm01(s[0], lo[3], hi[3]), 11) << 21) | (cply_unorm(cply_norm01(s[1], lo[4], hi[4]), 10) << 11) |
                              cply_unorm(cply_norm01(s[2], lo[5], hi[5]), 11);
        const uint32_t pcol = (cply_unorm(cply_norm01(rgb[0], lo[6], hi[6]), 8) << 24) | (cply_unorm(cply_norm01(rgb[1], lo[7], hi[7]), 8) << 16) |
                              (cply_unorm(cply_norm01(rgb[2], lo[8], hi[8]), 8) << 8) | cply_unorm(sigmoid(o), 8);
        const uint32_t prot = cply_rotation(q);
        // 16 B per row at 72 C + 16 r: 8-byte aligned (72 C is a multiple of 8, not always of 16)
        uint2* vw = reinterpret_cast<uint2*>(body + (size_t)nchunks * 72 + r * 16);
        vw[0] = make_uint2(ppos, prot);
        vw[1] = make_uint2(pscl, pcol);
    }
    if constexpr (SHB > 0) {
        // f_rest_{ch K + (k - 1)} = channel ch of coefficient k: the row's 3K bytes at t * 3K of the chunk's span
        uint8_t* stage = reinterpret_cast<uint8_t*>(sh_stage);
        if (live) {
            const float* row = sh + (size_t)src * C * 3;
#pragma unroll
            for (uint32_t ch = 0; ch < 3; ++ch)
#pragma unroll
                for (uint32_t k = 1; k <= K; ++k) stage[t * SHB + ch * K + (k - 1)] = (uint8_t)cply_sh_byte(row[k * 3 + ch]);
        }
        __syncthreads();
        // the chunk's span starts at 72 C + 16 n + 256 c 3K: a multiple of 8.  Whole words: a last chunk's final word may run up to
        // 3 bytes past the body, into the scratch's padding (never copied out)
        const uint32_t rows = (uint32_t)((uint64_t)n - (uint64_t)c * CPLY_WG < CPLY_WG ? (uint64_t)n - (uint64_t)c * CPLY_WG : CPLY_WG);
        const uint32_t words = (rows * SHB + 3) / 4;
        uint32_t* dst = reinterpret_cast<uint32_t*>(body + (size_t)nchunks * 72 + (size_t)n * 16 + (size_t)c * CPLY_WG * SHB);
        for (uint32_t i = t; i < words; i += CPLY_WG) dst[i] = sh_stage[i];
    }
}

static std::string compressed_ply_header(uint64_t n, uint32_t sh_degree, bool render_mip, const float* up_axis) {
    std::string h = "ply\nformat binary_little_endian 1.0\n";
    h += ply_header_comments(sh_degree, render_mip, up_axis);
    h += "element chunk " + std::to_string((n + CPLY_WG - 1) / CPLY_WG) + "\n";
    for (const char* p : kCplyChunkNames) h += std::string("property float ") + p + "\n";
    h += "element vertex " + std::to_string(n) + "\n";
    for (const char* p : kCplyVertexNames) h += std::string("property uint ") + p + "\n";
    const uint32_t rest = 3u * ((sh_degree + 1u) * (sh_degree + 1u) - 1u);
    if (rest) {
        h += "element sh " + std::to_string(n) + "\n";
        for (uint32_t k = 0; k < rest; ++k) h += "property uchar f_rest_" + std::to_string(k) + "\n";
    }
    h += "end_header\n";
    return h;
}

template <int D>
static void launch_chunks(bh_ctx* ctx, const float* t, const float* sh, const float* o, const uint32_t* order, uint32_t n, uint32_t nchunks,
                          uint8_t* body) {
    hipLaunchKernelGGL(cply_chunk_kernel<D>, dim3(nchunks), dim3(CPLY_WG), 0, ctx->stream, t, sh, o, order, n, nchunks, body);
}

}  // namespace bh

using namespace bh;

extern "C" {

int bh_splat_to_compressed_ply(bh_ctx* ctx, const float* transforms, const float* sh_coeffs, const float* raw_opacities, const float* min_scale,
                               uint32_t n, uint32_t sh_degree, int render_mip, const float* up_axis, uint32_t* order, void* out, uint64_t cap,
                               uint64_t* written) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!written) return set_error(ctx, BH_ERR_INVALID_ARG, "splat_to_compressed_ply: null size pointer");
    if (sh_degree > 4) return set_error(ctx, BH_ERR_INVALID_ARG, "sh_degree must be 0..4");
    const uint32_t coeffs = (sh_degree + 1) * (sh_degree + 1);
    const uint64_t shb = 3ull * (coeffs - 1u);
    const uint32_t nchunks = (uint32_t)(((uint64_t)n + CPLY_WG - 1) / CPLY_WG);
    const std::string header = compressed_ply_header(n, sh_degree, render_mip != 0, up_axis);
    const uint64_t body = 72ull * nchunks + 16ull * n + shb * n;
    *written = header.size() + body;
    if (!out) return 0;  // size query
    if (cap < *written) return set_error(ctx, BH_ERR_INVALID_ARG, "splat_to_compressed_ply: output buffer too small");
    if (n > 0 && (!transforms || !sh_coeffs || !raw_opacities)) return set_error(ctx, BH_ERR_INVALID_ARG, "splat_to_compressed_ply: null splat tensor");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    std::memcpy(out, header.data(), header.size());
    if (n == 0) return 0;
    // export.rs:183: bake the 3D-filter floor first, as bh_splat_to_ply does
    const float* t = transforms;
    const float* o = raw_opacities;
    if (min_scale) {
        auto* ft = (float*)ensure(ctx, SLOT_FOLDED_TRANSFORMS, (size_t)n * 10 * 4);
        auto* fo = (float*)ensure(ctx, SLOT_FOLDED_RAW_OPAC, (size_t)n * 4);
        if (!ft || !fo) return BH_ERR_OOM;
        BH_TRY(launch_fold_min_scale(ctx, transforms, raw_opacities, min_scale, n, ft, fo));
        t = ft;
        o = fo;
    }
    // scratch: box partials [CPLY_BOX_BLOCKS][6] | box [8] | keys [n] | sorted keys [n] | order [n] (when the caller gives none)
    const uint32_t box_blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n + CPLY_WG - 1) / CPLY_WG, CPLY_BOX_BLOCKS);
    const size_t head_words = (size_t)CPLY_BOX_BLOCKS * 6 + 8;
    auto* scratch = (uint32_t*)ensure(ctx, SLOT_PLY_COMPRESS, (head_words + (size_t)n * 3) * 4);
    if (!scratch) return BH_ERR_OOM;
    float* partial = reinterpret_cast<float*>(scratch);
    float* box = partial + (size_t)CPLY_BOX_BLOCKS * 6;
    uint32_t* keys = scratch + head_words;
    uint32_t* keys_sorted = keys + n;
    uint32_t* rows = order ? order : keys_sorted + n;
    auto* dev_body = (uint8_t*)ensure(ctx, SLOT_PLY_ROWS, (size_t)((body + 15) & ~15ull));
    if (!dev_body) return BH_ERR_OOM;
    hipLaunchKernelGGL(cply_box_kernel, dim3(box_blocks), dim3(CPLY_WG), 0, ctx->stream, t, n, partial);
    BH_LAUNCH_CHECK(ctx, "cply_box_kernel");
    hipLaunchKernelGGL(cply_box_final_kernel, dim3(1), dim3(64), 0, ctx->stream, partial, box_blocks, box);
    BH_LAUNCH_CHECK(ctx, "cply_box_final_kernel");
    hipLaunchKernelGGL(cply_keys_kernel, dim3(nchunks), dim3(CPLY_WG), 0, ctx->stream, t, n, box, keys);
    BH_LAUNCH_CHECK(ctx, "cply_keys_kernel");
    BH_TRY(radix_argsort(ctx, keys, nullptr, n, 30, keys_sorted, rows));   // stable: equal cells keep input order
    switch (sh_degree) {
        case 0: launch_chunks<0>(ctx, t, sh_coeffs, o, rows, n, nchunks, dev_body); break;
        case 1: launch_chunks<1>(ctx, t, sh_coeffs, o, rows, n, nchunks, dev_body); break;
        case 2: launch_chunks<2>(ctx, t, sh_coeffs, o, rows, n, nchunks, dev_body); break;
        case 3: launch_chunks<3>(ctx, t, sh_coeffs, o, rows, n, nchunks, dev_body); break;
        default: launch_chunks<4>(ctx, t, sh_coeffs, o, rows, n, nchunks, dev_body); break;
    }
    BH_LAUNCH_CHECK(ctx, "cply_chunk_kernel");
    BH_HIP(ctx, hipMemcpyAsync((char*)out + header.size(), dev_body, body, hipMemcpyDeviceToHost, ctx->stream));
    BH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"
