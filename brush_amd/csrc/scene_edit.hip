// scene_edit.hip — the entry points of brush_hip_scene.h: a similarity transform of a splat scene (with the rotation of its spherical
// harmonics), the same transform of a camera, and a region select.  The record arithmetic is host f64 in scene_math.h.  Not in the
// reference; DESIGN.md §6t.
//
// MI355X shape of bh_splats_transform.  About 5 flop per byte: a copy with arithmetic, and the rows are 40 B (transforms) and 12 ..
// 300 B (SH), so a thread that walks its own row from global memory touches 64 different cache lines per wave and load.  A block
// instead moves its tile of rows as ONE flat range — lane i takes bytes [16 i, 16 i + 16) — through LDS, and only there does a thread
// own a row.  In LDS a row starts every `stride` dwords and the 32 row-owners of a half wave (the group within which ds_read_b32
// conflicts) read the same column of 32 rows at once, bank (row * stride + column) mod 32: stride 10 (transforms) is a 2-way conflict,
// 12 (SH 1) 4-way, 48 (SH 3) 16-way; an odd stride has none, so even strides are padded by one dword (11, 13, 49; 27 and 75 are odd
// already).  A block reads its whole tile before it writes any of it and tiles are disjoint: that is what makes in place safe.  The
// 164 matrix entries are uniform: kernel arguments, read through the scalar cache; one kernel per degree, so the band loops unroll
// over literal argument offsets.
#include <cmath>

#include "../../include/brush_hip_scene.h"
#include "context.h"
#include "scene_math.h"

namespace bh {

constexpr int XF_ROWS = 256;          // transform rows per block (= threads)
constexpr int XF_STRIDE = 11;         // 10 padded to odd
constexpr int SEL_WG = 256;
constexpr uint32_t SEL_MAX_BLOCKS = 4096;   // grid-stride beyond this: the partial counts stay one page

struct XfArgs {
    float rot[9], quat[4], trans[3], scale, log_scale;
};

template <int DEG>
struct ShRot {
    float m[DEG == 1 ? 9 : DEG == 2 ? 34 : DEG == 3 ? 83 : 164];
};

// rows per block of the SH kernel: 13 / 27 / 49 / 75 dwords per padded row -> 13 / 27 / 25 / 38 KB of LDS
template <int DEG>
constexpr int sh_rows() { return DEG <= 2 ? 256 : 128; }

// flat element e of a tile of RS-dword rows -> its dword in LDS, rows RSP apart
template <int RS, int RSP>
BH_DEV uint32_t padded(uint32_t e) { return RS == RSP ? e : (e / RS) * RSP + e % RS; }

// The tile's `count` dwords at src into LDS.  VEC: src is 16-byte aligned — 16 bytes per lane, the last count % 4 dwords one by one.
template <int RS, int RSP, bool VEC>
BH_DEV void tile_load(const float* src, uint32_t count, float* lds) {
    uint32_t done = 0;
    if (VEC) {
        const uint32_t nvec = count >> 2;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        for (uint32_t v = threadIdx.x; v < nvec; v += blockDim.x) {
            const float4 x = s4[v];
            lds[padded<RS, RSP>(4 * v)] = x.x;
            lds[padded<RS, RSP>(4 * v + 1)] = x.y;
            lds[padded<RS, RSP>(4 * v + 2)] = x.z;
            lds[padded<RS, RSP>(4 * v + 3)] = x.w;
        }
        done = nvec << 2;
    }
    for (uint32_t e = done + threadIdx.x; e < count; e += blockDim.x) lds[padded<RS, RSP>(e)] = src[e];
}

template <int RS, int RSP, bool VEC>
BH_DEV void tile_store(float* dst, uint32_t count, const float* lds) {
    uint32_t done = 0;
    if (VEC) {
        const uint32_t nvec = count >> 2;
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (uint32_t v = threadIdx.x; v < nvec; v += blockDim.x)
            d4[v] = make_float4(lds[padded<RS, RSP>(4 * v)], lds[padded<RS, RSP>(4 * v + 1)], lds[padded<RS, RSP>(4 * v + 2)], lds[padded<RS, RSP>(4 * v + 3)]);
        done = nvec << 2;
    }
    for (uint32_t e = done + threadIdx.x; e < count; e += blockDim.x) dst[e] = lds[padded<RS, RSP>(e)];
}

// in / out (and min_scale / out_min_scale) may be the same memory: no __restrict__ on them.
template <bool VEC>
__global__ __launch_bounds__(XF_ROWS) void scene_transform_rows_kernel(XfArgs a, uint32_t n, const float* in, const float* min_scale, float* out,
                                                                       float* out_min_scale) {
    __shared__ float tile[XF_ROWS * XF_STRIDE];
    const uint64_t row0 = (uint64_t)blockIdx.x * XF_ROWS;
    const uint32_t rows = (uint32_t)((uint64_t)n - row0 < (uint64_t)XF_ROWS ? (uint64_t)n - row0 : (uint64_t)XF_ROWS);
    tile_load<10, XF_STRIDE, VEC>(in + row0 * 10, rows * 10, tile);
    __syncthreads();
    if (threadIdx.x < rows) {
        float* r = tile + threadIdx.x * XF_STRIDE;
        const float x = r[0], y = r[1], z = r[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float p0 = a.rot[3 * i] * x, p1 = a.rot[3 * i + 1] * y, p2 = a.rot[3 * i + 2] * z;
            const float s = (p0 + p1) + p2;
            const float m = s * a.scale;
            r[i] = m + a.trans[i];
        }
        const float W = a.quat[0], X = a.quat[1], Y = a.quat[2], Z = a.quat[3];
        const float qw = r[3], qx = r[4], qy = r[5], qz = r[6];
        {
            const float a0 = W * qw, a1 = X * qx, a2 = Y * qy, a3 = Z * qz;
            r[3] = ((a0 - a1) - a2) - a3;
        }
        {
            const float a0 = W * qx, a1 = X * qw, a2 = Y * qz, a3 = Z * qy;
            r[4] = ((a0 + a1) + a2) - a3;
        }
        {
            const float a0 = W * qy, a1 = X * qz, a2 = Y * qw, a3 = Z * qx;
            r[5] = ((a0 - a1) + a2) + a3;
        }
        {
            const float a0 = W * qz, a1 = X * qy, a2 = Y * qx, a3 = Z * qw;
            r[6] = ((a0 + a1) - a2) + a3;
        }
#pragma unroll
        for (int i = 7; i < 10; ++i) r[i] = r[i] + a.log_scale;
        if (min_scale) out_min_scale[row0 + threadIdx.x] = min_scale[row0 + threadIdx.x] * a.scale;
    }
    __syncthreads();
    tile_store<10, XF_STRIDE, VEC>(out + row0 * 10, rows * 10, tile);
}

// band L of one row in LDS (r at the band's first coefficient, m at D_L): out[k][c] = sum_j m[k][j] in[j][c], j ascending
template <int L>
BH_DEV void rotate_band(const float* m, float* r) {
    constexpr int M = 2 * L + 1;
    float v[M][3];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        v[j][0] = r[3 * j];
        v[j][1] = r[3 * j + 1];
        v[j][2] = r[3 * j + 2];
    }
#pragma unroll
    for (int k = 0; k < M; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float acc = m[k * M] * v[0][c];
#pragma unroll
            for (int j = 1; j < M; ++j) {
                const float p = m[k * M + j] * v[j][c];
                acc = acc + p;
            }
            r[3 * k + c] = acc;
        }
    }
}

template <int DEG, bool VEC>
__global__ __launch_bounds__(sh_rows<DEG>()) void scene_transform_sh_kernel(ShRot<DEG> d, uint32_t n, const float* in, float* out) {
    constexpr int RS = 3 * (DEG + 1) * (DEG + 1), RSP = RS | 1, ROWS = sh_rows<DEG>();
    __shared__ float tile[ROWS * RSP];
    const uint64_t row0 = (uint64_t)blockIdx.x * ROWS;
    const uint32_t rows = (uint32_t)((uint64_t)n - row0 < (uint64_t)ROWS ? (uint64_t)n - row0 : (uint64_t)ROWS);
    tile_load<RS, RSP, VEC>(in + row0 * RS, rows * RS, tile);
    __syncthreads();
    if (threadIdx.x < rows) {
        float* r = tile + threadIdx.x * RSP;   // (row 0, the DC term, passes through)
        rotate_band<1>(d.m, r + 3);
        if constexpr (DEG >= 2) rotate_band<2>(d.m + 9, r + 12);
        if constexpr (DEG >= 3) rotate_band<3>(d.m + 34, r + 27);
        if constexpr (DEG >= 4) rotate_band<4>(d.m + 83, r + 48);
    }
    __syncthreads();
    tile_store<RS, RSP, VEC>(out + row0 * RS, rows * RS, tile);
}

template <int DEG>
static int launch_sh(bh_ctx* ctx, const BhSceneTransform& T, uint32_t n, const float* in, float* out, bool vec) {
    ShRot<DEG> d;
    for (size_t k = 0; k < sizeof(d.m) / 4; ++k) d.m[k] = T.sh_rot[k];
    constexpr int ROWS = sh_rows<DEG>();
    const dim3 grid((uint32_t)(((uint64_t)n + ROWS - 1) / ROWS)), block(ROWS);
    if (vec)
        hipLaunchKernelGGL((scene_transform_sh_kernel<DEG, true>), grid, block, 0, ctx->stream, d, n, in, out);
    else
        hipLaunchKernelGGL((scene_transform_sh_kernel<DEG, false>), grid, block, 0, ctx->stream, d, n, in, out);
    BH_LAUNCH_CHECK(ctx, "scene_transform_sh_kernel");
    return 0;
}

// one thread per splat; the block's kept count (when asked for) goes to partial[block]: a grid-stride loop, counted per thread and
// summed over the block as integers
__global__ __launch_bounds__(SEL_WG) void select_region_kernel(BhSceneRegion g, const float* __restrict__ transforms, const float* __restrict__ raw_opac,
                                                               uint32_t n, float* __restrict__ keep, uint32_t* __restrict__ partial) {
    uint32_t mine = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * SEL_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SEL_WG) {
        const float* t = transforms + i * 10;
        const float x = t[0], y = t[1], z = t[2];
        const float dx = x - g.center[0], dy = y - g.center[1], dz = z - g.center[2];
        float p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float a0 = g.rot[k] * dx, a1 = g.rot[3 + k] * dy, a2 = g.rot[6 + k] * dz;
            p[k] = (a0 + a1) + a2;
        }
        bool inside;
        if (g.kind == BH_REGION_BOX) {
            inside = fabsf(p[0]) <= g.half_extent[0] && fabsf(p[1]) <= g.half_extent[1] && fabsf(p[2]) <= g.half_extent[2];
        } else {
            const float q0 = p[0] / g.half_extent[0], q1 = p[1] / g.half_extent[1], q2 = p[2] / g.half_extent[2];
            const float s0 = q0 * q0, s1 = q1 * q1, s2 = q2 * q2;
            inside = (s0 + s1) + s2 <= 1.0f;
        }
        if (g.invert) inside = !inside;
        const float top = fmaxf(fmaxf(fabsf(x), fabsf(y)), fabsf(z));
        bool k = inside && x == x && y == y && z == z && top < __builtin_inff();   // a non-finite mean is never kept
        if (raw_opac) k = k && raw_opac[i] >= g.min_raw_opacity;                    // (false for a NaN opacity)
        keep[i] = k ? 1.0f : 0.0f;
        mine += k ? 1u : 0u;
    }
    if (partial) {
        __shared__ uint32_t sums[SEL_WG];
        sums[threadIdx.x] = mine;
        __syncthreads();
        for (int s = SEL_WG / 2; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) sums[threadIdx.x] += sums[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) partial[blockIdx.x] = sums[0];
    }
}

// partial[blocks] -> partial[blocks] (the total), one block, in a fixed order
__global__ __launch_bounds__(SEL_WG) void select_total_kernel(uint32_t* __restrict__ partial, uint32_t blocks) {
    __shared__ uint32_t sums[SEL_WG];
    uint32_t mine = 0;
    for (uint32_t b = threadIdx.x; b < blocks; b += SEL_WG) mine += partial[b];
    sums[threadIdx.x] = mine;
    __syncthreads();
    for (int s = SEL_WG / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sums[threadIdx.x] += sums[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blocks] = sums[0];
}

struct Span {
    const void* p;
    size_t bytes;
};
static bool overlaps(const Span& a, const Span& b) {
    if (!a.p || !b.p || a.bytes == 0 || b.bytes == 0) return false;
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}
static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace bh

using namespace bh;

extern "C" {

int bh_scene_transform_make(const double quat_wxyz[4], const double trans[3], double scale, BhSceneTransform* out) {
    if (!quat_wxyz || !trans || !out) return BH_ERR_INVALID_ARG;
    return bh_scene::fill_record(quat_wxyz, trans, scale, out) ? 0 : BH_ERR_INVALID_ARG;
}

int bh_scene_transform_compose(const BhSceneTransform* a, const BhSceneTransform* b, BhSceneTransform* out) {
    if (!a || !b || !out) return BH_ERR_INVALID_ARG;
    return bh_scene::compose(*a, *b, out) ? 0 : BH_ERR_INVALID_ARG;
}

int bh_scene_transform_invert(const BhSceneTransform* a, BhSceneTransform* out) {
    if (!a || !out) return BH_ERR_INVALID_ARG;
    return bh_scene::invert(*a, out) ? 0 : BH_ERR_INVALID_ARG;
}

int bh_camera_apply_scene_transform(const BhCamera* in, const BhSceneTransform* T, BhCamera* out) {
    if (!in || !T || !out) return BH_ERR_INVALID_ARG;
    if (!std::isfinite(T->s) || !(T->s > 0.0)) return BH_ERR_INVALID_ARG;
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(T->q[k])) return BH_ERR_INVALID_ARG;
    if (!bh_scene::finite3(T->t)) return BH_ERR_INVALID_ARG;
    bh_scene::camera_apply(*in, *T, out);
    return 0;
}

int bh_splats_transform(bh_ctx* ctx, const BhSceneTransform* T, uint32_t n, uint32_t num_coeffs, const float* transforms, const float* sh_coeffs,
                        const float* min_scale, float* out_transforms, float* out_sh, float* out_min_scale) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!T) return set_error(ctx, BH_ERR_INVALID_ARG, "splats_transform: null record");
    uint32_t deg = 0;
    while ((deg + 1) * (deg + 1) < num_coeffs) ++deg;
    if (num_coeffs == 0 || deg > 4 || (deg + 1) * (deg + 1) != num_coeffs)
        return set_error(ctx, BH_ERR_INVALID_ARG, "splats_transform: num_coeffs must be (d+1)^2, d <= 4");
    if (n == 0) return 0;
    if (!transforms || !out_transforms || (sh_coeffs && !out_sh) || (min_scale && !out_min_scale))
        return set_error(ctx, BH_ERR_INVALID_ARG, "splats_transform: null argument");
    const size_t sh_bytes = (size_t)n * num_coeffs * 12;
    // each output is its own input or overlaps nothing: [0..2] inputs, [3..5] their outputs
    const Span spans[6] = {{transforms, (size_t)n * 40}, {sh_coeffs, sh_bytes}, {min_scale, (size_t)n * 4},
                           {out_transforms, (size_t)n * 40}, {sh_coeffs ? out_sh : nullptr, sh_bytes}, {min_scale ? out_min_scale : nullptr, (size_t)n * 4}};
    for (int o = 3; o < 6; ++o)
        for (int k = 0; k < 6; ++k) {
            if (k == o || (k == o - 3 && spans[k].p == spans[o].p)) continue;
            if (overlaps(spans[o], spans[k])) return set_error(ctx, BH_ERR_INVALID_ARG, "splats_transform: an output overlaps another argument (in place means the same pointer)");
        }
    BH_HIP(ctx, hipSetDevice(ctx->device));
    ProfScope ps(ctx, "SplatsTransform");
    const bool identity = bh_scene::is_identity(*T);
    if (identity || deg == 0) {
        // nothing to rotate in the DC term: the bits of the input
        if (sh_coeffs && out_sh != sh_coeffs) BH_HIP(ctx, hipMemcpyAsync(out_sh, sh_coeffs, sh_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (identity) {
        if (out_transforms != transforms) BH_HIP(ctx, hipMemcpyAsync(out_transforms, transforms, (size_t)n * 40, hipMemcpyDeviceToDevice, ctx->stream));
        if (min_scale && out_min_scale != min_scale) BH_HIP(ctx, hipMemcpyAsync(out_min_scale, min_scale, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        return 0;
    }
    XfArgs a;
    for (int k = 0; k < 9; ++k) a.rot[k] = T->rot[k];
    for (int k = 0; k < 4; ++k) a.quat[k] = T->quat[k];
    for (int k = 0; k < 3; ++k) a.trans[k] = T->trans[k];
    a.scale = T->scale;
    a.log_scale = T->log_scale;
    {
        const dim3 grid((uint32_t)(((uint64_t)n + XF_ROWS - 1) / XF_ROWS)), block(XF_ROWS);
        if (aligned16(transforms) && aligned16(out_transforms))
            hipLaunchKernelGGL((scene_transform_rows_kernel<true>), grid, block, 0, ctx->stream, a, n, transforms, min_scale, out_transforms, out_min_scale);
        else
            hipLaunchKernelGGL((scene_transform_rows_kernel<false>), grid, block, 0, ctx->stream, a, n, transforms, min_scale, out_transforms, out_min_scale);
        BH_LAUNCH_CHECK(ctx, "scene_transform_rows_kernel");
    }
    if (sh_coeffs && deg > 0) {
        const bool vec = aligned16(sh_coeffs) && aligned16(out_sh);
        switch (deg) {
            case 1: return launch_sh<1>(ctx, *T, n, sh_coeffs, out_sh, vec);
            case 2: return launch_sh<2>(ctx, *T, n, sh_coeffs, out_sh, vec);
            case 3: return launch_sh<3>(ctx, *T, n, sh_coeffs, out_sh, vec);
            default: return launch_sh<4>(ctx, *T, n, sh_coeffs, out_sh, vec);
        }
    }
    return 0;
}

int bh_splats_select_region(bh_ctx* ctx, const BhSceneRegion* region, const float* transforms, const float* raw_opacities, uint32_t n, float* keep,
                            uint32_t* count) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!region) return set_error(ctx, BH_ERR_INVALID_ARG, "select_region: null region");
    if (region->kind != BH_REGION_BOX && region->kind != BH_REGION_ELLIPSOID) return set_error(ctx, BH_ERR_INVALID_ARG, "select_region: unknown kind");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(region->half_extent[k]) || !(region->half_extent[k] > 0.0f) || !std::isfinite(region->center[k]))
            return set_error(ctx, BH_ERR_INVALID_ARG, "select_region: half extents must be finite and > 0, the centre finite");
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(region->rot[k])) return set_error(ctx, BH_ERR_INVALID_ARG, "select_region: an axis is not finite");
    if (region->min_raw_opacity != region->min_raw_opacity) return set_error(ctx, BH_ERR_INVALID_ARG, "select_region: the opacity floor is not a number");
    if (n > 0 && (!transforms || !keep)) return set_error(ctx, BH_ERR_INVALID_ARG, "select_region: null argument");
    if (n == 0) {
        if (count) *count = 0;
        return 0;
    }
    BH_HIP(ctx, hipSetDevice(ctx->device));
    ProfScope ps(ctx, "SelectRegion");
    const uint64_t want = ((uint64_t)n + SEL_WG - 1) / SEL_WG;
    const uint32_t blocks = (uint32_t)(want < SEL_MAX_BLOCKS ? want : SEL_MAX_BLOCKS);
    uint32_t* partial = nullptr;
    if (count) {
        partial = (uint32_t*)ensure(ctx, SLOT_SCENE, ((size_t)blocks + 1) * 4);
        if (!partial) return BH_ERR_OOM;
    }
    hipLaunchKernelGGL(select_region_kernel, dim3(blocks), dim3(SEL_WG), 0, ctx->stream, *region, transforms, raw_opacities, n, keep, partial);
    BH_LAUNCH_CHECK(ctx, "select_region_kernel");
    if (count) {
        hipLaunchKernelGGL(select_total_kernel, dim3(1), dim3(SEL_WG), 0, ctx->stream, partial, blocks);
        BH_LAUNCH_CHECK(ctx, "select_total_kernel");
        BH_HIP(ctx, hipMemcpyAsync(ctx->host_counters, partial + blocks, 4, hipMemcpyDeviceToHost, ctx->stream));
        BH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        deliver_pending_loss(ctx);
        *count = ctx->host_counters[0];
    }
    return 0;
}

}  // extern "C"
