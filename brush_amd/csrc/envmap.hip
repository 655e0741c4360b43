// envmap.hip — environment maps (include/brush_hip_envmap.h): a cubemap E[6,R,R,3] composited behind a rendered frame,
// the gradient to the frame and to the table, and Adam on the table, all on the device.  The header is the arithmetic's specification
// (tests/envmap_ref.py restates it); env_taps / env_colour below are its one copy on the device.
//
//   envmap_composite_kernel   streaming: one float4 in, one out per pixel (a wave: 1 KB of one row), the table through the cache
//   envmap_max_kernel         m = max |v_out rgb| as an unsigned maximum of the bit patterns (order-free): at most one u32 atomic per
//                             block, and none from a block whose maximum the word already holds (8192 atomics on the one word, one
//                             per wave, took 98 us at 1080p: they serialise)
//   envmap_backward_kernel    a block owns a 16 x 16 tile of pixels: v_img, and the tile's share of v_E reduced BY DESTINATION before it
//                             leaves the block.  At 1080p a texel of R = 64 covers ~2000 pixels, and atomics on one address serialise
//                             (EXPERIMENTS.md, K17: six times slower), so the tile's distinct texels are numbered in an LDS hash
//                             table (lift.hip numbers a tile's labels the same way, with a bit set: here the key space is 6 R^2), the
//                             contributions are added there as 64-bit integers, and every occupied entry leaves with ONE 64-bit integer
//                             atomic per channel.  A wave whose pixels all hit one texel (the common case once a texel is wider than
//                             the tile) adds them up in registers first; reducing a wave's two to four texels at a texel edge the
//                             same way, one after the other, was measured and lost to the lanes' own LDS adds.
//                             Only a tile with more distinct texels than the table's
//                             probe limit finds room for (R large against the frame: nothing to reduce, no contention either) sends
//                             the rest straight to memory.
//   envmap_final_kernel       v_E = the integer sums / S, and the Adam step of every texel
// Integer sums and an unsigned maximum: nothing depends on the order in which lanes, waves or blocks arrive.
// The table itself — a bh_envmap is a ParamTable of one row of 6 R R 3 with f32 moments, plus the sums and the maximum's word of the
// backward in flight — and every entry point that only manages it are param_table.h's, shared with exposure.hip and bilagrid.hip.
#include "param_table.h"

namespace bh {

namespace {

constexpr int ENV_WG = 256;
constexpr uint32_t ENV_STREAM_MAX_BLOCKS = 2048;   // final: grid-stride, at most 8 blocks of 256 per CU
constexpr uint32_t ENV_TILE = 16;                  // the backward's tile: 16 x 16 pixels, one per lane
constexpr uint32_t ENV_CAP = 512;                  // entries of the tile's hash table: 2 KB of keys + 12 KB of sums
constexpr uint32_t ENV_CAP_BITS = 9;
constexpr uint32_t ENV_PROBES = 8;                 // linear probes before a contribution goes to memory instead
constexpr uint32_t ENV_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t ENV_MAX_BLOCKS = 1024;          // the max pass: one conditional atomic per block

struct EnvGeom {
    float vm[9];   // the rotation's columns
    float fx, fy, cx, cy;
    uint32_t w, h, res;
    float half, rmax;   // R / 2, R - 1
};

struct EnvTaps {
    uint32_t texel[4];   // (face R + j) R + i
    float w[4];
};

BH_DEV void env_axis(float s, const EnvGeom& g, uint32_t& i0, uint32_t& i1, float& f) {
    float u = __builtin_fmaf(s, g.half, g.half) - 0.5f;
    u = fminf(fmaxf(u, 0.0f), g.rmax);   // (a NaN becomes 0)
    const float fl = floorf(u);
    i0 = (uint32_t)fl;
    i1 = i0 + 1u < g.res ? i0 + 1u : g.res - 1u;
    f = u - fl;
}

BH_DEV EnvTaps env_taps(const EnvGeom& g, uint32_t x, uint32_t y) {
    const float dx = (((float)x + 0.5f) - g.cx) / g.fx, dy = (((float)y + 0.5f) - g.cy) / g.fy;
    float d[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = __builtin_fmaf(g.vm[3 * i + 1], dy, g.vm[3 * i] * dx) + g.vm[3 * i + 2];
    const float a0 = fabsf(d[0]), a1 = fabsf(d[1]), a2 = fabsf(d[2]);
    uint32_t axis = 0u;
    float am = a0;
    if (a1 > am) { axis = 1u; am = a1; }
    if (a2 > am) { axis = 2u; am = a2; }
    const float major = axis == 0u ? d[0] : (axis == 1u ? d[1] : d[2]);
    const float a = axis == 0u ? d[1] : (axis == 1u ? d[2] : d[0]);
    const float b = axis == 0u ? d[2] : (axis == 1u ? d[0] : d[1]);
    const uint32_t face = 2u * axis + (major < 0.0f ? 1u : 0u);
    uint32_t i0, i1, j0, j1;
    float fu, fv;
    env_axis(a / am, g, i0, i1, fu);
    env_axis(b / am, g, j0, j1, fv);
    const float gu = 1.0f - fu, gv = 1.0f - fv;
    const uint32_t row0 = (face * g.res + j0) * g.res, row1 = (face * g.res + j1) * g.res;
    EnvTaps t;
    t.texel[0] = row0 + i0; t.texel[1] = row0 + i1; t.texel[2] = row1 + i0; t.texel[3] = row1 + i1;
    t.w[0] = gu * gv; t.w[1] = fu * gv; t.w[2] = gu * fv; t.w[3] = fu * fv;
    return t;
}

BH_DEV void env_colour(const float* __restrict__ table, const EnvTaps& t, float (&e)[3]) {
    const float* p0 = table + (size_t)t.texel[0] * 3;
    const float* p1 = table + (size_t)t.texel[1] * 3;
    const float* p2 = table + (size_t)t.texel[2] * 3;
    const float* p3 = table + (size_t)t.texel[3] * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) e[c] = __builtin_fmaf(t.w[3], p3[c], __builtin_fmaf(t.w[2], p2[c], __builtin_fmaf(t.w[1], p1[c], t.w[0] * p0[c])));
}

// E'(d) of the gradient to the frame: the same taps in f64, every operation rounded on its own (-ffp-contract=off)
BH_DEV void env_colour_f64(const float* __restrict__ table, const EnvTaps& t, double (&e)[3]) {
    const float* p0 = table + (size_t)t.texel[0] * 3;
    const float* p1 = table + (size_t)t.texel[1] * 3;
    const float* p2 = table + (size_t)t.texel[2] * 3;
    const float* p3 = table + (size_t)t.texel[3] * 3;
    const double w0 = t.w[0], w1 = t.w[1], w2 = t.w[2], w3 = t.w[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) e[c] = w3 * (double)p3[c] + (w2 * (double)p2[c] + (w1 * (double)p1[c] + w0 * (double)p0[c]));
}

// grid (ceil(w / 64), ceil(h / 4)): a wave takes 64 pixels of one row (1 KB, contiguous), a block four rows; no division finds x and y
__global__ __launch_bounds__(ENV_WG) void envmap_composite_kernel(EnvGeom g, const float* __restrict__ table, const float4* img, float4* out) {
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= g.w || y >= g.h) return;
    const size_t p = (size_t)y * g.w + x;
    const float4 v = img[p];
    const EnvTaps t = env_taps(g, x, y);
    float e[3];
    env_colour(table, t, e);
    const float oma = 1.0f - v.w;
    out[p] = make_float4(__builtin_fmaf(oma, e[0], v.x), __builtin_fmaf(oma, e[1], v.y), __builtin_fmaf(oma, e[2], v.z), v.w);
}

__global__ __launch_bounds__(ENV_WG) void envmap_max_kernel(const float4* __restrict__ v_out, uint32_t pixels, uint32_t* __restrict__ ctl) {
    const uint32_t stride = gridDim.x * ENV_WG;
    uint32_t m = 0u;
    for (uint32_t p = blockIdx.x * ENV_WG + threadIdx.x; p < pixels; p += stride) {
        const float4 v = v_out[p];
        m = max(m, max(f2u(v.x) & 0x7FFFFFFFu, max(f2u(v.y) & 0x7FFFFFFFu, f2u(v.z) & 0x7FFFFFFFu)));   // (a NaN's bits lie above the infinity's)
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, s, 64));
    __shared__ uint32_t wave_max[ENV_WG / 64];
    if ((threadIdx.x & 63u) == 0u) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0u) {
#pragma unroll
        for (int k = 1; k < ENV_WG / 64; ++k) m = max(m, wave_max[k]);
        if (m > __hip_atomic_load(&ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_fetch_max(&ctl[0], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// S = 2^(61 - e - L) from the bits of m (finite, > 0): e is the exponent field of (double)m - 1022 (every f32 is a normal f64)
BH_DEV double env_scale(uint32_t m_bits, uint32_t log_pixels) {
    const int e = (int)(((unsigned long long)__double_as_longlong((double)u2f(m_bits)) >> 52) & 0x7FFull) - 1022;
    return __longlong_as_double((long long)(1023 + 61 - e - (int)log_pixels) << 52);
}
BH_DEV bool env_finite_bits(uint32_t m_bits) { return m_bits < 0x7F800000u; }

// the slot of `key` in the tile's table (claimed if it is new), or ENV_CAP: no room within the probe limit
BH_DEV uint32_t env_slot(uint32_t* s_key, uint32_t key) {
    uint32_t slot = (key * 2654435761u) >> (32u - ENV_CAP_BITS);
    for (uint32_t i = 0; i < ENV_PROBES; ++i) {
        const uint32_t prev = atomicCAS(&s_key[slot], ENV_EMPTY, key);
        if (prev == ENV_EMPTY || prev == key) return slot;
        slot = (slot + 1u) & (ENV_CAP - 1u);
    }
    return ENV_CAP;
}

BH_DEV void env_add(unsigned long long* s_acc, unsigned long long* __restrict__ acc, uint32_t slot, uint32_t key, const long long (&q)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (q[c] == 0ll) continue;
        if (slot < ENV_CAP) __hip_atomic_fetch_add(&s_acc[slot * 3u + c], (unsigned long long)q[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else __hip_atomic_fetch_add(&acc[(size_t)key * 3 + c], (unsigned long long)q[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// grid: the frame's tiles, row-major.  v_img may be v_out: a lane reads its pixel before it writes it, and the max pass is behind us.
__global__ __launch_bounds__(ENV_WG) void envmap_backward_kernel(EnvGeom g, const float* __restrict__ table, const float4* __restrict__ img, const float4* v_out,
                                                                 float4* v_img, uint32_t tiles_x, uint32_t log_pixels, const uint32_t* __restrict__ ctl,
                                                                 unsigned long long* __restrict__ acc) {
    __shared__ uint32_t s_key[ENV_CAP];
    __shared__ unsigned long long s_acc[ENV_CAP * 3];
    const uint32_t m_bits = ctl[0];
    if (!env_finite_bits(m_bits)) return;   // (refused on the host where the host looks; here: nothing is written)
    for (uint32_t i = threadIdx.x; i < ENV_CAP; i += ENV_WG) s_key[i] = ENV_EMPTY;
    for (uint32_t i = threadIdx.x; i < ENV_CAP * 3; i += ENV_WG) s_acc[i] = 0ull;
    __syncthreads();
    const uint32_t x = (blockIdx.x % tiles_x) * ENV_TILE + (threadIdx.x & (ENV_TILE - 1u));
    const uint32_t y = (blockIdx.x / tiles_x) * ENV_TILE + threadIdx.x / ENV_TILE;
    const bool inside = x < g.w && y < g.h;
    const int lane = threadIdx.x & 63;
    EnvTaps t{};
    float gr[3] = {0.0f, 0.0f, 0.0f};
    bool contrib = false;
    if (inside) {
        const size_t p = (size_t)y * g.w + x;
        const float4 v = v_out[p];
        const float oma = 1.0f - img[p].w;
        t = env_taps(g, x, y);
        double e[3];
        env_colour_f64(table, t, e);
        const float s = (float)((double)v.z * e[2] + ((double)v.y * e[1] + (double)v.x * e[0]));
        v_img[p] = make_float4(v.x, v.y, v.z, v.w - s);
        contrib = m_bits != 0u && oma != 0.0f;
        gr[0] = oma * v.x; gr[1] = oma * v.y; gr[2] = oma * v.z;
    }
    const double S = m_bits != 0u ? env_scale(m_bits, log_pixels) : 1.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long act = __ballot(contrib);
        if (act == 0ull) continue;
        long long q[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = contrib ? llrint((double)(gr[c] * t.w[k]) * S) : 0ll;
        const uint32_t key = t.texel[k];
        const int first = __ffsll((long long)act) - 1;
        const uint32_t lead = (uint32_t)__shfl((int)key, first, 64);
        if (__ballot(contrib && key != lead) == 0ull) {   // the wave's pixels share the texel: one entry, one add per channel
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int s = 32; s >= 1; s >>= 1) q[c] += __shfl_xor(q[c], s, 64);
            if (lane == first) env_add(s_acc, acc, env_slot(s_key, lead), lead, q);
        } else if (contrib) {
            env_add(s_acc, acc, env_slot(s_key, key), key, q);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < ENV_CAP; i += ENV_WG) {
        const uint32_t key = s_key[i];
        if (key == ENV_EMPTY) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned long long sum = s_acc[i * 3u + c];
            if (sum != 0ull) __hip_atomic_fetch_add(&acc[(size_t)key * 3 + c], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

struct EnvAdam {
    float lr, beta1, beta2, omb1, omb2, eps, c1, c2, gscale;
    uint32_t t;
};

// dequant: grad = the integer sums / S.  adam: one step of every texel on gscale * grad.
__global__ __launch_bounds__(ENV_WG) void envmap_final_kernel(uint32_t cells, uint32_t log_pixels, int dequant, int adam, EnvAdam a, const uint32_t* __restrict__ ctl, uint32_t* __restrict__ t_dev,
                                                              const unsigned long long* __restrict__ acc, float* __restrict__ grad, float* __restrict__ param,
                                                              float* __restrict__ m1, float* __restrict__ m2) {
    const uint32_t m_bits = ctl[0];
    if (!env_finite_bits(m_bits)) return;   // (of the backward this launch belongs to)
    const double S = dequant && m_bits != 0u ? env_scale(m_bits, log_pixels) : 1.0;
    const uint32_t stride = gridDim.x * ENV_WG;
    for (uint32_t e = blockIdx.x * ENV_WG + threadIdx.x; e < cells; e += stride) {
        float gv;
        if (dequant) {
            gv = (float)((double)(long long)acc[e] / S);
            grad[e] = gv;
        } else {
            gv = grad[e];
        }
        if (adam) {
            const float gs = a.gscale * gv;
            const float n1 = a.beta1 * m1[e] + a.omb1 * gs;
            const float n2 = a.beta2 * m2[e] + (a.omb2 * gs) * gs;
            m1[e] = n1;
            m2[e] = n2;
            param[e] = param[e] - a.lr * ((n1 / a.c1) / (sqrtf(n2 / a.c2) + a.eps));
        }
    }
    if (adam && blockIdx.x == 0 && threadIdx.x == 0) t_dev[0] = a.t;
}

EnvGeom env_geom(const bh_envmap* map, const BhCamera& cam, uint32_t h, uint32_t w) {
    EnvGeom g;
    for (int i = 0; i < 9; ++i) g.vm[i] = cam.vm[i];
    g.fx = cam.fx; g.fy = cam.fy; g.cx = cam.cx; g.cy = cam.cy;
    g.w = w; g.h = h; g.res = map->res;
    g.half = (float)map->res * 0.5f;
    g.rmax = (float)(map->res - 1u);
    return g;
}

uint32_t stream_grid(uint64_t items) {
    const uint64_t blocks = (items + ENV_WG - 1) / ENV_WG;
    return (uint32_t)(blocks < ENV_STREAM_MAX_BLOCKS ? blocks : ENV_STREAM_MAX_BLOCKS);
}

uint32_t ceil_log2(uint64_t n) {
    uint32_t l = 0;
    while (((uint64_t)1 << l) < n) ++l;
    return l;
}

// beta^t in f64 by squaring, in the header's order
double pow_by_squaring(double b, uint32_t t) {
    double p = 1.0;
    while (t) {
        if (t & 1u) p = p * b;
        b = b * b;
        t >>= 1;
    }
    return p;
}

// the update of step map->t_host + 1 on the gradient as it stands (dequant: as the sums say); the map counts it once it is queued
int launch_final(bh_ctx* ctx, bh_envmap* map, uint32_t log_pixels, bool dequant, bool adam, float gscale) {
    EnvAdam a{};
    if (adam) {
        a.t = map->t_host + 1u;
        a.lr = (float)map->lr; a.beta1 = (float)map->beta1; a.beta2 = (float)map->beta2;
        a.omb1 = (float)(1.0 - map->beta1); a.omb2 = (float)(1.0 - map->beta2);
        a.eps = (float)map->eps;
        a.c1 = (float)(1.0 - pow_by_squaring(map->beta1, a.t));
        a.c2 = (float)(1.0 - pow_by_squaring(map->beta2, a.t));
        a.gscale = gscale;
    }
    hipLaunchKernelGGL(envmap_final_kernel, dim3(stream_grid(map->row)), dim3(ENV_WG), 0, ctx->stream, (uint32_t)map->row, log_pixels, dequant ? 1 : 0,
                       adam ? 1 : 0, a, map->ctl, map->t, map->acc, map->grad, map->param, static_cast<float*>(map->m1), static_cast<float*>(map->m2));
    BH_LAUNCH_CHECK(ctx, "envmap_final_kernel");
    if (adam) map->t_host = a.t;
    return 0;
}

}  // namespace

int check_envmap_frame(bh_ctx* ctx, const BhCamera* cam, uint32_t h, uint32_t w, const char* who) {
    if (!cam) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": null argument");
    BH_TRY(check_image(ctx, h, w, /*below_2_31=*/true, who));
    if (cam->model != BH_CAMERA_PINHOLE)
        return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": an environment map needs a pinhole camera (no other model can be unprojected to a ray)");
    return 0;
}

int launch_envmap_composite(bh_ctx* ctx, const bh_envmap* map, const BhCamera& cam, const float* img, uint32_t h, uint32_t w, float* out) {
    hipLaunchKernelGGL(envmap_composite_kernel, dim3((w + 63u) / 64u, (h + 3u) / 4u), dim3(ENV_WG), 0, ctx->stream, env_geom(map, cam, h, w), map->param,
                       reinterpret_cast<const float4*>(img), reinterpret_cast<float4*>(out));
    BH_LAUNCH_CHECK(ctx, "envmap_composite_kernel");
    return 0;
}

int launch_envmap_backward(bh_ctx* ctx, bh_envmap* map, const BhCamera& cam, const float* img, const float* v_out, uint32_t h, uint32_t w, float* v_img,
                           bool update, float gscale, bool check_host) {
    const uint32_t pixels = h * w, log_pixels = ceil_log2(pixels);
    BH_HIP(ctx, hipMemsetAsync(map->acc, 0, map->row * 8 + 16, ctx->stream));   // the sums and, behind them, the maximum's word
    hipLaunchKernelGGL(envmap_max_kernel, dim3(std::min(stream_grid(pixels), ENV_MAX_BLOCKS)), dim3(ENV_WG), 0, ctx->stream, reinterpret_cast<const float4*>(v_out), pixels, map->ctl);
    BH_LAUNCH_CHECK(ctx, "envmap_max_kernel");
    if (check_host) {
        uint32_t m_bits = 0;
        BH_TRY(read_back(ctx, &m_bits, map->ctl, 4));
        if (m_bits >= 0x7F800000u) return set_error(ctx, BH_ERR_INVALID_ARG, "envmap_backward: v_out holds a NaN or an infinity (nothing was written)");
    }
    const uint32_t tiles_x = (w + ENV_TILE - 1) / ENV_TILE, tiles_y = (h + ENV_TILE - 1) / ENV_TILE;
    hipLaunchKernelGGL(envmap_backward_kernel, dim3(tiles_x * tiles_y), dim3(ENV_WG), 0, ctx->stream, env_geom(map, cam, h, w), map->param,
                       reinterpret_cast<const float4*>(img), reinterpret_cast<const float4*>(v_out), reinterpret_cast<float4*>(v_img), tiles_x, log_pixels,
                       map->ctl, map->acc);
    BH_LAUNCH_CHECK(ctx, "envmap_backward_kernel");
    return launch_final(ctx, map, log_pixels, true, update, gscale);
}

int launch_envmap_adam(bh_ctx* ctx, bh_envmap* map, float gscale) { return launch_final(ctx, map, 0u, false, true, gscale); }

}  // namespace bh

using namespace bh;

extern "C" {

int bh_envmap_create(bh_ctx* ctx, uint32_t resolution, bh_envmap** map) {
    BH_TRY(param_table_create_args(ctx, map, 1, "envmap_create"));
    if (resolution == 0 || resolution > BH_ENVMAP_MAX_RESOLUTION) return set_error(ctx, BH_ERR_INVALID_ARG, "envmap_create: the resolution must be 1 .. 1024");
    const size_t cells = (size_t)6 * resolution * resolution * 3;
    bh_envmap* m = new bh_envmap;
    BH_TRY(param_table_create(ctx, m, 1, cells, cells * 8 + 16, /*pattern=*/nullptr, "envmap_create"));   // (a new map is black)
    m->res = resolution;
    m->acc = static_cast<unsigned long long*>(m->mem);
    m->ctl = reinterpret_cast<uint32_t*>(m->acc + cells);
    *map = m;
    return 0;
}

int bh_envmap_destroy(bh_ctx* ctx, bh_envmap* map) { return param_table_destroy(ctx, PT_ENVMAP, map, "envmap_destroy"); }

int bh_envmap_set_params(bh_ctx* ctx, bh_envmap* map, const float* host) { return param_table_set_params(ctx, PT_ENVMAP, map, 1, 1, host, "envmap_set_params"); }

int bh_envmap_get_params(bh_ctx* ctx, bh_envmap* map, float* host) {
    return param_table_get_rows(ctx, PT_ENVMAP, map, &ParamTable::param, 1, 1, host, "envmap_get_params");
}

int bh_envmap_get_grad(bh_ctx* ctx, bh_envmap* map, float* host) {
    return param_table_get_rows(ctx, PT_ENVMAP, map, &ParamTable::grad, 1, 1, host, "envmap_get_grad");
}

int bh_envmap_get_state(bh_ctx* ctx, bh_envmap* map, float* m1, float* m2, uint32_t* t) {
    return param_table_get_state(ctx, PT_ENVMAP, map, 1, m1, m2, t, "envmap_get_state");
}

int bh_envmap_set_state(bh_ctx* ctx, bh_envmap* map, const float* m1, const float* m2, uint32_t t) {
    BH_TRY(param_table_set_state(ctx, PT_ENVMAP, map, 1, m1, m2, t, "envmap_set_state"));
    map->t_host = t;
    return 0;
}

int bh_envmap_set_adam(bh_ctx* ctx, bh_envmap* map, double lr, double beta1, double beta2, double eps) {
    return param_table_set_adam(ctx, PT_ENVMAP, map, lr, beta1, beta2, eps, "envmap_set_adam");
}

int bh_envmap_composite(bh_ctx* ctx, bh_envmap* map, const BhCamera* cam, const float* img_hwc4, uint32_t h, uint32_t w, float* out_hwc4) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!img_hwc4 || !out_hwc4) return set_error(ctx, BH_ERR_INVALID_ARG, "envmap_composite: null argument");
    BH_TRY(check_envmap_frame(ctx, cam, h, w, "envmap_composite"));
    BH_TRY(param_table_owned(ctx, PT_ENVMAP, map, "envmap_composite"));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    ProfScope ps(ctx, "EnvMap");
    return launch_envmap_composite(ctx, map, *cam, img_hwc4, h, w, out_hwc4);
}

int bh_envmap_backward(bh_ctx* ctx, bh_envmap* map, const BhCamera* cam, const float* img_hwc4, const float* v_out, uint32_t h, uint32_t w, float* v_img,
                       int update) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!img_hwc4 || !v_out || !v_img) return set_error(ctx, BH_ERR_INVALID_ARG, "envmap_backward: null argument");
    BH_TRY(check_envmap_frame(ctx, cam, h, w, "envmap_backward"));
    BH_TRY(param_table_owned(ctx, PT_ENVMAP, map, "envmap_backward"));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    ProfScope ps(ctx, "EnvMap");
    return launch_envmap_backward(ctx, map, *cam, img_hwc4, v_out, h, w, v_img, update != 0, 1.0f, /*check_host=*/true);
}

int bh_train_set_envmap(bh_ctx* ctx, bh_envmap* map) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    BH_TRY(param_table_attachable(ctx, PT_ENVMAP, map, "train_set_envmap"));
    ctx->terms.envmap = map;
    return 0;
}

}  // extern "C"
