// tsdf.hip — mesh extraction (include/brush_hip_mesh.h): fusion of depth maps into a dense TSDF volume, marching
// tetrahedra on the Kuhn split of its cubes, and the triangle-mesh PLY.  Not in the reference.
//
// Integration is the hot path: 8 bytes of {T, W} and 12 of colour per sample, read and written.  One launch takes up to
// BH_TSDF_MAX_BATCH views from its kernel arguments (scalar loads, no per-thread camera traffic); a thread owns one sample, keeps
// it in registers across the views and stores it once, if a view touched it.  A block is 64 x 4 x 1 samples: a wave is one row of 64
// consecutive x (512 contiguous bytes of tw, 768 of rgb), and a wave whose samples all miss a view's frustum leaves that view behind
// the projection arithmetic with an empty exec mask — before the depth map is touched.  No LDS, no barrier, no atomics.  Measured
// (DESIGN.md §6q): what binds is the per-view arithmetic the contract fixes (18 unfused multiplies and adds, two IEEE divisions),
// not the sweep over the volume; batching saves the seven sweeps.  Issuing all views' depth gathers before the first update (a
// two-phase, fully unrolled loop) was measured and changed nothing for a batch, so the loop stays the plain one.
//
// Extraction is three phases without atomics: classify (per sample the mask of owned edges that carry a vertex, per cube the triangle
// count), two inclusive scans (scan.hip), emit (a vertex index is scan[owner] - popcount(mask) + popcount(mask below d)).
#include <cmath>
#include <cstring>
#include <string>

#include "context.h"
#include "device_math.h"
#include "device_tsdf.h"

namespace bh {

struct TsdfGridDev {
    float ox, oy, oz, vs;
    uint32_t nx, ny, nz;
    float trunc, max_weight;
    float2* tw;
    float* rgb;
};

constexpr int TSDF_BX = 64, TSDF_BY = 4, TSDF_WG = TSDF_BX * TSDF_BY;
constexpr uint32_t TSDF_MAX_BLOCKS = 1u << 20;   // (blocks x threads must stay below 2^32; larger volumes stride)

__global__ __launch_bounds__(TSDF_WG) void tsdf_clear_kernel(TsdfGridDev g, uint32_t n) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    g.tw[s] = make_float2(1.0f, 0.0f);
    if (g.rgb) {
        float* c = g.rgb + (size_t)s * 3;
        c[0] = 0.0f; c[1] = 0.0f; c[2] = 0.0f;
    }
}

// COLOUR: the volume has rgb and the batch has images (then every view has one)
template <bool COLOUR>
__global__ __launch_bounds__(TSDF_WG) void tsdf_integrate_kernel(const TsdfGridDev g, const TsdfBatch b, const uint32_t n_views, const float depth_min,
                                                                 const float depth_max, const float alpha_min, const uint32_t blocks_x, const uint32_t blocks_y,
                                                                 const uint32_t n_blocks) {
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint32_t bxi = blk % blocks_x, rest = blk / blocks_x;
        const uint32_t byi = rest % blocks_y, k = rest / blocks_y;
        const uint32_t i = bxi * TSDF_BX + (threadIdx.x & (TSDF_BX - 1)), j = byi * TSDF_BY + (threadIdx.x / TSDF_BX);
        if (i >= g.nx || j >= g.ny) continue;
        const size_t s = ((size_t)k * g.ny + j) * g.nx + i;
        const float px = g.ox + g.vs * (float)i, py = g.oy + g.vs * (float)j, pz = g.oz + g.vs * (float)k;
        const float2 tw = g.tw[s];
        float T = tw.x, W = tw.y;
        float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
        if (COLOUR) {
            const float* c = g.rgb + s * 3;
            c0 = c[0]; c1 = c[1]; c2 = c[2];
        }
        const bool touched = tsdf_update_sample<COLOUR>(b, n_views, depth_min, depth_max, alpha_min, g.trunc, g.max_weight, px, py, pz, T, W, c0, c1, c2);
        if (touched) {
            g.tw[s] = make_float2(T, W);
            if (COLOUR) {
                float* c = g.rgb + s * 3;
                c[0] = c0; c[1] = c1; c[2] = c2;
            }
        }
    }
}

// ---- extraction -------------------------------------------------------------------------------------------------------------------
// info[s] = the mask of owned edges with a vertex | the cube's triangle count << 8 | the inside bits of the cube's 8 corners << 16
__global__ __launch_bounds__(256) void tsdf_classify_kernel(const TsdfGridDev g, const uint32_t n, uint32_t* __restrict__ info, uint32_t* __restrict__ vcnt,
                                                            uint32_t* __restrict__ tcnt) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    const uint32_t nxy = g.nx * g.ny;
    const int i = (int)(s % g.nx), j = (int)((s / g.nx) % g.ny), k = (int)(s / nxy);
    uint32_t obs = 0, ins = 0;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int x = i + dx, y = j + dy, z = k + dz;
                if (x < 0 || y < 0 || z < 0 || x >= (int)g.nx || y >= (int)g.ny || z >= (int)g.nz) continue;
                const float2 t = g.tw[((size_t)z * g.ny + (size_t)y) * g.nx + (size_t)x];
                obs |= (t.y > 0.0f ? 1u : 0u) << nb_bit(dx, dy, dz);
                ins |= (t.x < 0.0f ? 1u : 0u) << nb_bit(dx, dy, dz);
            }
    const uint32_t word = tsdf_classify_word(obs, ins);
    info[s] = word;
    vcnt[s] = (uint32_t)__popc(word & 0x7Fu);
    tcnt[s] = (word >> 8) & 0xFFu;
}

__global__ __launch_bounds__(256) void tsdf_emit_kernel(const TsdfGridDev g, const uint32_t n, const uint32_t* __restrict__ info, const uint32_t* __restrict__ vinc,
                                                        const uint32_t* __restrict__ tinc, float* __restrict__ vertices, float* __restrict__ colours,
                                                        uint32_t* __restrict__ triangles) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    const uint32_t word = info[s];
    if ((word & 0xFF7Fu) == 0u) return;
    const uint32_t nxy = g.nx * g.ny;
    tsdf_emit_sample(g.ox, g.oy, g.oz, g.vs, s % g.nx, (s / g.nx) % g.ny, s / nxy, (size_t)s, word, g.tw, g.rgb, info, vinc, tinc, vertices, colours, triangles,
                     [&](uint32_t c) { return (size_t)s + (size_t)(c >> 2) * nxy + (size_t)((c >> 1) & 1u) * g.nx + (c & 1u); });
}

// ---- mesh PLY ---------------------------------------------------------------------------------------------------------------------
BH_DEV void put_u32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

__global__ __launch_bounds__(256) void mesh_ply_pack_kernel(const float* __restrict__ vertices, const float* __restrict__ colours, uint32_t n_v,
                                                            const uint32_t* __restrict__ triangles, uint32_t n_t, uint8_t* __restrict__ rows) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t vrow = colours ? 15u : 12u;
    if (r < n_v) {
        uint8_t* p = rows + r * vrow;
#pragma unroll
        for (int c = 0; c < 3; ++c) put_u32(p + 4 * c, __float_as_uint(vertices[r * 3 + c]));
        if (colours) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float x = colours[r * 3 + c];
                const float q = fminf(fmaxf(x == x ? x : 0.0f, 0.0f), 1.0f) * 255.0f;
                p[12 + c] = (uint8_t)rintf(q);   // half to even
            }
        }
    } else if (r - n_v < n_t) {
        const uint64_t f = r - n_v;
        uint8_t* p = rows + (uint64_t)n_v * vrow + f * 13u;
        p[0] = 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) put_u32(p + 1 + 4 * c, triangles[f * 3 + c]);
    }
}

static std::string mesh_ply_header(uint32_t n_v, bool colours, uint32_t n_t) {
    std::string h = "ply\nformat binary_little_endian 1.0\ncomment Exported from Brush\nelement vertex " + std::to_string(n_v) +
                    "\nproperty float x\nproperty float y\nproperty float z\n";
    if (colours) h += "property uchar red\nproperty uchar green\nproperty uchar blue\n";
    h += "element face " + std::to_string(n_t) + "\nproperty list uchar uint vertex_indices\nend_header\n";
    return h;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static int tsdf_check_grid(bh_ctx* ctx, const BhTsdfGrid* g, const char* who, TsdfGridDev* dev, uint32_t* n) {
    const std::string w(who);
    if (!g || !g->tw) return set_error(ctx, BH_ERR_INVALID_ARG, w + ": null grid");
    if (g->nx < 2u || g->ny < 2u || g->nz < 2u) return set_error(ctx, BH_ERR_INVALID_ARG, w + ": every dimension of the grid must be at least 2");
    if ((uint64_t)g->nx * g->ny > 0x7FFFFFFFull || (uint64_t)g->nx * g->ny * g->nz > 0x7FFFFFFFull)
        return set_error(ctx, BH_ERR_INVALID_ARG, w + ": more than 2^31 - 1 samples");
    if (!(std::isfinite(g->voxel_size) && g->voxel_size > 0.0f)) return set_error(ctx, BH_ERR_INVALID_ARG, w + ": voxel_size must be a finite number > 0");
    if (!(std::isfinite(g->trunc) && g->trunc > 0.0f)) return set_error(ctx, BH_ERR_INVALID_ARG, w + ": trunc must be a finite number > 0");
    if (!(g->max_weight >= 1.0f)) return set_error(ctx, BH_ERR_INVALID_ARG, w + ": max_weight must be at least 1");
    *dev = TsdfGridDev{g->origin[0], g->origin[1], g->origin[2], g->voxel_size, g->nx, g->ny, g->nz, g->trunc, g->max_weight,
                       reinterpret_cast<float2*>(g->tw), g->rgb};
    *n = g->nx * g->ny * g->nz;
    return 0;
}

// classify + the two scans; the counts are read back (blocking)
static int tsdf_classify_and_scan(bh_ctx* ctx, const TsdfGridDev& g, uint32_t n, uint32_t** info, uint32_t** vinc, uint32_t** tinc, uint32_t counts[2]) {
    auto* scratch = (uint32_t*)ensure(ctx, SLOT_TSDF, (size_t)n * 12);
    if (!scratch) return BH_ERR_OOM;
    *info = scratch; *vinc = scratch + n; *tinc = scratch + 2 * (size_t)n;
    const dim3 grid((n + 255u) / 256u), block(256);
    {
        ProfScope ps(ctx, "TsdfClassify");
        hipLaunchKernelGGL(tsdf_classify_kernel, grid, block, 0, ctx->stream, g, n, *info, *vinc, *tinc);
        BH_LAUNCH_CHECK(ctx, "tsdf_classify_kernel");
    }
    {
        ProfScope ps(ctx, "TsdfScan");
        BH_TRY(prefix_sum(ctx, *vinc, nullptr, n, *vinc, /*exclusive=*/false));
        BH_TRY(prefix_sum(ctx, *tinc, nullptr, n, *tinc, /*exclusive=*/false));
    }
    BH_HIP(ctx, hipMemcpyAsync(&counts[0], *vinc + (n - 1u), 4, hipMemcpyDeviceToHost, ctx->stream));
    BH_HIP(ctx, hipMemcpyAsync(&counts[1], *tinc + (n - 1u), 4, hipMemcpyDeviceToHost, ctx->stream));
    BH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // namespace bh

using namespace bh;

extern "C" {

int bh_tsdf_clear(bh_ctx* ctx, const BhTsdfGrid* grid) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    TsdfGridDev g;
    uint32_t n = 0;
    BH_TRY(tsdf_check_grid(ctx, grid, "tsdf_clear", &g, &n));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(tsdf_clear_kernel, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, g, n);
    BH_LAUNCH_CHECK(ctx, "tsdf_clear_kernel");
    return 0;
}

int bh_tsdf_integrate(bh_ctx* ctx, const BhTsdfGrid* grid, uint32_t n_views, const BhCamera* cams, const float* const* depths, const float* const* images,
                      const BhTsdfIntegrateConfig* cfg) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    TsdfGridDev g;
    uint32_t n = 0;
    BH_TRY(tsdf_check_grid(ctx, grid, "tsdf_integrate", &g, &n));
    if (!cfg) return set_error(ctx, BH_ERR_INVALID_ARG, "tsdf_integrate: null config");
    if (n_views == 0) return 0;
    BH_TRY(tsdf_check_views(ctx, "tsdf_integrate", n_views, cams, depths, images));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    ProfScope ps(ctx, "TsdfIntegrate");
    const uint32_t blocks_x = (g.nx + TSDF_BX - 1) / TSDF_BX, blocks_y = (g.ny + TSDF_BY - 1) / TSDF_BY;
    const uint32_t n_blocks = blocks_x * blocks_y * g.nz;   // <= nx ny nz
    const dim3 launch(n_blocks < TSDF_MAX_BLOCKS ? n_blocks : TSDF_MAX_BLOCKS), block(TSDF_WG);
    const bool colour = images && g.rgb;
    for (uint32_t first = 0; first < n_views; first += BH_TSDF_MAX_BATCH) {
        const uint32_t count = n_views - first < BH_TSDF_MAX_BATCH ? n_views - first : BH_TSDF_MAX_BATCH;
        const TsdfBatch b = tsdf_make_batch(first, count, cams, depths, images);
        if (colour)
            hipLaunchKernelGGL(tsdf_integrate_kernel<true>, launch, block, 0, ctx->stream, g, b, count, cfg->depth_min, cfg->depth_max, cfg->alpha_min, blocks_x,
                               blocks_y, n_blocks);
        else
            hipLaunchKernelGGL(tsdf_integrate_kernel<false>, launch, block, 0, ctx->stream, g, b, count, cfg->depth_min, cfg->depth_max, cfg->alpha_min, blocks_x,
                               blocks_y, n_blocks);
        BH_LAUNCH_CHECK(ctx, "tsdf_integrate_kernel");
    }
    return 0;
}

int bh_tsdf_extract_count(bh_ctx* ctx, const BhTsdfGrid* grid, uint32_t* n_vertices, uint32_t* n_triangles) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    TsdfGridDev g;
    uint32_t n = 0;
    BH_TRY(tsdf_check_grid(ctx, grid, "tsdf_extract_count", &g, &n));
    if (!n_vertices || !n_triangles) return set_error(ctx, BH_ERR_INVALID_ARG, "tsdf_extract_count: null count pointer");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t *info, *vinc, *tinc, counts[2] = {0, 0};
    BH_TRY(tsdf_classify_and_scan(ctx, g, n, &info, &vinc, &tinc, counts));
    *n_vertices = counts[0];
    *n_triangles = counts[1];
    return 0;
}

int bh_tsdf_extract(bh_ctx* ctx, const BhTsdfGrid* grid, float* vertices, float* colours, uint32_t* triangles, uint32_t cap_v, uint32_t cap_t,
                    uint32_t* n_vertices, uint32_t* n_triangles) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    TsdfGridDev g;
    uint32_t n = 0;
    BH_TRY(tsdf_check_grid(ctx, grid, "tsdf_extract", &g, &n));
    if (!n_vertices || !n_triangles) return set_error(ctx, BH_ERR_INVALID_ARG, "tsdf_extract: null count pointer");
    if (colours && !g.rgb) return set_error(ctx, BH_ERR_INVALID_ARG, "tsdf_extract: colours of a volume without rgb");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t *info, *vinc, *tinc, counts[2] = {0, 0};
    BH_TRY(tsdf_classify_and_scan(ctx, g, n, &info, &vinc, &tinc, counts));
    *n_vertices = counts[0];
    *n_triangles = counts[1];
    if (counts[0] > cap_v || counts[1] > cap_t) return set_error(ctx, BH_ERR_INVALID_ARG, "tsdf_extract: output capacity too small");
    if ((counts[0] && !vertices) || (counts[1] && !triangles)) return set_error(ctx, BH_ERR_INVALID_ARG, "tsdf_extract: null output");
    if (counts[0] == 0u) return 0;   // (no vertex, hence no triangle)
    {
        ProfScope ps(ctx, "TsdfEmit");
        hipLaunchKernelGGL(tsdf_emit_kernel, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, g, n, info, vinc, tinc, vertices, colours, triangles);
        BH_LAUNCH_CHECK(ctx, "tsdf_emit_kernel");
    }
    BH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int bh_mesh_to_ply(bh_ctx* ctx, const float* vertices, const float* colours, uint32_t n_v, const uint32_t* triangles, uint32_t n_t, void* out, uint64_t cap,
                   uint64_t* written) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!written) return set_error(ctx, BH_ERR_INVALID_ARG, "mesh_to_ply: null size pointer");
    const std::string header = mesh_ply_header(n_v, colours != nullptr, n_t);
    const uint64_t body = (uint64_t)n_v * (colours ? 15u : 12u) + (uint64_t)n_t * 13u;
    *written = header.size() + body;
    if (!out) return 0;   // size query
    if (cap < *written) return set_error(ctx, BH_ERR_INVALID_ARG, "mesh_to_ply: output buffer too small");
    if ((n_v && !vertices) || (n_t && !triangles)) return set_error(ctx, BH_ERR_INVALID_ARG, "mesh_to_ply: null mesh array");
    std::memcpy(out, header.data(), header.size());
    if (body == 0) return 0;
    BH_HIP(ctx, hipSetDevice(ctx->device));
    auto* rows = (uint8_t*)ensure(ctx, SLOT_PLY_ROWS, body);
    if (!rows) return BH_ERR_OOM;
    const uint64_t threads = (uint64_t)n_v + n_t;
    hipLaunchKernelGGL(mesh_ply_pack_kernel, dim3((unsigned)((threads + 255u) / 256u)), dim3(256), 0, ctx->stream, vertices, colours, n_v, triangles, n_t, rows);
    BH_LAUNCH_CHECK(ctx, "mesh_ply_pack_kernel");
    BH_HIP(ctx, hipMemcpyAsync((char*)out + header.size(), rows, body, hipMemcpyDeviceToHost, ctx->stream));
    BH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"
