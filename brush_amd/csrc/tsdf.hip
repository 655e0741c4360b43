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
//
// Shared with sparse_tsdf.hip through device_tsdf.h: the clear kernel, a sample's load / fuse / store, the classifier and the emitter,
// the field checks, and the host drivers behind integrate and the two extract entry points.  Here: the grid's struct and check, each
// kernel's map from thread to sample, the launch shapes, and the mesh PLY.
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
        tsdf_fuse_at<COLOUR>(g.tw, g.rgb, s, px, py, pz, b, n_views, depth_min, depth_max, alpha_min, g.trunc, g.max_weight);
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
    tsdf_store_class(info, vcnt, tcnt, s, tsdf_classify_word(obs, ins));
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
    BH_TRY(tsdf_check_dense_dims(ctx, w, "", g->nx, g->ny, g->nz));
    BH_TRY(tsdf_check_fields(ctx, w, g->nx, g->ny, g->nz, g->voxel_size, g->trunc, g->max_weight));
    *dev = TsdfGridDev{g->origin[0], g->origin[1], g->origin[2], g->voxel_size, g->nx, g->ny, g->nz, g->trunc, g->max_weight,
                       reinterpret_cast<float2*>(g->tw), g->rgb};
    *n = g->nx * g->ny * g->nz;
    return 0;
}

// bh_tsdf_extract and bh_tsdf_extract_count: the dense volume's two launches for tsdf_extract_run
static int tsdf_extract_grid(bh_ctx* ctx, const BhTsdfGrid* grid, const char* who, float* vertices, float* colours, uint32_t* triangles, uint32_t cap_v, uint32_t cap_t,
                             uint32_t* n_vertices, uint32_t* n_triangles, bool count_only) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    TsdfGridDev g;
    uint32_t n = 0;
    BH_TRY(tsdf_check_grid(ctx, grid, who, &g, &n));
    const dim3 launch((n + 255u) / 256u), block(256);
    static const char* const prof[3] = {"TsdfClassify", "TsdfScan", "TsdfEmit"};
    return tsdf_extract_run(
        ctx, who, SLOT_TSDF, n, g.rgb != nullptr,
        [&](uint32_t* info, uint32_t* vcnt, uint32_t* tcnt) {
            hipLaunchKernelGGL(tsdf_classify_kernel, launch, block, 0, ctx->stream, g, n, info, vcnt, tcnt);
            BH_LAUNCH_CHECK(ctx, "tsdf_classify_kernel");
            return 0;
        },
        [&](const uint32_t* info, const uint32_t* vinc, const uint32_t* tinc) {
            hipLaunchKernelGGL(tsdf_emit_kernel, launch, block, 0, ctx->stream, g, n, info, vinc, tinc, vertices, colours, triangles);
            BH_LAUNCH_CHECK(ctx, "tsdf_emit_kernel");
            return 0;
        },
        vertices, colours, triangles, cap_v, cap_t, n_vertices, n_triangles, count_only, prof);
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
    return tsdf_clear_samples(ctx, g.tw, g.rgb, n);
}

int bh_tsdf_integrate(bh_ctx* ctx, const BhTsdfGrid* grid, uint32_t n_views, const BhCamera* cams, const float* const* depths, const float* const* images,
                      const BhTsdfIntegrateConfig* cfg) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    TsdfGridDev g;
    uint32_t n = 0;
    BH_TRY(tsdf_check_grid(ctx, grid, "tsdf_integrate", &g, &n));
    const uint32_t blocks_x = (g.nx + TSDF_BX - 1) / TSDF_BX, blocks_y = (g.ny + TSDF_BY - 1) / TSDF_BY;
    const uint32_t n_blocks = blocks_x * blocks_y * g.nz;   // <= nx ny nz
    const dim3 launch(n_blocks < TSDF_MAX_BLOCKS ? n_blocks : TSDF_MAX_BLOCKS), block(TSDF_WG);
    return tsdf_integrate_batches(ctx, "tsdf_integrate", "TsdfIntegrate", n_views, cams, depths, images, cfg, g.rgb != nullptr,
                                  [&](bool colour, const TsdfBatch& b, uint32_t count) {
                                      hipLaunchKernelGGL(colour ? tsdf_integrate_kernel<true> : tsdf_integrate_kernel<false>, launch, block, 0, ctx->stream, g, b, count,
                                                         cfg->depth_min, cfg->depth_max, cfg->alpha_min, blocks_x, blocks_y, n_blocks);
                                  });
}

int bh_tsdf_extract_count(bh_ctx* ctx, const BhTsdfGrid* grid, uint32_t* n_vertices, uint32_t* n_triangles) {
    return tsdf_extract_grid(ctx, grid, "tsdf_extract_count", nullptr, nullptr, nullptr, 0, 0, n_vertices, n_triangles, /*count_only=*/true);
}

int bh_tsdf_extract(bh_ctx* ctx, const BhTsdfGrid* grid, float* vertices, float* colours, uint32_t* triangles, uint32_t cap_v, uint32_t cap_t,
                    uint32_t* n_vertices, uint32_t* n_triangles) {
    return tsdf_extract_grid(ctx, grid, "tsdf_extract", vertices, colours, triangles, cap_v, cap_t, n_vertices, n_triangles, /*count_only=*/false);
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
