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

namespace bh {

struct TsdfGridDev {
    float ox, oy, oz, vs;
    uint32_t nx, ny, nz;
    float trunc, max_weight;
    float2* tw;
    float* rgb;
};

struct TsdfView {
    float vm[12];
    float fx, fy, cx, cy;
    float wf, hf;   // (float)W, (float)H
    uint32_t w, pad;
    const float* depth;
    const float* image;   // [H,W,4] or NULL
};

struct TsdfBatch {
    TsdfView v[BH_TSDF_MAX_BATCH];
};
static_assert(sizeof(TsdfBatch) == 96 * BH_TSDF_MAX_BATCH, "TsdfBatch is passed by value: keep it well inside the kernel-argument segment");

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
        bool touched = false;
        for (uint32_t v = 0; v < n_views; ++v) {
            const TsdfView& cam = b.v[v];
            const float Z = ((cam.vm[2] * px + cam.vm[5] * py) + cam.vm[8] * pz) + cam.vm[11];
            if (!(Z > depth_min)) continue;
            // (one axis at a time: a sample outside in x never pays for the second division; a NaN fails every comparison)
            const float X = ((cam.vm[0] * px + cam.vm[3] * py) + cam.vm[6] * pz) + cam.vm[9];
            const float u = cam.fx * (X / Z) + cam.cx;
            if (!(u >= 0.0f && u < cam.wf)) continue;
            const float Y = ((cam.vm[1] * px + cam.vm[4] * py) + cam.vm[7] * pz) + cam.vm[10];
            const float vv = cam.fy * (Y / Z) + cam.cy;
            if (!(vv >= 0.0f && vv < cam.hf)) continue;
            const size_t pix = (size_t)(uint32_t)vv * cam.w + (uint32_t)u;         // 0 <= u < W: truncation is floor
            const float d = cam.depth[pix];
            if (!(is_finite_f32(d) && d > 0.0f && d <= depth_max)) continue;
            float4 px4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (cam.image) {
                px4 = reinterpret_cast<const float4*>(cam.image)[pix];
                if (px4.w < alpha_min) continue;
            }
            const float sdf = d - Z;
            if (sdf < -g.trunc) continue;
            const float sd = fminf(1.0f, sdf / g.trunc);
            const float Wn = W + 1.0f;
            T = (W * T + sd) / Wn;
            if (COLOUR) {
                c0 = (W * c0 + px4.x) / Wn;
                c1 = (W * c1 + px4.y) / Wn;
                c2 = (W * c2 + px4.z) / Wn;
            }
            W = fminf(Wn, g.max_weight);
            touched = true;
        }
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
// the 3x3x3 neighbourhood of a sample as 27 bits
constexpr uint32_t nb_bit(int dx, int dy, int dz) { return (uint32_t)((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)); }
// the 8 corners of the cube with min corner p - a
constexpr uint32_t cube_mask(int ax, int ay, int az) {
    uint32_t m = 0;
    for (int bz = 0; bz < 2; ++bz)
        for (int by = 0; by < 2; ++by)
            for (int bx = 0; bx < 2; ++bx) m |= 1u << nb_bit(bx - ax, by - ay, bz - az);
    return m;
}
// an edge's direction as a code x | y << 1 | z << 2, in the header's order of d; and the inverse map
__constant__ const uint8_t TSDF_D_CODE[7] = {1, 2, 4, 3, 5, 6, 7};
__constant__ const uint8_t TSDF_D_INDEX[8] = {0, 0, 1, 3, 2, 4, 5, 6};
// the vertices of tetrahedron t (permutations xyz xzy yxz yzx zxy zyx) as corner codes, 4 bits each from v0 up
__constant__ const uint16_t TSDF_TET[6] = {0x7310, 0x7510, 0x7320, 0x7620, 0x7540, 0x7640};
constexpr uint32_t TSDF_NEGATIVE = 0x26;   // bit t: tetrahedron t is negatively oriented (xzy, yxz, zyx)
// triangles per inside mask, 2 bits each: {0,1,1,2, 1,2,2,1, 1,2,2,1, 2,1,1,0}
constexpr uint32_t TSDF_NTRI = 0x16696994u;
// the header's case table: edge numbers, 3 bits each, first triple in the low 9 bits
#define TSDF_TRI(a, b, c) ((a) | (b) << 3 | (c) << 6)
__constant__ const uint32_t TSDF_CASE[16] = {
    0,
    TSDF_TRI(0, 1, 2),
    TSDF_TRI(0, 4, 3),
    TSDF_TRI(1, 2, 4) | TSDF_TRI(1, 4, 3) << 9,
    TSDF_TRI(5, 1, 3),
    TSDF_TRI(0, 3, 5) | TSDF_TRI(0, 5, 2) << 9,
    TSDF_TRI(0, 4, 5) | TSDF_TRI(0, 5, 1) << 9,
    TSDF_TRI(5, 2, 4),
    TSDF_TRI(5, 4, 2),
    TSDF_TRI(0, 1, 5) | TSDF_TRI(0, 5, 4) << 9,
    TSDF_TRI(0, 2, 5) | TSDF_TRI(0, 5, 3) << 9,
    TSDF_TRI(5, 3, 1),
    TSDF_TRI(1, 3, 4) | TSDF_TRI(1, 4, 2) << 9,
    TSDF_TRI(0, 3, 4),
    TSDF_TRI(0, 2, 1),
    0,
};
#undef TSDF_TRI
// the ends of tetrahedron edge e (v0v1 v0v2 v0v3 v1v2 v1v3 v2v3), 2 bits each
constexpr uint32_t TSDF_EDGE_A = 0x940, TSDF_EDGE_B = 0xFB9;

BH_DEV uint32_t tet_inside_mask(uint32_t tet, uint32_t corners8) {
    return ((corners8 >> (tet & 15u)) & 1u) | ((corners8 >> ((tet >> 4) & 15u)) & 1u) << 1 | ((corners8 >> ((tet >> 8) & 15u)) & 1u) << 2 |
           ((corners8 >> (tet >> 12)) & 1u) << 3;
}

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
    const uint32_t centre = (ins >> nb_bit(0, 0, 0)) & 1u;
    uint32_t mask = 0;
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        constexpr int codes[7] = {1, 2, 4, 3, 5, 6, 7};
        const int dx = codes[e] & 1, dy = (codes[e] >> 1) & 1, dz = codes[e] >> 2;
        bool has = false;
#pragma unroll
        for (int az = 0; az <= 1 - dz; ++az)
#pragma unroll
            for (int ay = 0; ay <= 1 - dy; ++ay)
#pragma unroll
                for (int ax = 0; ax <= 1 - dx; ++ax) {
                    const uint32_t cm = cube_mask(ax, ay, az);
                    has = has || (obs & cm) == cm;
                }
        const uint32_t other = (ins >> nb_bit(dx, dy, dz)) & 1u;
        if (has && other != centre) mask |= 1u << e;
    }
    uint32_t tris = 0, corners8 = 0;
    constexpr uint32_t own = cube_mask(0, 0, 0);
    if ((obs & own) == own) {
#pragma unroll
        for (int c = 0; c < 8; ++c) corners8 |= ((ins >> nb_bit(c & 1, (c >> 1) & 1, c >> 2)) & 1u) << c;
#pragma unroll
        for (int t = 0; t < 6; ++t) tris += (TSDF_NTRI >> (2u * tet_inside_mask(TSDF_TET[t], corners8))) & 3u;
    }
    info[s] = mask | tris << 8 | corners8 << 16;
    vcnt[s] = (uint32_t)__popc(mask);
    tcnt[s] = tris;
}

BH_DEV uint32_t tsdf_vertex_index(const uint32_t* __restrict__ info, const uint32_t* __restrict__ vinc, size_t owner, uint32_t d) {
    const uint32_t m = info[owner] & 0x7Fu;
    return vinc[owner] - (uint32_t)__popc(m) + (uint32_t)__popc(m & ((1u << d) - 1u));
}

__global__ __launch_bounds__(256) void tsdf_emit_kernel(const TsdfGridDev g, const uint32_t n, const uint32_t* __restrict__ info, const uint32_t* __restrict__ vinc,
                                                        const uint32_t* __restrict__ tinc, float* __restrict__ vertices, float* __restrict__ colours,
                                                        uint32_t* __restrict__ triangles) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    const uint32_t word = info[s];
    const uint32_t mask = word & 0x7Fu, tris = (word >> 8) & 0xFFu, corners8 = word >> 16;
    if ((mask | tris) == 0u) return;
    const uint32_t nxy = g.nx * g.ny;
    if (mask) {
        const uint32_t i = s % g.nx, j = (s / g.nx) % g.ny, k = s / nxy;
        const float ax = g.ox + g.vs * (float)i, ay = g.oy + g.vs * (float)j, az = g.oz + g.vs * (float)k;
        const float Ta = g.tw[s].x;
        size_t out = (size_t)(vinc[s] - (uint32_t)__popc(mask)) * 3;
        for (uint32_t e = 0; e < 7u; ++e) {
            if (!((mask >> e) & 1u)) continue;
            const uint32_t code = TSDF_D_CODE[e];
            const uint32_t dx = code & 1u, dy = (code >> 1) & 1u, dz = code >> 2;
            const size_t sb = (size_t)s + (size_t)dz * nxy + (size_t)dy * g.nx + dx;
            const float Tb = g.tw[sb].x;
            const float t = Ta / (Ta - Tb);
            const float bx = g.ox + g.vs * (float)(i + dx), by = g.oy + g.vs * (float)(j + dy), bz = g.oz + g.vs * (float)(k + dz);
            vertices[out] = ax + t * (bx - ax);
            vertices[out + 1] = ay + t * (by - ay);
            vertices[out + 2] = az + t * (bz - az);
            if (colours) {
                const float* ca = g.rgb + (size_t)s * 3;
                const float* cb = g.rgb + sb * 3;
                colours[out] = ca[0] + t * (cb[0] - ca[0]);
                colours[out + 1] = ca[1] + t * (cb[1] - ca[1]);
                colours[out + 2] = ca[2] + t * (cb[2] - ca[2]);
            }
            out += 3;
        }
    }
    if (tris) {
        size_t out = (size_t)(tinc[s] - tris) * 3;
        for (uint32_t t = 0; t < 6u; ++t) {
            const uint32_t tet = TSDF_TET[t];
            const uint32_t m = tet_inside_mask(tet, corners8);
            const uint32_t count = (TSDF_NTRI >> (2u * m)) & 3u;
            uint32_t cases = TSDF_CASE[m];
            const bool flip = (TSDF_NEGATIVE >> t) & 1u;
            for (uint32_t q = 0; q < count; ++q, cases >>= 9) {
                uint32_t idx[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint32_t e = (cases >> (3 * c)) & 7u;
                    const uint32_t ca = (tet >> (4u * ((TSDF_EDGE_A >> (2u * e)) & 3u))) & 15u;
                    const uint32_t cb = (tet >> (4u * ((TSDF_EDGE_B >> (2u * e)) & 3u))) & 15u;
                    const size_t owner = (size_t)s + (size_t)(ca >> 2) * nxy + (size_t)((ca >> 1) & 1u) * g.nx + (ca & 1u);
                    idx[c] = tsdf_vertex_index(info, vinc, owner, TSDF_D_INDEX[ca ^ cb]);
                }
                triangles[out] = idx[0];
                triangles[out + 1] = flip ? idx[2] : idx[1];
                triangles[out + 2] = flip ? idx[1] : idx[2];
                out += 3;
            }
        }
    }
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
    if (!cams || !depths) return set_error(ctx, BH_ERR_INVALID_ARG, "tsdf_integrate: null argument");
    for (uint32_t v = 0; v < n_views; ++v) {
        const BhCamera& c = cams[v];
        if (c.model != BH_CAMERA_PINHOLE) return set_error(ctx, BH_ERR_INVALID_ARG, "tsdf_integrate: pinhole cameras only");
        if (c.tile_row_begin != 0u || c.tile_row_end != 0u) return set_error(ctx, BH_ERR_INVALID_ARG, "tsdf_integrate: a camera with a tile-row window");
        if (c.img_w == 0u || c.img_h == 0u || (uint64_t)c.img_w * c.img_h > 0x7FFFFFFFull)
            return set_error(ctx, BH_ERR_INVALID_ARG, "tsdf_integrate: an image side of 0 or more than 2^31 - 1 pixels");
        if (!depths[v] || (images && !images[v])) return set_error(ctx, BH_ERR_INVALID_ARG, "tsdf_integrate: null depth map or image");
    }
    BH_HIP(ctx, hipSetDevice(ctx->device));
    ProfScope ps(ctx, "TsdfIntegrate");
    const uint32_t blocks_x = (g.nx + TSDF_BX - 1) / TSDF_BX, blocks_y = (g.ny + TSDF_BY - 1) / TSDF_BY;
    const uint32_t n_blocks = blocks_x * blocks_y * g.nz;   // <= nx ny nz
    const dim3 launch(n_blocks < TSDF_MAX_BLOCKS ? n_blocks : TSDF_MAX_BLOCKS), block(TSDF_WG);
    const bool colour = images && g.rgb;
    for (uint32_t first = 0; first < n_views; first += BH_TSDF_MAX_BATCH) {
        const uint32_t count = n_views - first < BH_TSDF_MAX_BATCH ? n_views - first : BH_TSDF_MAX_BATCH;
        TsdfBatch b{};
        for (uint32_t v = 0; v < count; ++v) {
            const BhCamera& c = cams[first + v];
            TsdfView& t = b.v[v];
            std::memcpy(t.vm, c.vm, sizeof(t.vm));
            t.fx = c.fx; t.fy = c.fy; t.cx = c.cx; t.cy = c.cy;
            t.wf = (float)c.img_w; t.hf = (float)c.img_h;
            t.w = c.img_w;
            t.depth = depths[first + v];
            t.image = images ? images[first + v] : nullptr;
        }
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
