// device_tsdf.h — what the dense volume (tsdf.hip, include/brush_hip_mesh.h) and the sparse one (sparse_tsdf.hip,
// include/brush_hip_sparse_mesh.h) share, ONE copy each.  On the device: the clear kernel, the views a launch takes from its kernel
// arguments, the per-sample fusion rule and the load / fuse / store around it, the edge order and the tetrahedron case table of the
// extraction, the classification of a sample from the 3x3x3 bits around it and the store of its word, and the emission of a sample's
// vertices and triangles.  On the host: the refusals of a volume's fields and of a dense grid's size, the integrate driver (refusals,
// the batch loop, the choice of instantiation) and the extraction driver (refusals, classify, the two scans, the readback, emit).
// A volume keeps what is its own: its struct, where a sample and its neighbours live, and hence its kernels' index arithmetic.
#pragma once
#include <cmath>
#include <cstring>
#include <string>

#include "context.h"
#include "device_math.h"

namespace bh {

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

// Steps 2-8 of brush_hip_mesh.h for the sample at (px, py, pz), over the batch's views in order; true if a view touched it.
// COLOUR: the volume has rgb and the batch has images (then every view has one)
template <bool COLOUR>
BH_DEV bool tsdf_update_sample(const TsdfBatch& b, const uint32_t n_views, const float depth_min, const float depth_max, const float alpha_min, const float trunc,
                               const float max_weight, const float px, const float py, const float pz, float& T, float& W, float& c0, float& c1, float& c2) {
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
        if (sdf < -trunc) continue;
        const float sd = fminf(1.0f, sdf / trunc);
        const float Wn = W + 1.0f;
        T = (W * T + sd) / Wn;
        if (COLOUR) {
            c0 = (W * c0 + px4.x) / Wn;
            c1 = (W * c1 + px4.y) / Wn;
            c2 = (W * c2 + px4.z) / Wn;
        }
        W = fminf(Wn, max_weight);
        touched = true;
    }
    return touched;
}

// The sample stored at s, at (px, py, pz): loaded, fused with the batch's views, stored if a view touched it.
template <bool COLOUR>
BH_DEV void tsdf_fuse_at(float2* tw, float* rgb, const size_t s, const float px, const float py, const float pz, const TsdfBatch& b, const uint32_t n_views,
                         const float depth_min, const float depth_max, const float alpha_min, const float trunc, const float max_weight) {
    const float2 t = tw[s];
    float T = t.x, W = t.y;
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    if (COLOUR) {
        const float* c = rgb + s * 3;
        c0 = c[0]; c1 = c[1]; c2 = c[2];
    }
    if (tsdf_update_sample<COLOUR>(b, n_views, depth_min, depth_max, alpha_min, trunc, max_weight, px, py, pz, T, W, c0, c1, c2)) {
        tw[s] = make_float2(T, W);
        if (COLOUR) {
            float* c = rgb + s * 3;
            c[0] = c0; c[1] = c1; c[2] = c2;
        }
    }
}

// T = 1, W = 0, rgb = 0 in n samples (static: both units launch it)
static __global__ __launch_bounds__(256) void tsdf_clear_samples_kernel(float2* tw, float* rgb, const uint32_t n) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    tw[s] = make_float2(1.0f, 0.0f);
    if (rgb) {
        float* c = rgb + (size_t)s * 3;
        c[0] = 0.0f; c[1] = 0.0f; c[2] = 0.0f;
    }
}

inline int tsdf_clear_samples(bh_ctx* ctx, float2* tw, float* rgb, uint32_t n) {
    hipLaunchKernelGGL(tsdf_clear_samples_kernel, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, tw, rgb, n);
    BH_LAUNCH_CHECK(ctx, "tsdf_clear_samples_kernel");
    return 0;
}

// What every entry point refuses about a volume's fields, dense or sparse.
inline int tsdf_check_fields(bh_ctx* ctx, const std::string& who, uint32_t nx, uint32_t ny, uint32_t nz, float voxel_size, float trunc, float max_weight) {
    if (nx < 2u || ny < 2u || nz < 2u) return set_error(ctx, BH_ERR_INVALID_ARG, who + ": every dimension of the grid must be at least 2");
    if (!(std::isfinite(voxel_size) && voxel_size > 0.0f)) return set_error(ctx, BH_ERR_INVALID_ARG, who + ": voxel_size must be a finite number > 0");
    if (!(std::isfinite(trunc) && trunc > 0.0f)) return set_error(ctx, BH_ERR_INVALID_ARG, who + ": trunc must be a finite number > 0");
    if (!(max_weight >= 1.0f)) return set_error(ctx, BH_ERR_INVALID_ARG, who + ": max_weight must be at least 1");
    return 0;
}

// The size a dense grid may have; `what` is "" for a volume of its own and "dense " for the target of bh_sptsdf_to_dense.
inline int tsdf_check_dense_dims(bh_ctx* ctx, const std::string& who, const std::string& what, uint32_t nx, uint32_t ny, uint32_t nz) {
    if (nx < 2u || ny < 2u || nz < 2u) return set_error(ctx, BH_ERR_INVALID_ARG, who + ": every dimension of the " + what + "grid must be at least 2");
    if ((uint64_t)nx * ny > 0x7FFFFFFFull || (uint64_t)nx * ny * nz > 0x7FFFFFFFull)
        return set_error(ctx, BH_ERR_INVALID_ARG, who + ": more than 2^31 - 1 " + what + "samples");
    return 0;
}

// What both integrate entry points refuse about their views, before the device is touched.
inline int tsdf_check_views(bh_ctx* ctx, const std::string& who, uint32_t n_views, const BhCamera* cams, const float* const* depths, const float* const* images) {
    if (!cams || !depths) return set_error(ctx, BH_ERR_INVALID_ARG, who + ": null argument");
    for (uint32_t v = 0; v < n_views; ++v) {
        const BhCamera& c = cams[v];
        if (c.model != BH_CAMERA_PINHOLE) return set_error(ctx, BH_ERR_INVALID_ARG, who + ": pinhole cameras only");
        if (c.tile_row_begin != 0u || c.tile_row_end != 0u) return set_error(ctx, BH_ERR_INVALID_ARG, who + ": a camera with a tile-row window");
        if (c.img_w == 0u || c.img_h == 0u || (uint64_t)c.img_w * c.img_h > 0x7FFFFFFFull)
            return set_error(ctx, BH_ERR_INVALID_ARG, who + ": an image side of 0 or more than 2^31 - 1 pixels");
        if (!depths[v] || (images && !images[v])) return set_error(ctx, BH_ERR_INVALID_ARG, who + ": null depth map or image");
    }
    return 0;
}

inline TsdfBatch tsdf_make_batch(uint32_t first, uint32_t count, const BhCamera* cams, const float* const* depths, const float* const* images) {
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
    return b;
}

// The tail of both integrate entry points, after the volume's own check: the refusals, then one launch per batch of views.
// launch(colour, batch, count) enqueues the volume's kernel, tsdf_..._kernel<colour>; `who` + "_kernel" names it in a launch error.
template <class Launch>
inline int tsdf_integrate_batches(bh_ctx* ctx, const char* who, const char* prof, uint32_t n_views, const BhCamera* cams, const float* const* depths,
                                  const float* const* images, const BhTsdfIntegrateConfig* cfg, bool has_rgb, Launch launch) {
    const std::string w(who);
    if (!cfg) return set_error(ctx, BH_ERR_INVALID_ARG, w + ": null config");
    if (n_views == 0) return 0;
    BH_TRY(tsdf_check_views(ctx, w, n_views, cams, depths, images));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    ProfScope ps(ctx, prof);
    const bool colour = images && has_rgb;
    for (uint32_t first = 0; first < n_views; first += BH_TSDF_MAX_BATCH) {
        const uint32_t count = n_views - first < BH_TSDF_MAX_BATCH ? n_views - first : BH_TSDF_MAX_BATCH;
        launch(colour, tsdf_make_batch(first, count, cams, depths, images), count);
        BH_LAUNCH_CHECK(ctx, (w + "_kernel").c_str());
    }
    return 0;
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

// From the observed (W > 0) and inside (T < 0) bits of the 3x3x3 samples around one (nb_bit; a sample that does not exist has neither):
// the mask of owned edges with a vertex | the cube's triangle count << 8 | the inside bits of the cube's 8 corners << 16
BH_DEV uint32_t tsdf_classify_word(const uint32_t obs, const uint32_t ins) {
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
    return mask | tris << 8 | corners8 << 16;
}

BH_DEV void tsdf_store_class(uint32_t* __restrict__ info, uint32_t* __restrict__ vcnt, uint32_t* __restrict__ tcnt, const size_t s, const uint32_t word) {
    info[s] = word;
    vcnt[s] = (uint32_t)__popc(word & 0x7Fu);
    tcnt[s] = (word >> 8) & 0xFFu;
}

BH_DEV uint32_t tsdf_vertex_index(const uint32_t* __restrict__ info, const uint32_t* __restrict__ vinc, size_t owner, uint32_t d) {
    const uint32_t m = info[owner] & 0x7Fu;
    return vinc[owner] - (uint32_t)__popc(m) + (uint32_t)__popc(m & ((1u << d) - 1u));
}

// The vertices and triangles of the sample (i, j, k) stored at s, whose info word (non-zero) is `word`.  at(code) is where the sample
// (i, j, k) + (code & 1, code >> 1 & 1, code >> 2) is stored: the index into tw, rgb / 3, info and the two scans alike.
template <class At>
BH_DEV void tsdf_emit_sample(const float ox, const float oy, const float oz, const float vs, const uint32_t i, const uint32_t j, const uint32_t k, const size_t s,
                             const uint32_t word, const float2* __restrict__ tw, const float* __restrict__ rgb, const uint32_t* __restrict__ info,
                             const uint32_t* __restrict__ vinc, const uint32_t* __restrict__ tinc, float* __restrict__ vertices, float* __restrict__ colours,
                             uint32_t* __restrict__ triangles, At at) {
    const uint32_t mask = word & 0x7Fu, tris = (word >> 8) & 0xFFu, corners8 = word >> 16;
    if (mask) {
        const float ax = ox + vs * (float)i, ay = oy + vs * (float)j, az = oz + vs * (float)k;
        const float Ta = tw[s].x;
        size_t out = (size_t)(vinc[s] - (uint32_t)__popc(mask)) * 3;
        for (uint32_t e = 0; e < 7u; ++e) {
            if (!((mask >> e) & 1u)) continue;
            const uint32_t code = TSDF_D_CODE[e];
            const uint32_t dx = code & 1u, dy = (code >> 1) & 1u, dz = code >> 2;
            const size_t sb = at(code);
            const float Tb = tw[sb].x;
            const float t = Ta / (Ta - Tb);
            const float bx = ox + vs * (float)(i + dx), by = oy + vs * (float)(j + dy), bz = oz + vs * (float)(k + dz);
            vertices[out] = ax + t * (bx - ax);
            vertices[out + 1] = ay + t * (by - ay);
            vertices[out + 2] = az + t * (bz - az);
            if (colours) {
                const float* ca = rgb + (size_t)s * 3;
                const float* cb = rgb + sb * 3;
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
                    idx[c] = tsdf_vertex_index(info, vinc, at(ca), TSDF_D_INDEX[ca ^ cb]);
                }
                triangles[out] = idx[0];
                triangles[out + 1] = flip ? idx[2] : idx[1];
                triangles[out + 2] = flip ? idx[1] : idx[2];
                out += 3;
            }
        }
    }
}

// All four extraction entry points, after the volume's own check, over its n stored samples: the refusals, classify into the scratch
// slot, the two inclusive scans, the counts read back (blocking) and, unless count_only, emit.  classify(info, vcnt, tcnt) and
// emit(info, vinc, tinc) enqueue the volume's kernels and return their launch check; prof names the stages Classify, Scan, Emit.
template <class Classify, class Emit>
inline int tsdf_extract_run(bh_ctx* ctx, const char* who, Slot slot, uint32_t n, bool has_rgb, Classify classify, Emit emit, const float* vertices, const float* colours,
                            const uint32_t* triangles, uint32_t cap_v, uint32_t cap_t, uint32_t* n_vertices, uint32_t* n_triangles, bool count_only,
                            const char* const prof[3]) {
    const std::string w(who);
    if (!n_vertices || !n_triangles) return set_error(ctx, BH_ERR_INVALID_ARG, w + ": null count pointer");
    if (colours && !has_rgb) return set_error(ctx, BH_ERR_INVALID_ARG, w + ": colours of a volume without rgb");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    auto* info = (uint32_t*)ensure(ctx, slot, (size_t)n * 12);
    if (!info) return BH_ERR_OOM;
    uint32_t *vinc = info + n, *tinc = info + 2 * (size_t)n, counts[2] = {0, 0};
    {
        ProfScope ps(ctx, prof[0]);
        BH_TRY(classify(info, vinc, tinc));
    }
    {
        ProfScope ps(ctx, prof[1]);
        BH_TRY(prefix_sum(ctx, vinc, nullptr, n, vinc, /*exclusive=*/false));
        BH_TRY(prefix_sum(ctx, tinc, nullptr, n, tinc, /*exclusive=*/false));
    }
    BH_HIP(ctx, hipMemcpyAsync(&counts[0], vinc + (n - 1u), 4, hipMemcpyDeviceToHost, ctx->stream));
    BH_HIP(ctx, hipMemcpyAsync(&counts[1], tinc + (n - 1u), 4, hipMemcpyDeviceToHost, ctx->stream));
    BH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_vertices = counts[0];
    *n_triangles = counts[1];
    if (count_only) return 0;
    if (counts[0] > cap_v || counts[1] > cap_t) return set_error(ctx, BH_ERR_INVALID_ARG, w + ": output capacity too small");
    if ((counts[0] && !vertices) || (counts[1] && !triangles)) return set_error(ctx, BH_ERR_INVALID_ARG, w + ": null output");
    if (counts[0] == 0u) return 0;   // (no vertex, hence no triangle)
    {
        ProfScope ps(ctx, prof[2]);
        BH_TRY(emit(info, vinc, tinc));
    }
    BH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // namespace bh
