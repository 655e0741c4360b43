// device_tsdf.h — what the dense volume (tsdf.hip, include/brush_hip_mesh.h) and the sparse one (sparse_tsdf.hip,
// include/brush_hip_sparse_mesh.h) share, ONE copy each: the views a launch takes from its kernel arguments, the per-sample fusion
// rule, the edge order and the tetrahedron case table of the extraction, the classification of a sample from the 3x3x3 bits around
// it, and the emission of a sample's vertices and triangles.  The two volumes differ only in where a sample's neighbours live.
#pragma once
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

}  // namespace bh
