// device_map_blend.h — the one blend skeleton of the attribute maps (depth.hip: depth maps, normal.hip: normal maps,
// distortion.hip: distortion maps, features.hip: feature maps).
//
// A map is one more blend over the lists a BH_FLAG_BWD_INFO forward saved: K16's splats in K16's order with K16's alpha, cut-off,
// clamp and saturation rule (device_blend.h), folding a per-splat attribute where K16 folds its colour.  Everything the maps share
// lives here once: the tile mapping, the near and far ranges, batch staging, the conic arithmetic, the pre-test, the backward's
// replay of the forward ("instruction for instruction": the bit-identity promise rests on it), the RAW sums P Q R2 R3 R4 Vs, the
// register butterfly they leave through and their atomics into the [Nv,10] accumulator K17 fills.  What differs comes from a traits
// struct P of the map's own file:
//
//   STRIDE                       floats per staged splat (a multiple of 4; the first six are always x y c00/2 c01 | c11/2 alpha0)
//   NACC, NV                     per-pixel accumulators of the forward; per-splat V sums of the backward (any count: 1, 3, a chunk of 16)
//   Attr, chunks(attr)           the per-splat input, passed by value (SinglePassMap: a const float*; features: the compact rows and
//                                their channel count), and the grid's y extent: passes over the lists (1; features: chunks of
//                                channels, the chunk of a block being blockIdx.y inside P's own functions)
//   FWD_WAVES, BWD_WAVES         the second __launch_bounds__ argument of the two kernels
//   Rec, load(p)                 the staged record (float4 s0, s1, ...) and its uniform LDS read
//   stage(d, v, cut, attr, cg)   the stage store: v = the six projected floats, cut = blend_sigma_cut
//   cut(r)                       where sigma_cut sits in the record
//   fold(r, ok, sat, alpha_eff, next_t, T, acc)   everything behind blend_step in the forward (median's early finish included)
//   store(out, attr, pix, acc, T)   the epilogue store of one pixel
//   BwdMaps, Pix, prologue(m, pix, px)   the map pointers the backward reads (passed by value), a pixel's cotangent (g[NV] and
//                                whatever else cv needs) and its start: fills px, returns S = the pixel's remaining sum
//   cv(r, px)                    the "colour" of the splat at the pixel
//   vg(r, px, i)                 the factor of V sum i for this splat at this pixel (depth and normal: the pixel's cotangent g[i] alone)
//   v_home(m, v_attr, cg, i)     where V sum i of splat cg is added (SinglePassMap: v_attr + cg * NV + i), or null: nowhere
//
// The butterfly.  The 6 + NV per-splat sums are numbered P Q R2 R3 | R4 Vs V0 V1 | V2 .. and leave four to a register: one
// swap32_add pair, one swap16_add and one row_allreduce per FOUR sums, after which every lane of 16-lane row r of register j holds
// sum 4 j + comp(r), comp = 0 2 1 3 for rows 0..3 (device_blend.h).  Lane j of each row adds its sum to its home: P Q R2 R3 R4 to
// columns 0..4 of v_combined, Vs to column 8, V sum i to P::v_home.
#pragma once
#include <algorithm>

#include "context.h"
#include "device_blend.h"

namespace bh {

constexpr int MAP_BATCH = 64;

struct MapUniforms {
    uint32_t tile_bw, num_tiles, tile_begin, img_w, img_h, band_mode;
};

inline MapUniforms map_uniforms(const bh_ctx* ctx, const ViewUniforms& vu) {
    MapUniforms u;
    u.tile_bw = vu.tile_bw;
    u.num_tiles = vu.tile_bw * (vu.tile_y1 - vu.tile_y0);
    u.tile_begin = vu.tile_bw * vu.tile_y0;
    u.img_w = vu.img_w;
    u.img_h = vu.img_h;
    u.band_mode = ctx->knob_band_mode;
    return u;
}

// a frame that lists nothing: every map is 0 over the rendered window of the [H,W,channels] output
inline int clear_map_window(bh_ctx* ctx, const ViewUniforms& vu, float* out, size_t channels) {
    const size_t row0 = (size_t)vu.tile_y0 * TILE_WIDTH, row1 = std::min<size_t>((size_t)vu.tile_y1 * TILE_WIDTH, vu.img_h);
    if (row1 > row0) BH_HIP(ctx, hipMemsetAsync(out + row0 * vu.img_w * channels, 0, (row1 - row0) * vu.img_w * channels * 4, ctx->stream));
    return 0;
}

// floats of a per-splat vector of a term's backward (v_z: 1 per splat, Vn: 3), padded to a multiple of 64 so that whatever follows it
// in the slot stays 256-byte aligned; never empty
inline size_t splat_vec_floats(uint32_t nv, uint32_t per_splat) { return ((size_t)(nv ? nv : 1u) * per_splat + 63u) & ~(size_t)63u; }

// The one layout of a map's scratch slot: the per-splat input vector [Nv,per_splat] (where the map stages one of its own making) |
// the per-splat V vector [Nv,per_splat] | the frame's accumulated map (map_floats), each vector padded by splat_vec_floats.  A
// forward (backward == false) asks for the input vector alone.
struct MapScratch {
    float* in = nullptr;
    float* v = nullptr;
    float* acc = nullptr;
    size_t vec_floats = 0;
};

inline int map_scratch(bh_ctx* ctx, Slot slot, uint32_t nv, uint32_t per_splat, bool has_input, bool backward, size_t map_floats, MapScratch* s) {
    s->vec_floats = splat_vec_floats(nv, per_splat);
    const size_t in_floats = has_input ? s->vec_floats : 0;
    auto* base = (float*)ensure(ctx, slot, (in_floats + (backward ? s->vec_floats + map_floats : 0)) * 4);
    if (!base) return BH_ERR_OOM;
    s->in = has_input ? base : nullptr;
    s->v = base + in_floats;
    s->acc = s->v + s->vec_floats;   // (16-byte aligned: vec_floats is a multiple of 64)
    return 0;
}

// What the maps with one pass over the lists and a V vector [Nv,NV_] share (depth, normal, distortion)
template <int NV_>
struct SinglePassMap {
    typedef const float* __restrict__ Attr;
    static constexpr int NV = NV_, FWD_WAVES = 8, BWD_WAVES = 6;
    static uint32_t chunks(Attr) { return 1u; }
    template <class M>
    static BH_DEV float* v_home(const M&, float* v_attr, uint32_t cg, int i) { return v_attr + (size_t)cg * NV_ + i; }
};

// The row-marking contract of the scatters behind K18 (depth.hip: v_z -> the mean, normal.hip: Vn -> the quaternion).  In the
// single-GPU train step only the refine-weight vector was cleared; K18 marked the rows it wrote in that vector's sign bits and the
// update reads marked rows only.  K18 skips a splat whose ten sums are all zero, so a row a scatter adds to may hold last step's
// bytes and carry no mark.  Such a row is claimed: stored whole as zeros (the ten transform floats at vt, its sh_floats SH floats,
// its raw opacity) and marked, so that the scatter's accumulate leaves what a zero-filled row would hold, bit for bit.  The mark is
// the sign of a zero: the refine weight itself is not touched.  A marked row (K18's, or an earlier scatter's) is left as it is.
BH_DEV void claim_grad_row(uint32_t gid, uint32_t sh_floats, float* __restrict__ vt, float* __restrict__ v_sh, float* __restrict__ v_raw_opac,
                           float* __restrict__ v_refine) {
    const uint32_t mark = f2u(v_refine[gid]);
    if (mark >> 31) return;
#pragma unroll
    for (int k = 0; k < 10; ++k) vt[k] = 0.0f;
    float* sh = v_sh + (size_t)gid * sh_floats;
    for (uint32_t k = 0; k < sh_floats; ++k) sh[k] = 0.0f;
    v_raw_opac[gid] = 0.0f;
    v_refine[gid] = u2f(mark | 0x80000000u);
}

// lane i stages splat i of the batch; the diagonal of the conic halved as in K16 (bit-identical sigma, rasterize.hip stage_batch)
template <bool SMOOTH, class P>
BH_DEV uint32_t stage_map_batch(const uint32_t* __restrict__ isect_gids, const float* __restrict__ projected, const typename P::Attr attr,
                                uint32_t batch_start, uint32_t cnt, int lane, float* s_splat) {
    uint32_t cg = 0;
    if ((uint32_t)lane < cnt) {
        cg = isect_gids[batch_start + lane];
        const float* p = projected + (size_t)cg * 9;
        float v[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = p[k];
        P::stage(reinterpret_cast<float4*>(s_splat + lane * P::STRIDE), v, blend_sigma_cut<SMOOTH>(v[5]), attr, cg);
    }
    return cg;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
// One wave64 per 16 x 16 tile, four pixels per lane (one per 8 x 8 quadrant) as in K16: wave-synchronous, the quadrant skip is one
// scalar branch, the "every pixel is done" test one ballot.  A finished pixel keeps a negative T (K16's convention: one unsigned
// compare tests "live and inside the cut").
template <bool SMOOTH, class P>
__global__ __launch_bounds__(64, P::FWD_WAVES) void map_forward_kernel(MapUniforms u, const uint32_t* __restrict__ isect_gids,
                                                                       const uint32_t* __restrict__ tile_offsets,
                                                                       const uint32_t* __restrict__ tile_offsets_far, const float* __restrict__ projected,
                                                                       const typename P::Attr attr, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_splat[MAP_BATCH * P::STRIDE];
    const uint32_t local_tile = tile_of_block(blockIdx.x, u.num_tiles, u.band_mode);
    if (local_tile >= u.num_tiles) return;
    const uint32_t tile = u.tile_begin + local_tile;
    const int lane = threadIdx.x;
    const uint32_t px0 = (tile % u.tile_bw) * TILE_WIDTH + (lane & 7), py0 = (tile / u.tile_bw) * TILE_WIDTH + (lane >> 3);
    const float pcx[2] = {(float)px0 + 0.5f, (float)(px0 + 8) + 0.5f};
    const float pcy[2] = {(float)py0 + 0.5f, (float)(py0 + 8) + 0.5f};
    float tr[4], acc[4][P::NACC];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t px = px0 + 8 * (q & 1), py = py0 + 8 * (q >> 1);
        tr[q] = (px < u.img_w && py < u.img_h) ? 1.0f : -1.0f;
#pragma unroll
        for (int i = 0; i < P::NACC; ++i) acc[q][i] = 0.0f;
    }
    auto any_live = [&]() {
        bool l = false;
#pragma unroll
        for (int q = 0; q < 4; ++q) l = l || tr[q] > 0.0f;
        return l;
    };
    uint32_t sign_mask = 0x80000000u;   // kept in a VGPR: an SGPR operand halves a VALU op's issue rate
    asm volatile("" : "+v"(sign_mask));
    // the tile's blended splats, front to back: the near list, then the far slice's (all zero for a tile the near slice finished)
    const uint32_t lo0 = tile_offsets[tile * 2], hi0 = tile_offsets[tile * 2 + 1];
    uint32_t lo1 = 0u, hi1 = 0u;
    if (tile_offsets_far) { lo1 = tile_offsets_far[tile * 2]; hi1 = tile_offsets_far[tile * 2 + 1]; }
    bool done = false;
#pragma nounroll
    for (int part = 0; part < 2 && !done; ++part) {
        const uint32_t range_lo = part ? lo1 : lo0, range_hi = part ? hi1 : hi0;
        for (uint32_t batch_start = range_lo; batch_start < range_hi && !done; batch_start += MAP_BATCH) {
            if (__ballot(any_live()) == 0ull) { done = true; break; }
            const uint32_t cnt = min((uint32_t)MAP_BATCH, range_hi - batch_start);
            __syncthreads();  // previous batch fully consumed (single wave: cheap)
            stage_map_batch<SMOOTH, P>(isect_gids, projected, attr, batch_start, cnt, lane, s_splat);
            __syncthreads();
            for (uint32_t t = 0; t < cnt; ++t) {
                const typename P::Rec r = P::load(&s_splat[t * P::STRIDE]);   // s0: x y c00/2 c01, s1: c11/2 a . .
                const uint32_t cut_bits = f2u(P::cut(r));
                float a_xx[2], b_x[2], c_y[2], dy[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const float dx = pcx[k] - r.s0.x;
                    a_xx[k] = (r.s0.z * dx) * dx;
                    b_x[k] = r.s0.w * dx;
                    dy[k] = pcy[k] - r.s0.y;
                    c_y[k] = r.s1.x * dy[k];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = q & 1, m = q >> 1;
                    const float half_qv = __builtin_fmaf(c_y[m], dy[m], a_xx[k]);
                    const float sigma = __builtin_fmaf(b_x[k], dy[m], half_qv);
                    const bool pre = ((f2u(tr[q]) & sign_mask) | f2u(sigma)) <= cut_bits;
                    if (__ballot(pre) != 0ull) {
                        const float alpha = blend_alpha(r.s1.y, sigma);
                        float alpha_eff, next_t;
                        bool sat;
                        const bool ok = blend_step<SMOOTH>(alpha, pre, tr[q], alpha_eff, next_t, sat);
                        P::fold(r, ok, sat, alpha_eff, next_t, tr[q], acc[q]);
                    }
                }
                // every pixel of the tile is done: the rest of the batch cannot contribute (checked every 8th splat, as K16 does)
                if ((t & 7u) == 7u && __ballot(any_live()) == 0ull) { done = true; break; }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t px = px0 + 8 * (q & 1), py = py0 + 8 * (q >> 1);
        if (px < u.img_w && py < u.img_h) P::store(out, attr, (size_t)px + (size_t)py * u.img_w, acc[q], tr[q]);
    }
}

// the blend over the saved lists of `r` (u.num_tiles > 0); the caller checks the launch under its kernel's name
template <class P>
void launch_map_forward(bh_ctx* ctx, const MapUniforms& u, bool smooth, const BhRenderOut& r, const typename P::Attr attr, float* out) {
    const dim3 grid(band_slots(u.num_tiles) * 8u, P::chunks(attr)), block(64);
    if (smooth)
        hipLaunchKernelGGL((map_forward_kernel<true, P>), grid, block, 0, ctx->stream, u, r.compact_gid_from_isect, r.tile_offsets, r.tile_offsets_far,
                           r.projected, attr, out);
    else
        hipLaunchKernelGGL((map_forward_kernel<false, P>), grid, block, 0, ctx->stream, u, r.compact_gid_from_isect, r.tile_offsets, r.tile_offsets_far,
                           r.projected, attr, out);
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
// One wave per tile, forward-order replay with the pixel state in registers like K17.  Per pixel a cotangent px (P::prologue) and
// S = the remaining sum of w_j cv_j, including the splat in flight, as in K17 (it needs the pixel's total: an accumulated-map
// forward into scratch precedes this kernel).  P Q R2 R3 R4 Vs join v_combined in K17's columns; V_i = sum of vis * vg_i goes to
// P::v_home in v_attr, which a small kernel of the map's own carries on behind K18.  v_alpha is linear in cv and S, so a map of
// several passes adds each pass's share.
template <bool SMOOTH, class P>
__global__ __launch_bounds__(64, P::BWD_WAVES) void map_backward_kernel(MapUniforms u, const uint32_t* __restrict__ isect_gids,
                                                                        const uint32_t* __restrict__ tile_offsets,
                                                                        const uint32_t* __restrict__ tile_offsets_far, const float* __restrict__ projected,
                                                                        const typename P::Attr attr, const typename P::BwdMaps maps,
                                                                        float* __restrict__ v_combined, float* __restrict__ v_attr) {
    constexpr int NV = P::NV, NVAL = 6 + NV, NG = (NVAL + 3) / 4;
    __shared__ __attribute__((aligned(16))) float s_splat[MAP_BATCH * P::STRIDE];
    __shared__ uint32_t s_cg[MAP_BATCH];
    const uint32_t local_tile = tile_of_block(blockIdx.x, u.num_tiles, u.band_mode);
    if (local_tile >= u.num_tiles) return;
    const uint32_t tile = u.tile_begin + local_tile;
    const uint32_t lo0 = tile_offsets[tile * 2], hi0 = tile_offsets[tile * 2 + 1];
    uint32_t lo1 = 0u, hi1 = 0u;
    if (tile_offsets_far) { lo1 = tile_offsets_far[tile * 2]; hi1 = tile_offsets_far[tile * 2 + 1]; }
    if (hi0 <= lo0 && hi1 <= lo1) return;
    const int lane = threadIdx.x;
    const uint32_t px0 = (tile % u.tile_bw) * TILE_WIDTH + (lane & 7), py0 = (tile / u.tile_bw) * TILE_WIDTH + (lane >> 3);
    const float pcx[2] = {(float)px0 + 0.5f, (float)(px0 + 8) + 0.5f};
    const float pcy[2] = {(float)py0 + 0.5f, (float)(py0 + 8) + 0.5f};
    float sS[4], sw[4];
    typename P::Pix pix[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t px = px0 + 8 * (q & 1), py = py0 + 8 * (q >> 1);
        sS[q] = sw[q] = 0.0f;
        pix[q] = typename P::Pix{};
        if (px < u.img_w && py < u.img_h) {
            sS[q] = P::prologue(maps, (size_t)px + (size_t)py * u.img_w, pix[q]);
            sw[q] = 1.0f;
        }
    }
    float val[NVAL];   // P Q R2 R3 R4 Vs V0 ..
#pragma unroll
    for (int i = 0; i < NVAL; ++i) val[i] = 0.0f;
#pragma nounroll
    for (int part = 0; part < 2; ++part) {
        const uint32_t range_lo = part ? lo1 : lo0, range_hi = part ? hi1 : hi0;
        for (uint32_t batch_start = range_lo; batch_start < range_hi; batch_start += MAP_BATCH) {
            const uint32_t cnt = min((uint32_t)MAP_BATCH, range_hi - batch_start);
            __syncthreads();
            const uint32_t my_cg = stage_map_batch<SMOOTH, P>(isect_gids, projected, attr, batch_start, cnt, lane, s_splat);
            s_cg[lane] = my_cg;
            __syncthreads();
            for (uint32_t t = 0; t < cnt; ++t) {
                const typename P::Rec r = P::load(&s_splat[t * P::STRIDE]);   // s0: x y c00/2 c01, s1: c11/2 a . .
                const uint32_t cut_bits = f2u(P::cut(r));
                float dxp[2], dyp[2], a_xx[2], b_x[2], c_y[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    dxp[k] = pcx[k] - r.s0.x;
                    a_xx[k] = (r.s0.z * dxp[k]) * dxp[k];
                    b_x[k] = r.s0.w * dxp[k];
                    dyp[k] = pcy[k] - r.s0.y;
                    c_y[k] = r.s1.x * dyp[k];
                }
                bool any = false;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = q & 1, m = q >> 1;
                    // --- replay: the forward's arithmetic, instruction for instruction ---
                    const float half_qv = __builtin_fmaf(c_y[m], dyp[m], a_xx[k]);
                    const float sigma = __builtin_fmaf(b_x[k], dyp[m], half_qv);
                    const bool pre = sw[q] > 0.0f && f2u(sigma) <= cut_bits;
                    if (__ballot(pre) != 0ull) {
                        const float alpha_raw = r.s1.y * exp_blend(-sigma);
                        const float alpha = __builtin_fminf(0.999f, alpha_raw);
                        const float T = sw[q];
                        float alpha_eff, next_t;
                        bool sat;
                        const bool ok = blend_step<SMOOTH>(alpha, pre, T, alpha_eff, next_t, sat);
                        sw[q] = (ok && sat) ? 0.0f : T;   // the pixel is done WITHOUT this splat
                        if (ok && !sat) {
                            // --- gradients (tolerance-checked) ---
                            const float vis = alpha_eff * T;
#pragma unroll
                            for (int i = 0; i < NV; ++i) val[6 + i] = __builtin_fmaf(vis, P::vg(r, pix[q], i), val[6 + i]);
                            const float cv = P::cv(r, pix[q]);
                            const float v_alpha_eff = __builtin_fmaf(T, cv, -sS[q]) * __builtin_amdgcn_rcpf(1.0f - alpha_eff);
                            const float v_alpha = SMOOTH ? v_alpha_eff * (alpha_cutoff_weight(alpha) + alpha * alpha_cutoff_weight_deriv(alpha)) : v_alpha_eff;
                            // geometry / opacity gradients only below the alpha clamp
                            const float v_sigma = alpha_raw <= 0.999f ? -alpha * v_alpha : 0.0f;
                            const float ux = v_sigma * dxp[k], uy = v_sigma * dyp[m];
                            val[0] += ux;
                            val[1] += uy;
                            val[2] = __builtin_fmaf(ux, dxp[k], val[2]);
                            val[3] = __builtin_fmaf(ux, dyp[m], val[3]);
                            val[4] = __builtin_fmaf(uy, dyp[m], val[4]);
                            val[5] += v_sigma;
                            sS[q] = __builtin_fmaf(-vis, cv, sS[q]);
                            sw[q] = next_t;
                            any = true;
                        }
                    }
                }
                if (__ballot(any) != 0ull) {
                    // the RAW sums leave through the register butterfly (the header has the numbering)
                    const int ri = lane & 15, rrow = lane >> 4;
                    const int comp = ((rrow & 1) << 1) | (rrow >> 1);   // which of a register's four sums this row holds
                    float mine = 0.0f;
#pragma unroll
                    for (int j = 0; j < NG; ++j) {
                        const float h0 = swap32_add(val[4 * j], 4 * j + 1 < NVAL ? val[4 * j + 1] : 0.0f);
                        const float h1 = 4 * j + 2 < NVAL ? swap32_add(val[4 * j + 2], 4 * j + 3 < NVAL ? val[4 * j + 3] : 0.0f) : 0.0f;
                        const float kj = row_allreduce(swap16_add(h0, h1));
                        mine = ri == j ? kj : mine;
                    }
                    const int vi = 4 * ri + comp;
                    const uint32_t cg = s_cg[t];
                    if (ri < NG && vi < NVAL) {
                        if (vi < 5) {
                            unsafeAtomicAdd(&v_combined[(size_t)cg * 10 + vi], mine);   // P Q R2 R3 R4: columns 0..4
                        } else if (vi == 5) {
                            unsafeAtomicAdd(&v_combined[(size_t)cg * 10 + 8], mine);    // Vs
                        } else if (float* home = P::v_home(maps, v_attr, cg, vi - 6)) {
                            unsafeAtomicAdd(home, mine);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < NVAL; ++i) val[i] = 0.0f;
                }
            }
        }
    }
}

// the term's replay (u.num_tiles > 0); the caller checks the launch under its kernel's name
template <class P>
void launch_map_backward(bh_ctx* ctx, const MapUniforms& u, bool smooth, const BhRenderOut& r, const typename P::Attr attr,
                         const typename P::BwdMaps& maps, float* v_combined, float* v_attr) {
    const dim3 grid(band_slots(u.num_tiles) * 8u, P::chunks(attr)), block(64);
    if (smooth)
        hipLaunchKernelGGL((map_backward_kernel<true, P>), grid, block, 0, ctx->stream, u, r.compact_gid_from_isect, r.tile_offsets, r.tile_offsets_far,
                           r.projected, attr, maps, v_combined, v_attr);
    else
        hipLaunchKernelGGL((map_backward_kernel<false, P>), grid, block, 0, ctx->stream, u, r.compact_gid_from_isect, r.tile_offsets, r.tile_offsets_far,
                           r.projected, attr, maps, v_combined, v_attr);
}

}  // namespace bh
