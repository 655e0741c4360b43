// depth.hip — depth maps of a rendered frame and their gradient (include/brush_hip_depth.h).
//
// A depth map is a second blend over the lists a BH_FLAG_BWD_INFO forward saved: the same splats in the same order with the same
// alpha, cut-off, clamp and saturation rule as the colour blend (device_blend.h holds the one copy of that arithmetic), folding the
// camera-space z of each splat (BhRenderOut.depths_sorted) where K16 folds its colour.  The tuned colour kernels K16 / K17 are not
// touched: a frame that asks for no depth pays nothing.
//
//   * forward: one wave64 per 16 x 16 tile, four pixels per lane (one per 8 x 8 quadrant) as in K16: wave-synchronous, the quadrant
//     skip is one scalar branch, the "every pixel is done" test one ballot.  A staged splat is 8 floats (32 B: x y c00/2 c01 |
//     c11/2 alpha0 z sigma_cut), two uniform ds_read_b128 per splat where K16 reads 40 bytes, and one fma per contributing pair where
//     K16 does three.  Median mode marks a pixel done as soon as its transmittance has crossed 1/2, so its tiles end earlier still.
//   * backward (accumulated and expected depth): one wave per tile, forward-order replay with the pixel state in registers like K17
//     (the "remaining" sum S needs the pixel's total, which is the accumulated depth map: a forward pass into scratch precedes it).
//     The RAW sums P Q R2 R3 R4 Vs are added to the [Nv,10] accumulator K17 fills (project.hip maps them once per splat), and
//     v_z = sum of v_D * w to a per-splat vector of its own, which a small kernel behind K18 carries to the means.
#include <algorithm>

#include "context.h"
#include "device_blend.h"
#include "../../include/brush_hip_depth.h"

namespace bh {

namespace {

constexpr int DEPTH_STRIDE = 8;   // floats per staged splat
constexpr int DEPTH_BATCH = 64;

struct DepthUniforms {
    uint32_t tile_bw, num_tiles, tile_begin, img_w, img_h, band_mode;
};

// block -> tile of the window (context.h XCD BANDS; >= num_tiles: the slot names no tile)
BH_DEV uint32_t depth_tile_of_block(uint32_t b, uint32_t num_tiles, uint32_t band_mode) {
    const uint32_t per = band_slots(num_tiles);
    const uint32_t i = b >> 3;
    return i < per ? band_tile(b & 7u, i, per, band_mode) : 0xFFFFFFFFu;
}

// lane i stages splat i of the batch; the diagonal of the conic halved as in K16 (bit-identical sigma, rasterize.hip stage_batch)
template <bool SMOOTH>
BH_DEV uint32_t stage_depth_batch(const uint32_t* __restrict__ isect_gids, const float* __restrict__ projected, const float* __restrict__ depths,
                                  uint32_t batch_start, uint32_t cnt, int lane, float* s_splat) {
    uint32_t cg = 0;
    if ((uint32_t)lane < cnt) {
        cg = isect_gids[batch_start + lane];
        const float* p = projected + (size_t)cg * 9;
        float v[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = p[k];
        const float z = depths[cg];
        float4* d = reinterpret_cast<float4*>(s_splat + lane * DEPTH_STRIDE);
        d[0] = make_float4(v[0], v[1], 0.5f * v[2], v[3]);
        d[1] = make_float4(0.5f * v[4], v[5], z, blend_sigma_cut<SMOOTH>(v[5]));
    }
    return cg;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
// MODE: BH_DEPTH_ACCUMULATED / EXPECTED / MEDIAN.  A finished pixel keeps a negative T (K16's convention: one unsigned compare
// tests "live and inside the cut").
template <bool SMOOTH, uint32_t MODE>
__global__ __launch_bounds__(64, 8) void depth_forward_kernel(DepthUniforms u, const uint32_t* __restrict__ isect_gids,
                                                              const uint32_t* __restrict__ tile_offsets, const uint32_t* __restrict__ tile_offsets_far,
                                                              const float* __restrict__ projected, const float* __restrict__ depths,
                                                              float* __restrict__ out_depth) {
    constexpr bool MEDIAN = MODE == BH_DEPTH_MEDIAN;
    __shared__ __attribute__((aligned(16))) float s_splat[DEPTH_BATCH * DEPTH_STRIDE];
    const uint32_t local_tile = depth_tile_of_block(blockIdx.x, u.num_tiles, u.band_mode);
    if (local_tile >= u.num_tiles) return;
    const uint32_t tile = u.tile_begin + local_tile;
    const int lane = threadIdx.x;
    const uint32_t px0 = (tile % u.tile_bw) * TILE_WIDTH + (lane & 7), py0 = (tile / u.tile_bw) * TILE_WIDTH + (lane >> 3);
    const float pcx[2] = {(float)px0 + 0.5f, (float)(px0 + 8) + 0.5f};
    const float pcy[2] = {(float)py0 + 0.5f, (float)(py0 + 8) + 0.5f};
    float tr[4], dd[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t px = px0 + 8 * (q & 1), py = py0 + 8 * (q >> 1);
        tr[q] = (px < u.img_w && py < u.img_h) ? 1.0f : -1.0f;
        dd[q] = 0.0f;
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
        for (uint32_t batch_start = range_lo; batch_start < range_hi && !done; batch_start += DEPTH_BATCH) {
            if (__ballot(any_live()) == 0ull) { done = true; break; }
            const uint32_t cnt = min((uint32_t)DEPTH_BATCH, range_hi - batch_start);
            __syncthreads();  // previous batch fully consumed (single wave: cheap)
            stage_depth_batch<SMOOTH>(isect_gids, projected, depths, batch_start, cnt, lane, s_splat);
            __syncthreads();
            for (uint32_t t = 0; t < cnt; ++t) {
                const float4 s0 = *reinterpret_cast<const float4*>(&s_splat[t * DEPTH_STRIDE]);      // x y c00/2 c01
                const float4 s1 = *reinterpret_cast<const float4*>(&s_splat[t * DEPTH_STRIDE + 4]);  // c11/2 a z sigma_cut
                const uint32_t cut_bits = f2u(s1.w);
                float a_xx[2], b_x[2], c_y[2], dy[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const float dx = pcx[k] - s0.x;
                    a_xx[k] = (s0.z * dx) * dx;
                    b_x[k] = s0.w * dx;
                    dy[k] = pcy[k] - s0.y;
                    c_y[k] = s1.x * dy[k];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = q & 1, m = q >> 1;
                    const float half_qv = __builtin_fmaf(c_y[m], dy[m], a_xx[k]);
                    const float sigma = __builtin_fmaf(b_x[k], dy[m], half_qv);
                    const bool pre = ((f2u(tr[q]) & sign_mask) | f2u(sigma)) <= cut_bits;
                    if (__ballot(pre) != 0ull) {
                        const float alpha = blend_alpha(s1.y, sigma);
                        float alpha_eff, next_t;
                        bool sat;
                        const bool ok = blend_step<SMOOTH>(alpha, pre, tr[q], alpha_eff, next_t, sat);
                        const bool contrib = ok && !sat;
                        if (MEDIAN) {
                            // T is monotone: it FIRST becomes <= 1/2 at the one contributing splat that finds it above and leaves it at or
                            // below.  Nothing behind that splat matters to the median: the pixel is done.
                            const bool hit = contrib && tr[q] > 0.5f && next_t <= 0.5f;
                            dd[q] = hit ? s1.z : dd[q];
                            tr[q] = ok ? ((sat || hit) ? -tr[q] : next_t) : tr[q];
                        } else {
                            const float vis = contrib ? alpha_eff * tr[q] : 0.0f;
                            dd[q] = __builtin_fmaf(s1.z, vis, dd[q]);   // (one explicit fma per term, as the colour channels)
                            tr[q] = ok ? (sat ? -tr[q] : next_t) : tr[q];
                        }
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
        if (px < u.img_w && py < u.img_h) {
            float v = dd[q];
            if (MODE == BH_DEPTH_EXPECTED) {
                const float a = 1.0f - __builtin_fabsf(tr[q]);   // the colour image's alpha, bit for bit (rasterize.hip store_pixels)
                v = a == 0.0f ? 0.0f : v / a;
            }
            out_depth[(size_t)px + (size_t)py * u.img_w] = v;
        }
    }
}

// ---------------------------------------------------------------------------
// backward (accumulated and expected depth)
// ---------------------------------------------------------------------------
// Expected depth E = D / A with A = sum of w: dE = (1/A) sum of dw_i (z_i - E) + (1/A) sum of w_i dz_i.  So both modes are ONE
// replay with a per-pixel gain g and offset e: the "colour" of splat i at the pixel is z_i - e and the pixel's cotangent is g
// (accumulated: g = v_D, e = 0; expected: g = v_D / A, e = E, 0 where A == 0) — the chain through 1/A, which is a gradient on the
// alpha channel, is the offset.  S = g * (remaining sum of w_j (z_j - e)), including the splat in flight, as in K17.
template <bool SMOOTH>
__global__ __launch_bounds__(64, 6) void depth_backward_kernel(DepthUniforms u, const uint32_t expected, const uint32_t* __restrict__ isect_gids,
                                                               const uint32_t* __restrict__ tile_offsets, const uint32_t* __restrict__ tile_offsets_far,
                                                               const float* __restrict__ projected, const float* __restrict__ depths,
                                                               const float* __restrict__ out_img, const float* __restrict__ depth_acc,
                                                               const float* __restrict__ v_depth, float* __restrict__ v_combined,
                                                               float* __restrict__ v_z) {
    __shared__ __attribute__((aligned(16))) float s_splat[DEPTH_BATCH * DEPTH_STRIDE];
    __shared__ uint32_t s_cg[DEPTH_BATCH];
    const uint32_t local_tile = depth_tile_of_block(blockIdx.x, u.num_tiles, u.band_mode);
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
    float sS[4], sw[4], gq[4], eq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t px = px0 + 8 * (q & 1), py = py0 + 8 * (q >> 1);
        sS[q] = sw[q] = gq[q] = eq[q] = 0.0f;
        if (px < u.img_w && py < u.img_h) {
            const size_t pix = (size_t)px + (size_t)py * u.img_w;
            const float a = out_img[pix * 4 + 3], d = depth_acc[pix], v = v_depth[pix];
            if (expected) {
                const bool has = a > 0.0f;
                gq[q] = has ? v / a : 0.0f;
                eq[q] = has ? d / a : 0.0f;
            } else {
                gq[q] = v;
            }
            sS[q] = gq[q] * __builtin_fmaf(-eq[q], a, d);
            sw[q] = 1.0f;
        }
    }
    float aP = 0.f, aQ = 0.f, aR2 = 0.f, aR3 = 0.f, aR4 = 0.f, aVs = 0.f, aVz = 0.f;
#pragma nounroll
    for (int part = 0; part < 2; ++part) {
        const uint32_t range_lo = part ? lo1 : lo0, range_hi = part ? hi1 : hi0;
        for (uint32_t batch_start = range_lo; batch_start < range_hi; batch_start += DEPTH_BATCH) {
            const uint32_t cnt = min((uint32_t)DEPTH_BATCH, range_hi - batch_start);
            __syncthreads();
            const uint32_t my_cg = stage_depth_batch<SMOOTH>(isect_gids, projected, depths, batch_start, cnt, lane, s_splat);
            s_cg[lane] = my_cg;
            __syncthreads();
            for (uint32_t t = 0; t < cnt; ++t) {
                const float4 s0 = *reinterpret_cast<const float4*>(&s_splat[t * DEPTH_STRIDE]);      // x y c00/2 c01
                const float4 s1 = *reinterpret_cast<const float4*>(&s_splat[t * DEPTH_STRIDE + 4]);  // c11/2 a z sigma_cut
                const uint32_t cut_bits = f2u(s1.w);
                float dxp[2], dyp[2], a_xx[2], b_x[2], c_y[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    dxp[k] = pcx[k] - s0.x;
                    a_xx[k] = (s0.z * dxp[k]) * dxp[k];
                    b_x[k] = s0.w * dxp[k];
                    dyp[k] = pcy[k] - s0.y;
                    c_y[k] = s1.x * dyp[k];
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
                        const float alpha_raw = s1.y * exp_blend(-sigma);
                        const float alpha = __builtin_fminf(0.999f, alpha_raw);
                        const float T = sw[q];
                        float alpha_eff, next_t;
                        bool sat;
                        const bool ok = blend_step<SMOOTH>(alpha, pre, T, alpha_eff, next_t, sat);
                        sw[q] = (ok && sat) ? 0.0f : T;   // the pixel is done WITHOUT this splat
                        if (ok && !sat) {
                            // --- gradients (tolerance-checked) ---
                            const float vis = alpha_eff * T;
                            aVz = __builtin_fmaf(vis, gq[q], aVz);
                            const float cv = gq[q] * (s1.z - eq[q]);
                            const float v_alpha_eff = __builtin_fmaf(T, cv, -sS[q]) * __builtin_amdgcn_rcpf(1.0f - alpha_eff);
                            const float v_alpha = SMOOTH ? v_alpha_eff * (alpha_cutoff_weight(alpha) + alpha * alpha_cutoff_weight_deriv(alpha)) : v_alpha_eff;
                            // geometry / opacity gradients only below the alpha clamp
                            const float v_sigma = alpha_raw <= 0.999f ? -alpha * v_alpha : 0.0f;
                            const float ux = v_sigma * dxp[k], uy = v_sigma * dyp[m];
                            aP += ux;
                            aQ += uy;
                            aR2 = __builtin_fmaf(ux, dxp[k], aR2);
                            aR3 = __builtin_fmaf(ux, dyp[m], aR3);
                            aR4 = __builtin_fmaf(uy, dyp[m], aR4);
                            aVs += v_sigma;
                            sS[q] = __builtin_fmaf(-vis, cv, sS[q]);
                            sw[q] = next_t;
                            any = true;
                        }
                    }
                }
                if (__ballot(any) != 0ull) {
                    // the seven RAW sums leave through K17's register butterfly: k0 holds P R2 Q R3 in rows 0..3, k1 R4 Vz Vs -
                    const float h0 = swap32_add(aP, aQ), h1 = swap32_add(aR2, aR3), h2 = swap32_add(aR4, aVs), h3 = swap32_add(aVz, 0.0f);
                    const float k0 = row_allreduce(swap16_add(h0, h1));
                    const float k1 = row_allreduce(swap16_add(h2, h3));
                    const int ri = lane & 15, rrow = lane >> 4;
                    const int c = ((rrow & 1) << 1) | (rrow >> 1);   // which of the register's four components this row holds
                    const uint32_t cg = s_cg[t];
                    if (ri == 0) {
                        unsafeAtomicAdd(&v_combined[(size_t)cg * 10 + c], k0);               // P Q R2 R3: columns 0..3
                    } else if (ri == 1) {
                        if (c == 0) unsafeAtomicAdd(&v_combined[(size_t)cg * 10 + 4], k1);   // R4
                        else if (c == 1) unsafeAtomicAdd(&v_combined[(size_t)cg * 10 + 8], k1);   // Vs
                        else if (c == 2) unsafeAtomicAdd(&v_z[cg], k1);
                    }
                    aP = aQ = aR2 = aR3 = aR4 = aVs = aVz = 0.0f;
                }
            }
        }
    }
}

// v_mean += (row 2 of the view matrix) * v_z, behind K18: a row K18 skipped (its ten sums are zero) is zero in the dense output
__global__ __launch_bounds__(256) void depth_vz_scatter_kernel(uint32_t nv, float r0, float r1, float r2, const uint32_t* __restrict__ global_from_compact,
                                                               const float* __restrict__ v_z, float* __restrict__ v_transforms) {
    const uint32_t cg = blockIdx.x * 256u + threadIdx.x;
    if (cg >= nv) return;
    const float vz = v_z[cg];
    if (vz == 0.0f) return;
    float* vt = v_transforms + (size_t)global_from_compact[cg] * 10;
    vt[0] = __builtin_fmaf(r0, vz, vt[0]);
    vt[1] = __builtin_fmaf(r1, vz, vt[1]);
    vt[2] = __builtin_fmaf(r2, vz, vt[2]);
}

// The same behind a K18 in marking mode (the single-GPU train step: only the refine-weight vector was cleared, K18 marked the rows
// it wrote in that vector's sign bits and the update reads marked rows only).  K18 skips a splat whose ten sums are all zero — one
// whose every pair sat at the alpha clamp still has a v_z — so a row that receives v_z may hold last step's bytes and carry no
// mark: such a row is STORED whole (what a zero-filled row would hold after the accumulate above, bit for bit) and marked.  The
// mark is the sign of a zero: the refine weight itself is not touched.
__global__ __launch_bounds__(256) void depth_vz_scatter_marking_kernel(uint32_t nv, float r0, float r1, float r2, uint32_t sh_floats,
                                                                       const uint32_t* __restrict__ global_from_compact, const float* __restrict__ v_z,
                                                                       float* __restrict__ v_transforms, float* __restrict__ v_sh, float* __restrict__ v_raw_opac,
                                                                       float* __restrict__ v_refine) {
    const uint32_t cg = blockIdx.x * 256u + threadIdx.x;
    if (cg >= nv) return;
    const float vz = v_z[cg];
    if (vz == 0.0f) return;
    const uint32_t gid = global_from_compact[cg];
    float* vt = v_transforms + (size_t)gid * 10;
    const uint32_t mark = f2u(v_refine[gid]);
    if (mark >> 31) {
        vt[0] = __builtin_fmaf(r0, vz, vt[0]);
        vt[1] = __builtin_fmaf(r1, vz, vt[1]);
        vt[2] = __builtin_fmaf(r2, vz, vt[2]);
        return;
    }
    vt[0] = __builtin_fmaf(r0, vz, 0.0f);
    vt[1] = __builtin_fmaf(r1, vz, 0.0f);
    vt[2] = __builtin_fmaf(r2, vz, 0.0f);
#pragma unroll
    for (int k = 3; k < 10; ++k) vt[k] = 0.0f;
    float* sh = v_sh + (size_t)gid * sh_floats;
    for (uint32_t k = 0; k < sh_floats; ++k) sh[k] = 0.0f;
    v_raw_opac[gid] = 0.0f;
    v_refine[gid] = u2f(mark | 0x80000000u);
}

DepthUniforms depth_uniforms(const bh_ctx* ctx, const ViewUniforms& vu) {
    DepthUniforms u;
    u.tile_bw = vu.tile_bw;
    u.num_tiles = vu.tile_bw * (vu.tile_y1 - vu.tile_y0);
    u.tile_begin = vu.tile_bw * vu.tile_y0;
    u.img_w = vu.img_w;
    u.img_h = vu.img_h;
    u.band_mode = ctx->knob_band_mode;
    return u;
}

}  // namespace

int launch_depth_forward(bh_ctx* ctx, const ForwardState& fs, uint32_t mode, float* out_depth) {
    const BhRenderOut& r = fs.out;
    const DepthUniforms u = depth_uniforms(ctx, fs.uniforms);
    if (u.num_tiles == 0) return 0;
    const dim3 grid(band_slots(u.num_tiles) * 8u), block(64);
    const bool smooth = fs.flags & BH_FLAG_SMOOTH_CUTOFF;
#define BH_DEPTH_FWD(S, M) hipLaunchKernelGGL((depth_forward_kernel<S, M>), grid, block, 0, ctx->stream, u, r.compact_gid_from_isect, r.tile_offsets, r.tile_offsets_far, r.projected, r.depths_sorted, out_depth)
    switch (mode) {
        case BH_DEPTH_ACCUMULATED: if (smooth) BH_DEPTH_FWD(true, BH_DEPTH_ACCUMULATED); else BH_DEPTH_FWD(false, BH_DEPTH_ACCUMULATED); break;
        case BH_DEPTH_EXPECTED: if (smooth) BH_DEPTH_FWD(true, BH_DEPTH_EXPECTED); else BH_DEPTH_FWD(false, BH_DEPTH_EXPECTED); break;
        case BH_DEPTH_MEDIAN: if (smooth) BH_DEPTH_FWD(true, BH_DEPTH_MEDIAN); else BH_DEPTH_FWD(false, BH_DEPTH_MEDIAN); break;
        default: return set_error(ctx, BH_ERR_INVALID_ARG, "render_depth: unknown depth mode");
    }
#undef BH_DEPTH_FWD
    BH_LAUNCH_CHECK(ctx, "depth_forward_kernel");
    return 0;
}

// The depth term of a backward, between K17 and K18: v_combined += its raw sums, v_z (SLOT_DEPTH) = sum of v_D * w.
int launch_depth_backward(bh_ctx* ctx, const ForwardState& fs, const DepthTerm& term, float* v_combined) {
    const BhRenderOut& r = fs.out;
    const uint32_t nv = r.num_listed_splats;
    const DepthUniforms u = depth_uniforms(ctx, fs.uniforms);
    // SLOT_DEPTH: v_z [Nv] (padded to a multiple of 64 floats) | the frame's accumulated depth [H,W]
    const size_t vz_floats = ((size_t)(nv ? nv : 1u) + 63u) & ~(size_t)63u;
    const size_t pixels = (size_t)u.img_w * u.img_h;
    auto* v_z = (float*)ensure(ctx, SLOT_DEPTH, (vz_floats + pixels) * 4);
    if (!v_z) return BH_ERR_OOM;
    float* depth_acc = v_z + vz_floats;
    BH_HIP(ctx, hipMemsetAsync(v_z, 0, vz_floats * 4, ctx->stream));
    if (r.num_intersections == 0 || u.num_tiles == 0) return 0;
    BH_TRY(launch_depth_forward(ctx, fs, BH_DEPTH_ACCUMULATED, depth_acc));
    const dim3 grid(band_slots(u.num_tiles) * 8u), block(64);
    const uint32_t expected = term.mode == BH_DEPTH_EXPECTED ? 1u : 0u;
    if (fs.flags & BH_FLAG_SMOOTH_CUTOFF)
        hipLaunchKernelGGL((depth_backward_kernel<true>), grid, block, 0, ctx->stream, u, expected, r.compact_gid_from_isect, r.tile_offsets, r.tile_offsets_far,
                           r.projected, r.depths_sorted, r.out_img, depth_acc, term.v_depth, v_combined, v_z);
    else
        hipLaunchKernelGGL((depth_backward_kernel<false>), grid, block, 0, ctx->stream, u, expected, r.compact_gid_from_isect, r.tile_offsets, r.tile_offsets_far,
                           r.projected, r.depths_sorted, r.out_img, depth_acc, term.v_depth, v_combined, v_z);
    BH_LAUNCH_CHECK(ctx, "depth_backward_kernel");
    return 0;
}

int launch_depth_vz_scatter(bh_ctx* ctx, const ForwardState& fs, float* v_transforms, bool mark_rows, float* v_sh_coeffs, float* v_raw_opacities,
                            float* v_refine_weight) {
    const BhRenderOut& r = fs.out;
    const uint32_t nv = r.num_listed_splats;
    if (nv == 0 || r.num_intersections == 0) return 0;
    const float* v_z = (const float*)ctx->slots[SLOT_DEPTH].ptr;
    const float* vm = fs.uniforms.vm;   // column-major rotation: row 2 = (vm[2], vm[5], vm[8])
    if (mark_rows) {
        const uint32_t sh_floats = (fs.sh_degree + 1) * (fs.sh_degree + 1) * 3;
        hipLaunchKernelGGL(depth_vz_scatter_marking_kernel, dim3((nv + 255u) / 256u), dim3(256), 0, ctx->stream, nv, vm[2], vm[5], vm[8], sh_floats,
                           r.global_from_compact_gid, v_z, v_transforms, v_sh_coeffs, v_raw_opacities, v_refine_weight);
        BH_LAUNCH_CHECK(ctx, "depth_vz_scatter_marking_kernel");
        return 0;
    }
    hipLaunchKernelGGL(depth_vz_scatter_kernel, dim3((nv + 255u) / 256u), dim3(256), 0, ctx->stream, nv, vm[2], vm[5], vm[8], r.global_from_compact_gid, v_z,
                       v_transforms);
    BH_LAUNCH_CHECK(ctx, "depth_vz_scatter_kernel");
    return 0;
}

}  // namespace bh

extern "C" {

int bh_render_depth(bh_ctx* ctx, const BhRenderOut* saved, uint32_t mode, float* out_depth) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!saved || !out_depth) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "render_depth: null argument");
    if (mode > BH_DEPTH_MEDIAN) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "render_depth: unknown depth mode");
    if (!(saved->flags & BH_FLAG_BWD_INFO)) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "render_depth: the saved forward was not a BH_FLAG_BWD_INFO forward");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    const bh::ForwardState* found = nullptr;
    BH_TRY(bh::find_saved_forward(ctx, saved, "render_depth", &found));
    const bh::ForwardState& fs = *found;
    if (fs.out.num_intersections == 0) {   // nothing listed: every mode is 0 over the rendered window
        const bh::ViewUniforms& vu = fs.uniforms;
        const size_t row0 = (size_t)vu.tile_y0 * bh::TILE_WIDTH, row1 = std::min<size_t>((size_t)vu.tile_y1 * bh::TILE_WIDTH, vu.img_h);
        if (row1 > row0) BH_HIP(ctx, hipMemsetAsync(out_depth + row0 * vu.img_w, 0, (row1 - row0) * vu.img_w * 4, ctx->stream));
        return 0;
    }
    bh::ProfScope ps(ctx, "RenderDepth");
    return bh::launch_depth_forward(ctx, fs, mode, out_depth);
}

int bh_render_backward_depth_saved(bh_ctx* ctx, const BhRenderOut* saved, const float* v_output, const float* v_depth, uint32_t mode,
                                   const float* transforms, const float* sh_coeffs, const float* raw_opacities, float* v_transforms,
                                   float* v_sh_coeffs, float* v_raw_opacities, float* v_refine_weight) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!saved || !v_depth || !v_transforms || !v_sh_coeffs || !v_raw_opacities || !v_refine_weight)
        return bh::set_error(ctx, BH_ERR_INVALID_ARG, "render_backward_depth_saved: null argument");
    if (mode == BH_DEPTH_MEDIAN) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "render_backward_depth_saved: median depth has no gradient");
    if (mode > BH_DEPTH_MEDIAN) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "render_backward_depth_saved: unknown depth mode");
    if (!(saved->flags & BH_FLAG_BWD_INFO)) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "render_backward_depth_saved: the saved forward was not a BH_FLAG_BWD_INFO forward");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    const bh::ForwardState* found = nullptr;
    BH_TRY(bh::find_saved_forward(ctx, saved, "render_backward_depth_saved", &found));
    const bh::ForwardState& fs = *found;
    bh::DepthTerm term;
    term.v_depth = v_depth;
    term.mode = mode;
    return bh::backward_impl(ctx, fs, v_output, transforms, sh_coeffs, raw_opacities, v_transforms, v_sh_coeffs, v_raw_opacities, v_refine_weight,
                             /*span_floats=*/0, /*want_refine=*/true, &term);
}

}  // extern "C"
