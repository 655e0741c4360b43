// features.hip — feature maps of a rendered frame: the blend of caller-owned per-splat vectors with any channel count, its
// gradient, and two fused losses on such a map (include/brush_hip_features.h).
//
// A feature map is one more blend over the lists a BH_FLAG_BWD_INFO forward saved, as a depth or a normal map is: the same splats in
// the same order with the same alpha, cut-off, clamp and saturation rule as the colour blend (device_blend.h holds the one copy of
// that arithmetic).  The skeleton of the other maps (device_map_blend.h) keeps NACC accumulators per pixel and at most three
// per-splat sums through a fixed register butterfly; that does not stretch to 16, 64 or 256 channels, so the kernels here stand
// BESIDE it and share its host pieces (MapUniforms, clear_map_window, splat_vec_floats) and device_blend.h.  No existing kernel is
// touched: a process that never calls these entry points launches nothing new.
//
//   * gather: features[global_from_compact_gid[cg], :] -> a compact [Nv,C] array, what the two blends stage (as normals do);
//   * forward: one wave64 per 16 x 16 tile and CHUNK of CH channels (blockIdx.y), four pixels per lane.  A chunk is one pass over
//     the tile's lists with the skeleton's staging (x y c00/2 c01 | c11/2 alpha0 sigma_cut - | CH features) and 4 CH accumulators per
//     lane, one explicit fma per channel and term.  CH is a template parameter (4, 8, 16): the trade is passes over the lists
//     against registers, i.e. waves per SIMD; feature_chunk() picks per C;
//   * backward: per chunk a forward-order replay, instruction for instruction, with g[CH] per pixel in registers: the "colour" of a
//     splat is cv = sum of g_c f_c over the chunk, the remaining sum S starts at sum of g_c F_c (an accumulated-map forward into
//     scratch precedes the replay).  v_alpha is linear in cv and S, so every chunk adds its share of P Q R2 R3 R4 Vs to v_combined,
//     between K17 and K18.  The 6 + CH per-splat sums leave through the register butterfly four to a register (swap32 / swap16 /
//     one row reduction per FOUR values), V by f32 atomics into a compact [Nv,C] that a small kernel behind K18 carries to the dense
//     v_features;
//   * losses: one streaming kernel, a pixel per lane, f64 sums in the fixed order of the other pixel losses.
#include <cmath>

#include "context.h"
#include "device_map_blend.h"
#include "device_f64_sum.h"
#include "../../include/brush_hip_features.h"

namespace bh {

namespace {

__global__ __launch_bounds__(256) void feature_gather_kernel(uint64_t total, uint32_t channels, const uint32_t* __restrict__ gid,
                                                             const float* __restrict__ features, float* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const uint64_t cg = i / channels, c = i - cg * channels;
    out[i] = features[(uint64_t)gid[cg] * channels + c];
}

// compact [Nv,C] -> rows gid of the zero-filled dense [N,C]
__global__ __launch_bounds__(256) void feature_scatter_kernel(uint64_t total, uint32_t channels, const uint32_t* __restrict__ gid,
                                                              const float* __restrict__ v_compact, float* __restrict__ v_features) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const uint64_t cg = i / channels, c = i - cg * channels;
    v_features[(uint64_t)gid[cg] * channels + c] = v_compact[i];
}

// lane i stages splat i of the batch: the conic's diagonal halved as in K16 (bit-identical sigma), then channels c0 .. c0 + CH of
// its compact feature row (0 behind the last channel)
template <bool SMOOTH, int CH>
BH_DEV uint32_t stage_feature_batch(const uint32_t* __restrict__ isect_gids, const float* __restrict__ projected, const float* __restrict__ feat,
                                    uint32_t channels, uint32_t c0, uint32_t batch_start, uint32_t cnt, int lane, float* s_splat) {
    constexpr int STRIDE = 8 + CH;
    uint32_t cg = 0;
    if ((uint32_t)lane < cnt) {
        cg = isect_gids[batch_start + lane];
        const float* p = projected + (size_t)cg * 9;
        float v[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = p[k];
        float4* d = reinterpret_cast<float4*>(s_splat + lane * STRIDE);
        d[0] = make_float4(v[0], v[1], 0.5f * v[2], v[3]);
        d[1] = make_float4(0.5f * v[4], v[5], blend_sigma_cut<SMOOTH>(v[5]), 0.0f);
        const float* f = feat + (size_t)cg * channels + c0;
        float x[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) x[i] = c0 + i < channels ? f[i] : 0.0f;
#pragma unroll
        for (int i = 0; i < CH / 4; ++i) d[2 + i] = make_float4(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]);
    }
    return cg;
}

template <int CH>
BH_DEV void load_features(const float* p, float (&f)[CH]) {
#pragma unroll
    for (int i = 0; i < CH / 4; ++i) {
        const float4 x = *reinterpret_cast<const float4*>(p + 8 + 4 * i);
        f[4 * i] = x.x; f[4 * i + 1] = x.y; f[4 * i + 2] = x.z; f[4 * i + 3] = x.w;
    }
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
// map_forward_kernel's loop (device_map_blend.h) with CH accumulators per pixel; blockIdx.y is the chunk
template <bool SMOOTH, int CH>
__global__ __launch_bounds__(64) void feature_forward_kernel(MapUniforms u, uint32_t channels, const uint32_t* __restrict__ isect_gids,
                                                             const uint32_t* __restrict__ tile_offsets, const uint32_t* __restrict__ tile_offsets_far,
                                                             const float* __restrict__ projected, const float* __restrict__ feat,
                                                             float* __restrict__ out) {
    constexpr int STRIDE = 8 + CH;
    __shared__ __attribute__((aligned(16))) float s_splat[MAP_BATCH * STRIDE];
    const uint32_t local_tile = tile_of_block(blockIdx.x, u.num_tiles, u.band_mode);
    if (local_tile >= u.num_tiles) return;
    const uint32_t tile = u.tile_begin + local_tile;
    const uint32_t c0 = blockIdx.y * CH;
    const int lane = threadIdx.x;
    const uint32_t px0 = (tile % u.tile_bw) * TILE_WIDTH + (lane & 7), py0 = (tile / u.tile_bw) * TILE_WIDTH + (lane >> 3);
    const float pcx[2] = {(float)px0 + 0.5f, (float)(px0 + 8) + 0.5f};
    const float pcy[2] = {(float)py0 + 0.5f, (float)(py0 + 8) + 0.5f};
    float tr[4], acc[4][CH];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t px = px0 + 8 * (q & 1), py = py0 + 8 * (q >> 1);
        tr[q] = (px < u.img_w && py < u.img_h) ? 1.0f : -1.0f;
#pragma unroll
        for (int i = 0; i < CH; ++i) acc[q][i] = 0.0f;
    }
    auto any_live = [&]() {
        bool l = false;
#pragma unroll
        for (int q = 0; q < 4; ++q) l = l || tr[q] > 0.0f;
        return l;
    };
    uint32_t sign_mask = 0x80000000u;   // kept in a VGPR: an SGPR operand halves a VALU op's issue rate
    asm volatile("" : "+v"(sign_mask));
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
            stage_feature_batch<SMOOTH, CH>(isect_gids, projected, feat, channels, c0, batch_start, cnt, lane, s_splat);
            __syncthreads();
            for (uint32_t t = 0; t < cnt; ++t) {
                const float* rec = &s_splat[t * STRIDE];
                const float4 s0 = *reinterpret_cast<const float4*>(rec);       // x y c00/2 c01
                const float4 s1 = *reinterpret_cast<const float4*>(rec + 4);   // c11/2 a sigma_cut -
                float f[CH];
                load_features<CH>(rec, f);
                const uint32_t cut_bits = f2u(s1.z);
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
                        const float vis = (ok && !sat) ? alpha_eff * tr[q] : 0.0f;
#pragma unroll
                        for (int i = 0; i < CH; ++i) acc[q][i] = __builtin_fmaf(f[i], vis, acc[q][i]);   // (one explicit fma per channel and term: the contract)
                        tr[q] = ok ? (sat ? -tr[q] : next_t) : tr[q];
                    }
                }
                if ((t & 7u) == 7u && __ballot(any_live()) == 0ull) { done = true; break; }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t px = px0 + 8 * (q & 1), py = py0 + 8 * (q >> 1);
        if (px < u.img_w && py < u.img_h) {
            float* o = out + ((size_t)px + (size_t)py * u.img_w) * channels + c0;
#pragma unroll
            for (int i = 0; i < CH; ++i)
                if (c0 + i < channels) o[i] = acc[q][i];
        }
    }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
// map_backward_kernel's replay (device_map_blend.h) with a CH-vector cotangent per pixel; blockIdx.y is the chunk.  The 6 + CH
// per-splat sums are numbered P Q R2 R3 | R4 Vs V0 V1 | V2 .. and leave four to a register: after the butterfly every lane of
// 16-lane row r of k[j] holds sum 4 j + comp(r), comp = 0 2 1 3 for rows 0..3 (device_blend.h), and lane j of each row adds it to
// its home: one swap32 pair, one swap16 and one row reduction per FOUR sums.
template <bool SMOOTH, int CH>
__global__ __launch_bounds__(64) void feature_backward_kernel(MapUniforms u, uint32_t channels, const uint32_t* __restrict__ isect_gids,
                                                              const uint32_t* __restrict__ tile_offsets, const uint32_t* __restrict__ tile_offsets_far,
                                                              const float* __restrict__ projected, const float* __restrict__ feat,
                                                              const float* __restrict__ map_acc, const float* __restrict__ v_map,
                                                              float* __restrict__ v_combined, float* __restrict__ v_feat) {
    constexpr int STRIDE = 8 + CH, NVAL = 6 + CH, NG = (NVAL + 3) / 4;
    __shared__ __attribute__((aligned(16))) float s_splat[MAP_BATCH * STRIDE];
    __shared__ uint32_t s_cg[MAP_BATCH];
    const uint32_t local_tile = tile_of_block(blockIdx.x, u.num_tiles, u.band_mode);
    if (local_tile >= u.num_tiles) return;
    const uint32_t tile = u.tile_begin + local_tile;
    const uint32_t lo0 = tile_offsets[tile * 2], hi0 = tile_offsets[tile * 2 + 1];
    uint32_t lo1 = 0u, hi1 = 0u;
    if (tile_offsets_far) { lo1 = tile_offsets_far[tile * 2]; hi1 = tile_offsets_far[tile * 2 + 1]; }
    if (hi0 <= lo0 && hi1 <= lo1) return;
    const uint32_t c0 = blockIdx.y * CH;
    const int lane = threadIdx.x;
    const uint32_t px0 = (tile % u.tile_bw) * TILE_WIDTH + (lane & 7), py0 = (tile / u.tile_bw) * TILE_WIDTH + (lane >> 3);
    const float pcx[2] = {(float)px0 + 0.5f, (float)(px0 + 8) + 0.5f};
    const float pcy[2] = {(float)py0 + 0.5f, (float)(py0 + 8) + 0.5f};
    float sS[4], sw[4], g[4][CH];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t px = px0 + 8 * (q & 1), py = py0 + 8 * (q >> 1);
        sS[q] = sw[q] = 0.0f;
#pragma unroll
        for (int i = 0; i < CH; ++i) g[q][i] = 0.0f;
        if (px < u.img_w && py < u.img_h) {
            const size_t base = ((size_t)px + (size_t)py * u.img_w) * channels + c0;
            float s = 0.0f;
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                if (c0 + i < channels) {
                    g[q][i] = v_map[base + i];
                    s = __builtin_fmaf(g[q][i], map_acc[base + i], s);
                }
            }
            sS[q] = s;   // the chunk's share of the pixel's remaining sum
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
            const uint32_t my_cg = stage_feature_batch<SMOOTH, CH>(isect_gids, projected, feat, channels, c0, batch_start, cnt, lane, s_splat);
            s_cg[lane] = my_cg;
            __syncthreads();
            for (uint32_t t = 0; t < cnt; ++t) {
                const float* rec = &s_splat[t * STRIDE];
                const float4 s0 = *reinterpret_cast<const float4*>(rec);
                const float4 s1 = *reinterpret_cast<const float4*>(rec + 4);
                float f[CH];
                load_features<CH>(rec, f);
                const uint32_t cut_bits = f2u(s1.z);
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
                            float cv = 0.0f;
#pragma unroll
                            for (int i = 0; i < CH; ++i) {
                                val[6 + i] = __builtin_fmaf(vis, g[q][i], val[6 + i]);
                                cv = __builtin_fmaf(g[q][i], f[i], cv);
                            }
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
                        if (vi < 5) unsafeAtomicAdd(&v_combined[(size_t)cg * 10 + vi], mine);        // P Q R2 R3 R4: columns 0..4
                        else if (vi == 5) unsafeAtomicAdd(&v_combined[(size_t)cg * 10 + 8], mine);   // Vs
                        else if (c0 + (uint32_t)(vi - 6) < channels) unsafeAtomicAdd(&v_feat[(size_t)cg * channels + c0 + (vi - 6)], mine);
                    }
#pragma unroll
                    for (int i = 0; i < NVAL; ++i) val[i] = 0.0f;
                }
            }
        }
    }
}

// The chunk width for C channels.  One pass over the lists per chunk, so the widest chunk that does not waste most of itself:
// DESIGN.md §6r has the measurement behind the thresholds.
uint32_t feature_chunk(uint32_t channels) { return channels <= 4u ? 4u : (channels <= 8u ? 8u : 16u); }

template <int CH>
void launch_forward_width(bh_ctx* ctx, const MapUniforms& u, bool smooth, const BhRenderOut& r, uint32_t channels, const float* feat, float* out) {
    const dim3 grid(band_slots(u.num_tiles) * 8u, (channels + CH - 1) / CH), block(64);
    if (smooth)
        hipLaunchKernelGGL((feature_forward_kernel<true, CH>), grid, block, 0, ctx->stream, u, channels, r.compact_gid_from_isect, r.tile_offsets,
                           r.tile_offsets_far, r.projected, feat, out);
    else
        hipLaunchKernelGGL((feature_forward_kernel<false, CH>), grid, block, 0, ctx->stream, u, channels, r.compact_gid_from_isect, r.tile_offsets,
                           r.tile_offsets_far, r.projected, feat, out);
}

template <int CH>
void launch_backward_width(bh_ctx* ctx, const MapUniforms& u, bool smooth, const BhRenderOut& r, uint32_t channels, const float* feat, const float* acc,
                           const float* v_map, float* v_combined, float* v_feat) {
    const dim3 grid(band_slots(u.num_tiles) * 8u, (channels + CH - 1) / CH), block(64);
    if (smooth)
        hipLaunchKernelGGL((feature_backward_kernel<true, CH>), grid, block, 0, ctx->stream, u, channels, r.compact_gid_from_isect, r.tile_offsets,
                           r.tile_offsets_far, r.projected, feat, acc, v_map, v_combined, v_feat);
    else
        hipLaunchKernelGGL((feature_backward_kernel<false, CH>), grid, block, 0, ctx->stream, u, channels, r.compact_gid_from_isect, r.tile_offsets,
                           r.tile_offsets_far, r.projected, feat, acc, v_map, v_combined, v_feat);
}

// the blend of the compact rows `feat` into `out` (option feature_chunk forces a width: the probe's, and the tests')
int launch_feature_forward(bh_ctx* ctx, const ForwardState& fs, uint32_t channels, const float* feat, float* out) {
    const MapUniforms u = map_uniforms(ctx, fs.uniforms);
    if (u.num_tiles == 0) return 0;
    const bool smooth = fs.flags & BH_FLAG_SMOOTH_CUTOFF;
    switch (ctx->feature_chunk ? ctx->feature_chunk : feature_chunk(channels)) {
        case 4u: launch_forward_width<4>(ctx, u, smooth, fs.out, channels, feat, out); break;
        case 8u: launch_forward_width<8>(ctx, u, smooth, fs.out, channels, feat, out); break;
        default: launch_forward_width<16>(ctx, u, smooth, fs.out, channels, feat, out); break;
    }
    BH_LAUNCH_CHECK(ctx, "feature_forward_kernel");
    return 0;
}

// SLOT_FEATURES: compact features [Nv,C] | V [Nv,C] (each padded to a multiple of 64 floats) | the accumulated map [H,W,C]
struct FeatureScratch {
    float* feat = nullptr;
    float* v_feat = nullptr;
    float* acc = nullptr;
    size_t vec_floats = 0;
};

int feature_scratch(bh_ctx* ctx, uint32_t nv, uint32_t channels, size_t pixels, bool backward, FeatureScratch* s) {
    s->vec_floats = splat_vec_floats(nv, channels);
    const size_t floats = backward ? 2 * s->vec_floats + pixels * channels : s->vec_floats;
    auto* base = (float*)ensure(ctx, SLOT_FEATURES, floats * 4);
    if (!base) return BH_ERR_OOM;
    s->feat = base;
    s->v_feat = base + s->vec_floats;
    s->acc = base + 2 * s->vec_floats;
    return 0;
}

int launch_feature_gather(bh_ctx* ctx, const ForwardState& fs, const float* features, uint32_t channels, float* feat) {
    const uint64_t total = (uint64_t)fs.out.num_listed_splats * channels;
    if (total == 0) return 0;
    hipLaunchKernelGGL(feature_gather_kernel, dim3((uint32_t)((total + 255u) / 256u)), dim3(256), 0, ctx->stream, total, channels,
                       fs.out.global_from_compact_gid, features, feat);
    BH_LAUNCH_CHECK(ctx, "feature_gather_kernel");
    return 0;
}

// ---------------------------------------------------------------------------
// losses
// ---------------------------------------------------------------------------
struct FeatureLossArgs {
    uint64_t pixels;
    uint32_t channels;
    float c;   // weight / (H W C) or weight / (H W), rounded once on the host
};

// A pixel per lane; its C values are read twice (L1: validity, then the terms; cross-entropy: the max, then the sum), and a third
// time, from cache, where the cross-entropy gradient is wanted (the softmax needs the finished sum).  brush_hip_features.h states
// the arithmetic.
template <uint32_t KIND, bool GRAD>
__global__ __launch_bounds__(DL_WG) void feature_loss_kernel(FeatureLossArgs a, const float* __restrict__ map, const void* __restrict__ target,
                                                             float* __restrict__ v_map, double* __restrict__ partials) {
    __shared__ double wave_rows[DL_WAVES][DL_ROW];
    double s[2] = {0.0, 0.0};
    const uint32_t C = a.channels;
    const uint64_t stride = (uint64_t)gridDim.x * DL_WG;
    for (uint64_t p = (uint64_t)blockIdx.x * DL_WG + threadIdx.x; p < a.pixels; p += stride) {
        const float* F = map + p * C;
        float* v = GRAD ? v_map + p * C : nullptr;
        bool valid;
        if (KIND == BH_FEATURE_LOSS_L1) {
            const float* t = static_cast<const float*>(target) + p * C;
            valid = true;
            for (uint32_t c = 0; c < C; ++c) valid = valid && is_finite_f32(t[c]);
            if (valid) {
                double l = 0.0;
                for (uint32_t c = 0; c < C; ++c) {
                    const float d = F[c] - t[c];
                    l += (double)__builtin_fabsf(d);
                    if (GRAD) v[c] = d > 0.0f ? a.c : (d < 0.0f ? -a.c : 0.0f);
                }
                s[0] += l;
            }
        } else {
            const uint32_t label = static_cast<const uint8_t*>(target)[p];
            valid = label < C;
            if (valid) {
                float m = F[0];
                for (uint32_t c = 1; c < C; ++c) m = __builtin_fmaxf(m, F[c]);
                const double md = (double)m;
                double sum = 0.0;
                for (uint32_t c = 0; c < C; ++c) sum += exp((double)F[c] - md);
                s[0] += log(sum) + (md - (double)F[label]);
                if (GRAD) {
                    for (uint32_t c = 0; c < C; ++c) {
                        const double e = exp((double)F[c] - md);
                        v[c] = a.c * (float)(e / sum - (c == label ? 1.0 : 0.0));
                    }
                }
            }
        }
        if (valid) s[1] += 1.0;
        else if (GRAD)
            for (uint32_t c = 0; c < C; ++c) v[c] = 0.0f;
    }
    dl_block_store<2>(s, wave_rows, partials);
}

}  // namespace

// The feature term of a backward, between K17 and K18: v_combined += its raw sums, the compact V = sum of w g is left in
// SLOT_FEATURES for launch_feature_scatter; the dense v_features is cleared here.
int launch_feature_backward(bh_ctx* ctx, const ForwardState& fs, const FeatureTerm& term, float* v_combined, const float** v_compact) {
    const BhRenderOut& r = fs.out;
    const uint32_t nv = r.num_listed_splats, C = term.channels;
    const MapUniforms u = map_uniforms(ctx, fs.uniforms);
    FeatureScratch s;
    BH_TRY(feature_scratch(ctx, nv, C, (size_t)u.img_w * u.img_h, /*backward=*/true, &s));
    *v_compact = s.v_feat;
    if (fs.n > 0) BH_HIP(ctx, hipMemsetAsync(term.v_features, 0, (size_t)fs.n * C * 4, ctx->stream));
    BH_HIP(ctx, hipMemsetAsync(s.v_feat, 0, s.vec_floats * 4, ctx->stream));
    if (r.num_intersections == 0 || nv == 0 || u.num_tiles == 0) return 0;
    BH_TRY(launch_feature_gather(ctx, fs, term.features, C, s.feat));
    BH_TRY(launch_feature_forward(ctx, fs, C, s.feat, s.acc));
    const bool smooth = fs.flags & BH_FLAG_SMOOTH_CUTOFF;
    switch (ctx->feature_chunk ? ctx->feature_chunk : feature_chunk(C)) {
        case 4u: launch_backward_width<4>(ctx, u, smooth, r, C, s.feat, s.acc, term.v_map, v_combined, s.v_feat); break;
        case 8u: launch_backward_width<8>(ctx, u, smooth, r, C, s.feat, s.acc, term.v_map, v_combined, s.v_feat); break;
        default: launch_backward_width<16>(ctx, u, smooth, r, C, s.feat, s.acc, term.v_map, v_combined, s.v_feat); break;
    }
    BH_LAUNCH_CHECK(ctx, "feature_backward_kernel");
    return 0;
}

// compact V -> the rows of the dense v_features launch_feature_backward cleared, behind K18
int launch_feature_scatter(bh_ctx* ctx, const ForwardState& fs, const FeatureTerm& term, const float* v_compact) {
    const BhRenderOut& r = fs.out;
    const uint64_t total = (uint64_t)r.num_listed_splats * term.channels;
    if (total == 0 || r.num_intersections == 0) return 0;
    hipLaunchKernelGGL(feature_scatter_kernel, dim3((uint32_t)((total + 255u) / 256u)), dim3(256), 0, ctx->stream, total, term.channels,
                       r.global_from_compact_gid, v_compact, term.v_features);
    BH_LAUNCH_CHECK(ctx, "feature_scatter_kernel");
    return 0;
}

}  // namespace bh

using namespace bh;

extern "C" {

int bh_render_features(bh_ctx* ctx, const BhRenderOut* saved, const float* features, uint32_t channels, float* out) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!saved || !features || !out) return set_error(ctx, BH_ERR_INVALID_ARG, "render_features: null argument");
    if (channels == 0 || channels > BH_FEATURE_MAX_CHANNELS) return set_error(ctx, BH_ERR_INVALID_ARG, "render_features: channels must be 1 .. 256");
    const ForwardState* found = nullptr;
    BH_TRY(find_saved_bwd_forward(ctx, saved, BH_ERR_INVALID_ARG, "render_features", &found));
    const ForwardState& fs = *found;
    if (fs.out.num_intersections == 0 || fs.out.num_listed_splats == 0) return clear_map_window(ctx, fs.uniforms, out, channels);
    ProfScope ps(ctx, "RenderFeatures");
    FeatureScratch s;
    BH_TRY(feature_scratch(ctx, fs.out.num_listed_splats, channels, 0, /*backward=*/false, &s));
    BH_TRY(launch_feature_gather(ctx, fs, features, channels, s.feat));
    return launch_feature_forward(ctx, fs, channels, s.feat, out);
}

int bh_render_backward_features_saved(bh_ctx* ctx, const BhRenderOut* saved, const float* v_output, const float* features, uint32_t channels,
                                      const float* v_map, const float* transforms, const float* sh_coeffs, const float* raw_opacities,
                                      float* v_transforms, float* v_sh_coeffs, float* v_raw_opacities, float* v_refine_weight, float* v_features) {
    FeatureTerm term;
    term.features = features;
    term.channels = channels;
    term.v_map = v_map;
    term.v_features = v_features;
    BackwardCall call{transforms, sh_coeffs, raw_opacities, v_transforms, v_sh_coeffs, v_raw_opacities, v_refine_weight};
    call.feature = &term;
    return backward_entry(ctx, "render_backward_features_saved", BH_ERR_INVALID_ARG, NEED_V_FEATURES, saved, v_output, call);
}

int bh_feature_loss_value_and_grad(bh_ctx* ctx, const float* map, const BhFeatureTarget* target, float* loss, float* v_map) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    const char* who = "feature_loss_value_and_grad";
    if (!map || !loss || !target || !target->target) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": null argument");
    if (target->h == 0 || target->w == 0) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": a feature map of zero size");
    if (target->channels == 0 || target->channels > BH_FEATURE_MAX_CHANNELS)
        return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": channels must be 1 .. 256");
    if (target->kind > BH_FEATURE_LOSS_CROSS_ENTROPY) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": unknown feature loss kind");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    FeatureLossArgs a;
    a.pixels = (uint64_t)target->h * target->w;
    a.channels = target->channels;
    if (!(target->weight > 0.0f)) {   // no term: all +0, nothing is read
        BH_HIP(ctx, hipMemsetAsync(loss, 0, 8, ctx->stream));
        if (v_map) BH_HIP(ctx, hipMemsetAsync(v_map, 0, (size_t)a.pixels * a.channels * 4, ctx->stream));
        return 0;
    }
    const double count = target->kind == BH_FEATURE_LOSS_L1 ? (double)a.pixels * (double)a.channels : (double)a.pixels;
    a.c = (float)((double)target->weight / count);
    uint32_t blocks = 0;
    double* partials = loss_partials(ctx, a.pixels, &blocks);
    if (!partials) return BH_ERR_OOM;
    ProfScope ps(ctx, "FeatureLoss");
    const dim3 grid(blocks), block(DL_WG);
#define BH_FL(K, G) hipLaunchKernelGGL((feature_loss_kernel<K, G>), grid, block, 0, ctx->stream, a, map, target->target, v_map, partials)
    if (target->kind == BH_FEATURE_LOSS_L1) { if (v_map) BH_FL(BH_FEATURE_LOSS_L1, true); else BH_FL(BH_FEATURE_LOSS_L1, false); }
    else { if (v_map) BH_FL(BH_FEATURE_LOSS_CROSS_ENTROPY, true); else BH_FL(BH_FEATURE_LOSS_CROSS_ENTROPY, false); }
#undef BH_FL
    BH_LAUNCH_CHECK(ctx, "feature_loss_kernel");
    return launch_loss_pair_final(ctx, grid.x, partials, a.c, loss, nullptr, nullptr);
}

}  // extern "C"
