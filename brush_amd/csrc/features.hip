// features.hip — feature maps of a rendered frame: the blend of caller-owned per-splat vectors with any channel count, its
// gradient, and two fused losses on such a map (include/brush_hip_features.h).
//
// A feature map is one more blend over the lists a BH_FLAG_BWD_INFO forward saved, as a depth or a normal map is: the same splats in
// the same order with the same alpha, cut-off, clamp and saturation rule as the colour blend (device_blend.h holds the one copy of
// that arithmetic).  The blend and the replay themselves are device_map_blend.h's map_forward_kernel / map_backward_kernel, shared
// with depth.hip, normal.hip and distortion.hip; FeatureMap<CH> below is what a feature map adds to them.  A process that never
// calls these entry points launches nothing of it.
//
//   * gather: features[global_from_compact_gid[cg], :] -> a compact [Nv,C] array, what the two blends stage (as normals do);
//   * forward: the skeleton once per CHUNK of CH channels (the grid's y: FeatureMap::chunks).  A chunk is one pass over the tile's
//     lists with 8 + CH staged floats per splat and 4 CH accumulators per lane, one explicit fma per channel and term.  CH is a
//     template parameter (4, 8, 16): the trade is passes over the lists against registers, i.e. waves per SIMD; feature_chunk()
//     picks per C;
//   * backward: per chunk the skeleton's replay with g[CH] per pixel in registers: the "colour" of a splat is cv = sum of g_c f_c
//     over the chunk, the remaining sum S starts at sum of g_c F_c (an accumulated-map forward into scratch precedes the replay).
//     v_alpha is linear in cv and S, so every chunk adds its share of P Q R2 R3 R4 Vs to v_combined, between K17 and K18.  The
//     6 + CH per-splat sums leave through the skeleton's butterfly, V by f32 atomics into a compact [Nv,C] (FeatureMap::v_home)
//     that a small kernel behind K18 carries to the dense v_features;
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

// What a feature map adds to the map skeleton: CH channels of the C per pass over the lists, the chunk of a block being
// blockIdx.y.  A staged splat is x y c00/2 c01 | c11/2 alpha0 sigma_cut - | CH features (0 behind the last channel).
//
// Backward.  The "colour" of splat i at the pixel is cv = sum of g_c f_ic over the chunk and S starts at the chunk's share
// sum of g_c F_c of the pixel's remaining sum; V sum i is channel c0 + i of the compact [Nv,C] vector.
template <int CH>
struct FeatureMap {
    static constexpr int STRIDE = 8 + CH, NACC = CH, NV = CH, FWD_WAVES = 1, BWD_WAVES = 1;
    struct Attr {
        const float* __restrict__ feat;   // compact rows [Nv,C]
        uint32_t channels;
    };
    static uint32_t chunks(const Attr& a) { return (a.channels + CH - 1) / CH; }
    struct Rec { float4 s0, s1; float f[CH]; };
    static BH_DEV Rec load(const float* p) {
        Rec r{*reinterpret_cast<const float4*>(p), *reinterpret_cast<const float4*>(p + 4), {}};
#pragma unroll
        for (int i = 0; i < CH / 4; ++i) {
            const float4 x = *reinterpret_cast<const float4*>(p + 8 + 4 * i);
            r.f[4 * i] = x.x; r.f[4 * i + 1] = x.y; r.f[4 * i + 2] = x.z; r.f[4 * i + 3] = x.w;
        }
        return r;
    }
    static BH_DEV float cut(const Rec& r) { return r.s1.z; }
    static BH_DEV void stage(float4* d, const float* v, float sigma_cut, const Attr& a, uint32_t cg) {
        const uint32_t c0 = blockIdx.y * CH;
        d[0] = make_float4(v[0], v[1], 0.5f * v[2], v[3]);
        d[1] = make_float4(0.5f * v[4], v[5], sigma_cut, 0.0f);
        const float* f = a.feat + (size_t)cg * a.channels + c0;
        float x[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) x[i] = c0 + i < a.channels ? f[i] : 0.0f;
#pragma unroll
        for (int i = 0; i < CH / 4; ++i) d[2 + i] = make_float4(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]);
    }
    static BH_DEV void fold(const Rec& r, bool ok, bool sat, float alpha_eff, float next_t, float& T, float* acc) {
        const float vis = (ok && !sat) ? alpha_eff * T : 0.0f;
#pragma unroll
        for (int i = 0; i < CH; ++i) acc[i] = __builtin_fmaf(r.f[i], vis, acc[i]);   // (one explicit fma per channel and term: the contract)
        T = ok ? (sat ? -T : next_t) : T;
    }
    static BH_DEV void store(float* __restrict__ out, const Attr& a, size_t pix, const float* acc, float) {
        const uint32_t c0 = blockIdx.y * CH;
        float* o = out + pix * a.channels + c0;
#pragma unroll
        for (int i = 0; i < CH; ++i)
            if (c0 + i < a.channels) o[i] = acc[i];
    }

    struct BwdMaps {
        const float* __restrict__ map_acc;   // [H,W,C] the frame's accumulated feature map
        const float* __restrict__ v_map;     // [H,W,C]
        uint32_t channels;
    };
    struct Pix { float g[CH] = {}; };
    static BH_DEV float prologue(const BwdMaps& m, size_t pixel, Pix& px) {
        const uint32_t c0 = blockIdx.y * CH;
        const size_t base = pixel * m.channels + c0;
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            if (c0 + i < m.channels) {
                px.g[i] = m.v_map[base + i];
                s = __builtin_fmaf(px.g[i], m.map_acc[base + i], s);
            }
        }
        return s;
    }
    static BH_DEV float cv(const Rec& r, const Pix& px) {
        float cv = 0.0f;
#pragma unroll
        for (int i = 0; i < CH; ++i) cv = __builtin_fmaf(px.g[i], r.f[i], cv);
        return cv;
    }
    static BH_DEV float vg(const Rec&, const Pix& px, int i) { return px.g[i]; }
    static BH_DEV float* v_home(const BwdMaps& m, float* v_attr, uint32_t cg, int i) {
        const uint32_t c = blockIdx.y * CH + (uint32_t)i;
        return c < m.channels ? v_attr + (size_t)cg * m.channels + c : nullptr;
    }
};

// The chunk width for C channels.  One pass over the lists per chunk, so the widest chunk that does not waste most of itself:
// DESIGN.md §6r has the measurement behind the thresholds.
uint32_t feature_chunk(uint32_t channels) { return channels <= 4u ? 4u : (channels <= 8u ? 8u : 16u); }

// runs `f` with the traits struct of the chunk width (option feature_chunk forces one: the probe's, and the tests')
template <class F>
void with_feature_map(const bh_ctx* ctx, uint32_t channels, F&& f) {
    switch (ctx->feature_chunk ? ctx->feature_chunk : feature_chunk(channels)) {
        case 4u: f(FeatureMap<4>{}); break;
        case 8u: f(FeatureMap<8>{}); break;
        default: f(FeatureMap<16>{}); break;
    }
}

}  // namespace

// the blend of the compact rows `feat` into `out`
int launch_feature_forward(bh_ctx* ctx, const ForwardState& fs, uint32_t channels, const float* feat, float* out) {
    const MapUniforms u = map_uniforms(ctx, fs.uniforms);
    if (u.num_tiles == 0) return 0;
    with_feature_map(ctx, channels, [&](auto p) {
        using P = decltype(p);
        launch_map_forward<P>(ctx, u, fs.flags & BH_FLAG_SMOOTH_CUTOFF, fs.out, typename P::Attr{feat, channels}, out);
    });
    BH_LAUNCH_CHECK(ctx, "feature_forward_kernel");
    return 0;
}

namespace {

// SLOT_FEATURES: compact features [Nv,C] | V [Nv,C] | the accumulated map [H,W,C]
int feature_scratch(bh_ctx* ctx, uint32_t nv, uint32_t channels, size_t pixels, bool backward, MapScratch* s) {
    return map_scratch(ctx, SLOT_FEATURES, nv, channels, /*has_input=*/true, backward, pixels * channels, s);
}

}  // namespace

int launch_feature_gather(bh_ctx* ctx, const ForwardState& fs, const float* features, uint32_t channels, float* feat) {
    const uint64_t total = (uint64_t)fs.out.num_listed_splats * channels;
    if (total == 0) return 0;
    hipLaunchKernelGGL(feature_gather_kernel, dim3((uint32_t)((total + 255u) / 256u)), dim3(256), 0, ctx->stream, total, channels,
                       fs.out.global_from_compact_gid, features, feat);
    BH_LAUNCH_CHECK(ctx, "feature_gather_kernel");
    return 0;
}

// the train step's compact rows: where launch_feature_backward will look for them (the slot is sized for that backward here, so
// it does not move in between)
int feature_term_rows(bh_ctx* ctx, const ForwardState& fs, uint32_t channels, float** feat) {
    MapScratch s;
    BH_TRY(feature_scratch(ctx, fs.out.num_listed_splats, channels, 0, /*backward=*/true, &s));
    *feat = s.in;
    return 0;
}

namespace {

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
    const bool rendered = term.map_acc != nullptr;   // the train step: the map and the compact rows exist (feature_term_rows' layout)
    MapScratch s;
    BH_TRY(feature_scratch(ctx, nv, C, rendered ? 0 : (size_t)u.img_w * u.img_h, /*backward=*/true, &s));
    *v_compact = s.v;
    if (fs.n > 0) BH_HIP(ctx, hipMemsetAsync(term.v_features, 0, (size_t)fs.n * C * 4, ctx->stream));
    BH_HIP(ctx, hipMemsetAsync(s.v, 0, s.vec_floats * 4, ctx->stream));
    if (r.num_intersections == 0 || nv == 0 || u.num_tiles == 0) return 0;
    const float* map_acc = term.map_acc;
    if (!rendered) {
        BH_TRY(launch_feature_gather(ctx, fs, term.features, C, s.in));
        BH_TRY(launch_feature_forward(ctx, fs, C, s.in, s.acc));
        map_acc = s.acc;
    } else if (term.compact != s.in) {
        return set_error(ctx, BH_ERR_STATE, "internal: the feature term's compact rows are not where the backward's scratch has them");
    }
    with_feature_map(ctx, C, [&](auto p) {
        using P = decltype(p);
        launch_map_backward<P>(ctx, u, fs.flags & BH_FLAG_SMOOTH_CUTOFF, r, typename P::Attr{s.in, C}, typename P::BwdMaps{map_acc, term.v_map, C}, v_combined, s.v);
    });
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
    MapScratch s;
    BH_TRY(feature_scratch(ctx, fs.out.num_listed_splats, channels, 0, /*backward=*/false, &s));
    BH_TRY(launch_feature_gather(ctx, fs, features, channels, s.in));
    return launch_feature_forward(ctx, fs, channels, s.in, out);
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
    return launch_feature_loss(ctx, map, *target, loss, v_map, nullptr, nullptr);
}

// brush_hip_feature_train.h: the field and the target of the ctx's next train steps (context.h StepTerms; train.hip applies them)
int bh_train_set_features(bh_ctx* ctx, const BhFeatureField* field, const BhFeatureTarget* target) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    const char* who = "train_set_features";
    if (field) {
        if (!field->features || !field->m1 || !field->m2) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": null pointer in the field");
        if (field->channels == 0 || field->channels > BH_FEATURE_MAX_CHANNELS)
            return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": channels must be 1 .. 256");
        if (target) {
            if (target->channels != field->channels) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": the target's channels differ from the field's");
            if (target->kind > BH_FEATURE_LOSS_CROSS_ENTROPY) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": unknown feature loss kind");
            if (target->weight > 0.0f && !target->target) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": the target has no target map");
        }
    }
    ctx->terms.feature_attached = field != nullptr;
    ctx->terms.feature_field = field ? *field : BhFeatureField{};
    ctx->terms.feature_target = (field && target) ? *target : BhFeatureTarget{};
    return 0;
}

}  // extern "C"

namespace bh {

int launch_feature_loss(bh_ctx* ctx, const float* map, const BhFeatureTarget& t, float* loss, float* v_map, float* accum, float* accum_host) {
    const BhFeatureTarget* target = &t;
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
    return launch_loss_pair_final(ctx, grid.x, partials, a.c, loss, accum, accum_host);
}

}  // namespace bh
