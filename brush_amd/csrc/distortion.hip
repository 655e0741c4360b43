// distortion.hip — distortion maps of a rendered frame, their gradient, the loss and the train step's term
// (include/brush_hip_distortion.h).
//
// A distortion map is one more blend over the lists a BH_FLAG_BWD_INFO forward saved, as depth and normal maps are: the same splats in
// the same order with the colour blend's own weights (device_blend.h), on device_map_blend.h's map_forward_kernel /
// map_backward_kernel.  DistortionMap below is what it adds to them.
//
//   dist = sum_i sum_{j<i} w_i w_j (m_i - m_j)^2 = A M2 - M1^2,   A = sum w_i, M1 = sum w_i m_i, M2 = sum w_i m_i^2
//
//   * the per-splat depth m: BH_DISTORTION_Z stages z itself (BhRenderOut.depths_sorted).  BH_DISTORTION_NDC stages
//     m' = -far near / ((far - near) z) from a compact [Nv] vector a one-thread-per-splat kernel fills: 2DGS's
//     m = far (z - near) / ((far - near) z) without its constant far / (far - near), which no difference m_i - m_j sees and which would
//     only cost m' its leading bits.  dm/dz = far near / ((far - near) z^2) is a factor of the splat alone, so it is applied once per
//     splat behind the replay, not per pair: the staged record is the depth map's 8 floats for both kinds.
//   * forward: the sums are folded over d_i = m_i - r, r = the m of the pixel's FIRST contributing splat (dist is invariant under the
//     shift; unshifted f32 sums lose the spread to cancellation at large z, §6o has the figures).  "First" is explicit state, a fourth
//     accumulator that goes from 0 to 1, never a test of T == 1 (under the smooth cut-off a contributor can leave T at 1.0).  Two fmas
//     per contributing pair more than accumulated depth.  Two store modes: dist [H,W], or the moments { A, M1', M2', r } [H,W,4].
//     No atomics: two calls give the same bits.
//   * backward: a moment forward into scratch (or the caller's moment map: the train step's) precedes the replay.  The "colour" of
//     splat i at the pixel is cv_i = g (d_i^2 A + M2' - 2 d_i M1'), the remaining sum starts at S = 2 g dist, and the V sum's factor is
//     the per-(splat, pixel) g 2 (d_i A - M1') through the skeleton's vg hook — all on the shifted quantities, never rebuilt from
//     unshifted sums.  P Q R2 R3 R4 Vs join the [Nv,10] accumulator between K17 and K18 in depth's columns; v_m goes to a compact
//     vector, is multiplied by dm/dz and lands in the depth term's v_z when a depth term runs in the same backward (one scatter
//     serves both: depth.hip's, marking variant included) or in a v_z of its own.
//   * loss: weight * sum(dist) / (H W), f64 partial rows in a fixed order (device_f64_sum.h), the final block of depth_loss.hip.
#include "context.h"
#include "device_map_blend.h"
#include "device_f64_sum.h"
#include "../../include/brush_hip_distortion.h"

namespace bh {

namespace {

// What a distortion map adds to the map skeleton.  MOMENTS: the store writes { A, M1', M2', r } instead of dist.
template <bool MOMENTS>
struct DistortionMap : SinglePassMap<1> {
    static constexpr int STRIDE = 8, NACC = 4;   // acc: r, M1', M2', seen (0 until the pixel's first contributor)
    struct Rec { float4 s0, s1; };   // x y c00/2 c01 | c11/2 a m sigma_cut
    static BH_DEV Rec load(const float* p) { return Rec{*reinterpret_cast<const float4*>(p), *reinterpret_cast<const float4*>(p + 4)}; }
    static BH_DEV float cut(const Rec& r) { return r.s1.w; }
    static BH_DEV void stage(float4* d, const float* v, float sigma_cut, Attr m_of, uint32_t cg) {
        const float m = m_of[cg];
        d[0] = make_float4(v[0], v[1], 0.5f * v[2], v[3]);
        d[1] = make_float4(0.5f * v[4], v[5], m, sigma_cut);
    }
    static BH_DEV void fold(const Rec& r, bool ok, bool sat, float alpha_eff, float next_t, float& T, float* acc) {
        const bool contrib = ok && !sat;
        const float vis = contrib ? alpha_eff * T : 0.0f;
        const bool first = contrib && acc[3] == 0.0f;
        acc[0] = first ? r.s1.z : acc[0];
        acc[3] = contrib ? 1.0f : acc[3];
        const float d = r.s1.z - acc[0];   // (0 for the first contributor; vis == 0 for a splat that does not contribute)
        acc[1] = __builtin_fmaf(vis, d, acc[1]);
        acc[2] = __builtin_fmaf(vis * d, d, acc[2]);
        T = ok ? (sat ? -T : next_t) : T;
    }
    static BH_DEV void store(float* __restrict__ out, Attr, size_t pix, const float* acc, float T) {
        const float a = 1.0f - __builtin_fabsf(T);   // the colour image's alpha, bit for bit (rasterize.hip store_pixels)
        if (MOMENTS) reinterpret_cast<float4*>(out)[pix] = make_float4(a, acc[1], acc[2], acc[0]);
        else out[pix] = __builtin_fmaf(a, acc[2], -(acc[1] * acc[1]));
    }

    struct BwdMaps {
        const float* __restrict__ moments;        // [H,W,4] A M1' M2' r
        const float* __restrict__ v_distortion;   // [H,W], or NULL: the uniform gain
        float gain;
    };
    struct Pix { float g[1] = {0.0f}, a = 0.0f, m1 = 0.0f, m2 = 0.0f, r = 0.0f; };
    static BH_DEV float prologue(const BwdMaps& m, size_t pix, Pix& px) {
        const float4 mo = reinterpret_cast<const float4*>(m.moments)[pix];
        px.g[0] = m.v_distortion ? m.v_distortion[pix] : m.gain;
        px.a = mo.x; px.m1 = mo.y; px.m2 = mo.z; px.r = mo.w;
        return 2.0f * px.g[0] * __builtin_fmaf(mo.x, mo.z, -(mo.y * mo.y));
    }
    static BH_DEV float cv(const Rec& r, const Pix& px) {
        const float d = r.s1.z - px.r;
        return px.g[0] * __builtin_fmaf(d, __builtin_fmaf(d, px.a, -2.0f * px.m1), px.m2);
    }
    static BH_DEV float vg(const Rec& r, const Pix& px, int) {
        const float d = r.s1.z - px.r;
        return 2.0f * px.g[0] * __builtin_fmaf(d, px.a, -px.m1);
    }
};

// BH_DISTORTION_NDC: c = far near / (far - near), rounded once on the host
__global__ __launch_bounds__(256) void distortion_ndc_depth_kernel(uint32_t nv, float c, const float* __restrict__ z, float* __restrict__ m) {
    const uint32_t cg = blockIdx.x * 256u + threadIdx.x;
    if (cg >= nv) return;
    m[cg] = -c / z[cg];
}

// v_z = dm/dz * v_m per splat: stored (ADD = false: a v_z of the term's own, in place) or added to the depth term's v_z
template <bool ADD>
__global__ __launch_bounds__(256) void distortion_ndc_chain_kernel(uint32_t nv, float c, const float* __restrict__ z, const float* __restrict__ v_m,
                                                                   float* __restrict__ v_z) {
    const uint32_t cg = blockIdx.x * 256u + threadIdx.x;
    if (cg >= nv) return;
    const float zz = z[cg];
    const float g = v_m[cg] * (c / (zz * zz));
    v_z[cg] = ADD ? v_z[cg] + g : g;
}

template <int CHANNELS>
__global__ __launch_bounds__(DL_WG) void distortion_loss_kernel(uint64_t pixels, const float* __restrict__ map, double* __restrict__ partials) {
    __shared__ double wave_rows[DL_WAVES][DL_ROW];
    double s[2] = {0.0, 0.0};   // sum of dist, pixels
    const uint64_t stride = (uint64_t)gridDim.x * DL_WG;
    for (uint64_t p = (uint64_t)blockIdx.x * DL_WG + threadIdx.x; p < pixels; p += stride) {
        float d;
        if (CHANNELS == 4) {
            const float4 mo = reinterpret_cast<const float4*>(map)[p];
            d = __builtin_fmaf(mo.x, mo.z, -(mo.y * mo.y));
        } else {
            d = map[p];
        }
        s[0] += (double)d;
        s[1] += 1.0;
    }
    dl_block_store<2>(s, wave_rows, partials);
}

float ndc_factor(const DistortionTerm& t) { return (float)((double)t.far_z * (double)t.near_z / ((double)t.far_z - (double)t.near_z)); }

// the per-splat depth the blends stage: depths_sorted itself, or the NDC vector in `scratch_m`
int launch_distortion_depths(bh_ctx* ctx, const ForwardState& fs, const DistortionTerm& t, float* scratch_m, const float** m_of) {
    const uint32_t nv = fs.out.num_listed_splats;
    if (t.kind == BH_DISTORTION_Z) { *m_of = fs.out.depths_sorted; return 0; }
    hipLaunchKernelGGL(distortion_ndc_depth_kernel, dim3((nv + 255u) / 256u), dim3(256), 0, ctx->stream, nv, ndc_factor(t), fs.out.depths_sorted, scratch_m);
    BH_LAUNCH_CHECK(ctx, "distortion_ndc_depth_kernel");
    *m_of = scratch_m;
    return 0;
}

// the blend over the saved lists (something is listed)
int launch_distortion_blend(bh_ctx* ctx, const ForwardState& fs, const float* m_of, bool moments, float* out) {
    const MapUniforms u = map_uniforms(ctx, fs.uniforms);
    if (u.num_tiles == 0) return 0;
    const bool smooth = fs.flags & BH_FLAG_SMOOTH_CUTOFF;
    if (moments) launch_map_forward<DistortionMap<true>>(ctx, u, smooth, fs.out, m_of, out);
    else launch_map_forward<DistortionMap<false>>(ctx, u, smooth, fs.out, m_of, out);
    BH_LAUNCH_CHECK(ctx, "distortion_forward_kernel");
    return 0;
}

}  // namespace

int check_distortion_kind(bh_ctx* ctx, uint32_t kind, float near_z, float far_z, const char* who) {
    if (kind > BH_DISTORTION_NDC) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": unknown distortion kind");
    if (kind == BH_DISTORTION_NDC && !(near_z > 0.0f && far_z > near_z && far_z <= 3.0e38f))
        return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": BH_DISTORTION_NDC needs 0 < near < far");
    return 0;
}

// The distortion map (moments: the moment map) of the saved forward `fs` (something is listed); the NDC depths go through SLOT_DISTORTION.
int launch_distortion_map(bh_ctx* ctx, const ForwardState& fs, const DistortionTerm& t, bool moments, float* out) {
    MapScratch s;
    const float* m_of = nullptr;
    if (t.kind != BH_DISTORTION_Z) BH_TRY(map_scratch(ctx, SLOT_DISTORTION, fs.out.num_listed_splats, 1, /*has_input=*/true, /*backward=*/false, 0, &s));
    BH_TRY(launch_distortion_depths(ctx, fs, t, s.in, &m_of));
    return launch_distortion_blend(ctx, fs, m_of, moments, out);
}

// The distortion term of a backward, between K17 and K18 and behind the depth term's replay: v_combined += its raw sums; its v_z is
// added into *v_z (the depth term's vector, already filled) or, *v_z == NULL, stored in a vector of its own.  *v_z on return: the
// vector the ONE scatter behind K18 reads.
int launch_distortion_backward(bh_ctx* ctx, const ForwardState& fs, const DistortionTerm& t, float* v_combined, float** v_z) {
    const BhRenderOut& r = fs.out;
    const uint32_t nv = r.num_listed_splats;
    const MapUniforms u = map_uniforms(ctx, fs.uniforms);
    const size_t pixels = (size_t)u.img_w * u.img_h;
    // SLOT_DISTORTION: m [Nv] | v_m [Nv] | the frame's moment map [H,W,4] (none where the caller brings its own)
    MapScratch s;
    BH_TRY(map_scratch(ctx, SLOT_DISTORTION, nv, 1, /*has_input=*/true, /*backward=*/true, t.moments ? 0 : pixels * 4, &s));
    float* const depth_v_z = *v_z;
    // Z with a depth term: the replay's atomics go straight into the depth term's v_z; every other case starts from a zeroed v_m
    const bool direct = depth_v_z && t.kind == BH_DISTORTION_Z;
    if (!direct) BH_HIP(ctx, hipMemsetAsync(s.v, 0, s.vec_floats * 4, ctx->stream));
    if (!depth_v_z) *v_z = s.v;
    if (r.num_intersections == 0 || nv == 0 || u.num_tiles == 0) return 0;
    const float* m_of = nullptr;
    BH_TRY(launch_distortion_depths(ctx, fs, t, s.in, &m_of));
    const float* moments = t.moments;
    if (!moments) {
        BH_TRY(launch_distortion_blend(ctx, fs, m_of, /*moments=*/true, s.acc));
        moments = s.acc;
    }
    using P = DistortionMap<true>;
    const P::BwdMaps maps{moments, t.v_distortion, t.gain};
    launch_map_backward<P>(ctx, u, fs.flags & BH_FLAG_SMOOTH_CUTOFF, r, m_of, maps, v_combined, direct ? depth_v_z : s.v);
    BH_LAUNCH_CHECK(ctx, "distortion_backward_kernel");
    if (t.kind == BH_DISTORTION_NDC) {
        const dim3 grid((nv + 255u) / 256u), block(256);
        if (depth_v_z) hipLaunchKernelGGL(distortion_ndc_chain_kernel<true>, grid, block, 0, ctx->stream, nv, ndc_factor(t), r.depths_sorted, s.v, depth_v_z);
        else hipLaunchKernelGGL(distortion_ndc_chain_kernel<false>, grid, block, 0, ctx->stream, nv, ndc_factor(t), r.depths_sorted, s.v, s.v);
        BH_LAUNCH_CHECK(ctx, "distortion_ndc_chain_kernel");
    }
    return 0;
}

// weight * sum(dist) / (H W) of a distortion map (channels == 1) or a moment map (channels == 4); accum as launch_depth_loss's
int launch_distortion_loss(bh_ctx* ctx, const float* map, uint32_t h, uint32_t w, uint32_t channels, float weight, float* loss, float* accum,
                           float* accum_host) {
    const uint64_t pixels = (uint64_t)h * w;
    const float c = (float)((double)weight / (double)pixels);
    uint32_t blocks = 0;
    double* partials = loss_partials(ctx, pixels, &blocks);
    if (!partials) return BH_ERR_OOM;
    const dim3 grid(blocks), block(DL_WG);
    if (channels == 4) hipLaunchKernelGGL(distortion_loss_kernel<4>, grid, block, 0, ctx->stream, pixels, map, partials);
    else hipLaunchKernelGGL(distortion_loss_kernel<1>, grid, block, 0, ctx->stream, pixels, map, partials);
    BH_LAUNCH_CHECK(ctx, "distortion_loss_kernel");
    return launch_loss_pair_final(ctx, grid.x, partials, c, loss, accum, accum_host);
}

}  // namespace bh

using namespace bh;

namespace {

DistortionTerm term_of(const BhDistortionConfig& cfg) {
    DistortionTerm t;
    t.kind = cfg.kind;
    t.near_z = cfg.near_z;
    t.far_z = cfg.far_z;
    return t;
}

int render_distortion(bh_ctx* ctx, const BhRenderOut* saved, const BhDistortionConfig* cfg, float* out, bool moments, const char* who) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!saved || !cfg || !out) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": null argument");
    BH_TRY(check_distortion_kind(ctx, cfg->kind, cfg->near_z, cfg->far_z, who));
    const ForwardState* found = nullptr;
    BH_TRY(find_saved_bwd_forward(ctx, saved, BH_ERR_INVALID_ARG, who, &found));
    const ForwardState& fs = *found;
    if (fs.out.num_intersections == 0 || fs.out.num_listed_splats == 0) return clear_map_window(ctx, fs.uniforms, out, moments ? 4 : 1);
    ProfScope ps(ctx, "RenderDistortion");
    return launch_distortion_map(ctx, fs, term_of(*cfg), moments, out);
}

}  // namespace

extern "C" {

int bh_render_distortion(bh_ctx* ctx, const BhRenderOut* saved, const BhDistortionConfig* cfg, float* out) {
    return render_distortion(ctx, saved, cfg, out, /*moments=*/false, "render_distortion");
}

int bh_render_distortion_moments(bh_ctx* ctx, const BhRenderOut* saved, const BhDistortionConfig* cfg, float* out) {
    return render_distortion(ctx, saved, cfg, out, /*moments=*/true, "render_distortion_moments");
}

int bh_render_backward_distortion_saved(bh_ctx* ctx, const BhRenderOut* saved, const float* v_output, const float* v_depth, uint32_t depth_mode,
                                        const float* v_normal, uint32_t normal_mode, const float* v_distortion, const BhDistortionConfig* cfg,
                                        const float* transforms, const float* sh_coeffs, const float* raw_opacities, float* v_transforms,
                                        float* v_sh_coeffs, float* v_raw_opacities, float* v_refine_weight) {
    DepthTerm depth;
    depth.v_depth = v_depth;
    depth.mode = depth_mode;
    NormalTerm normal;
    normal.v_normal = v_normal;
    normal.mode = normal_mode;
    DistortionTerm dist = cfg ? term_of(*cfg) : DistortionTerm{};
    dist.v_distortion = v_distortion;
    BackwardCall call{transforms, sh_coeffs, raw_opacities, v_transforms, v_sh_coeffs, v_raw_opacities, v_refine_weight};
    call.depth = &depth;
    call.normal = &normal;
    call.distortion = cfg ? &dist : nullptr;   // (no configuration: no term, and the term is required)
    return backward_entry(ctx, "render_backward_distortion_saved", BH_ERR_INVALID_ARG, NEED_V_DISTORTION, saved, v_output, call);
}

int bh_distortion_loss(bh_ctx* ctx, const float* map, uint32_t h, uint32_t w, uint32_t channels, float weight, float* loss) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!map || !loss) return set_error(ctx, BH_ERR_INVALID_ARG, "distortion_loss: null argument");
    if (h == 0 || w == 0) return set_error(ctx, BH_ERR_INVALID_ARG, "distortion_loss: a map of zero size");
    if ((uint64_t)h * w > 0x7FFFFFFFull) return set_error(ctx, BH_ERR_INVALID_ARG, "distortion_loss: more than 2^31 - 1 pixels");
    if (channels != 1u && channels != 4u) return set_error(ctx, BH_ERR_INVALID_ARG, "distortion_loss: channels must be 1 (a distortion map) or 4 (a moment map)");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    if (!(weight > 0.0f)) {   // no term: all +0, no pixel is looked at
        BH_HIP(ctx, hipMemsetAsync(loss, 0, 8, ctx->stream));
        return 0;
    }
    ProfScope ps(ctx, "DistortionLoss");
    return launch_distortion_loss(ctx, map, h, w, channels, weight, loss, nullptr, nullptr);
}

int bh_train_set_distortion(bh_ctx* ctx, const BhDistortionTermConfig* cfg) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    const bool on = cfg != nullptr && cfg->weight > 0.0f;   // (a NaN weight compares false: no term)
    if (on) BH_TRY(check_distortion_kind(ctx, cfg->kind, cfg->near_z, cfg->far_z, "train_set_distortion"));
    ctx->terms.distortion_attached = on;
    ctx->terms.distortion_term = on ? *cfg : BhDistortionTermConfig{};
    return 0;
}

}  // extern "C"
