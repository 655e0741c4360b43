// depth.hip — depth maps of a rendered frame and their gradient (include/brush_hip_depth.h).
//
// A depth map is a second blend over the lists a BH_FLAG_BWD_INFO forward saved: the same splats in the same order with the same
// alpha, cut-off, clamp and saturation rule as the colour blend (device_blend.h holds the one copy of that arithmetic), folding the
// camera-space z of each splat (BhRenderOut.depths_sorted) where K16 folds its colour.  The tuned colour kernels K16 / K17 are not
// touched: a frame that asks for no depth pays nothing.  The blend and the replay themselves are device_map_blend.h's
// map_forward_kernel / map_backward_kernel, shared with normal.hip; this file holds what a depth map adds to them (DepthMap).
//
//   * forward: a staged splat is 8 floats (32 B: x y c00/2 c01 | c11/2 alpha0 z sigma_cut), two uniform ds_read_b128 per splat where
//     K16 reads 40 bytes, and one fma per contributing pair where K16 does three.  Median mode marks a pixel done as soon as its
//     transmittance has crossed 1/2, so its tiles end earlier still.
//   * backward (accumulated and expected depth): the "remaining" sum S needs the pixel's total, which is the accumulated depth map:
//     a forward pass into scratch precedes the replay.  The RAW sums P Q R2 R3 R4 Vs are added to the [Nv,10] accumulator K17 fills
//     (project.hip maps them once per splat), and v_z = sum of v_D * w to a per-splat vector of its own, which a small kernel behind
//     K18 carries to the means.
#include "context.h"
#include "device_map_blend.h"
#include "../../include/brush_hip_depth.h"

namespace bh {

namespace {

// What a depth map adds to the map skeleton.  MODE: BH_DEPTH_ACCUMULATED / EXPECTED / MEDIAN (the backward does not read it).
//
// Backward.  Expected depth E = D / A with A = sum of w: dE = (1/A) sum of dw_i (z_i - E) + (1/A) sum of w_i dz_i.  So both modes are
// ONE replay with a per-pixel gain g and offset e: the "colour" of splat i at the pixel is z_i - e and the pixel's cotangent is g
// (accumulated: g = v_D, e = 0; expected: g = v_D / A, e = E, 0 where A == 0) — the chain through 1/A, which is a gradient on the
// alpha channel, is the offset.  S = g * (remaining sum of w_j (z_j - e)).
template <uint32_t MODE>
struct DepthMap : SinglePassMap<1> {
    static constexpr int STRIDE = 8, NACC = 1;
    struct Rec { float4 s0, s1; };   // x y c00/2 c01 | c11/2 a z sigma_cut
    static BH_DEV Rec load(const float* p) { return Rec{*reinterpret_cast<const float4*>(p), *reinterpret_cast<const float4*>(p + 4)}; }
    static BH_DEV float cut(const Rec& r) { return r.s1.w; }
    static BH_DEV void stage(float4* d, const float* v, float sigma_cut, Attr depths, uint32_t cg) {
        const float z = depths[cg];
        d[0] = make_float4(v[0], v[1], 0.5f * v[2], v[3]);
        d[1] = make_float4(0.5f * v[4], v[5], z, sigma_cut);
    }
    static BH_DEV void fold(const Rec& r, bool ok, bool sat, float alpha_eff, float next_t, float& T, float* acc) {
        const bool contrib = ok && !sat;
        if (MODE == BH_DEPTH_MEDIAN) {
            // T is monotone: it FIRST becomes <= 1/2 at the one contributing splat that finds it above and leaves it at or
            // below.  Nothing behind that splat matters to the median: the pixel is done.
            const bool hit = contrib && T > 0.5f && next_t <= 0.5f;
            acc[0] = hit ? r.s1.z : acc[0];
            T = ok ? ((sat || hit) ? -T : next_t) : T;
        } else {
            const float vis = contrib ? alpha_eff * T : 0.0f;
            acc[0] = __builtin_fmaf(r.s1.z, vis, acc[0]);   // (one explicit fma per term, as the colour channels)
            T = ok ? (sat ? -T : next_t) : T;
        }
    }
    static BH_DEV void store(float* __restrict__ out, Attr, size_t pix, const float* acc, float T) {
        float v = acc[0];
        if (MODE == BH_DEPTH_EXPECTED) {
            const float a = 1.0f - __builtin_fabsf(T);   // the colour image's alpha, bit for bit (rasterize.hip store_pixels)
            v = a == 0.0f ? 0.0f : v / a;
        }
        out[pix] = v;
    }

    struct BwdMaps {
        const float* __restrict__ out_img;     // [H,W,4] the frame's colour image (its alpha)
        const float* __restrict__ depth_acc;   // [H,W] the frame's accumulated depth
        const float* __restrict__ v_depth;     // [H,W]
        uint32_t expected;
    };
    struct Pix { float g[1] = {0.0f}, e = 0.0f; };
    static BH_DEV float prologue(const BwdMaps& m, size_t pix, Pix& px) {
        const float a = m.out_img[pix * 4 + 3], d = m.depth_acc[pix], v = m.v_depth[pix];
        if (m.expected) {
            const bool has = a > 0.0f;
            px.g[0] = has ? v / a : 0.0f;
            px.e = has ? d / a : 0.0f;
        } else {
            px.g[0] = v;
        }
        return px.g[0] * __builtin_fmaf(-px.e, a, d);
    }
    static BH_DEV float cv(const Rec& r, const Pix& px) { return px.g[0] * (r.s1.z - px.e); }
    static BH_DEV float vg(const Rec&, const Pix& px, int i) { return px.g[i]; }
};

// v_mean += (row 2 of the view matrix) * v_z, behind K18 in its dense mode: a row K18 skipped (its ten sums are zero) is zero in the
// zero-filled dense output.  MARK (behind a K18 in marking mode, the single-GPU train step): K18 skips a splat whose ten sums are
// all zero — one whose every pair sat at the alpha clamp still has a v_z — so the row is claimed first (claim_grad_row).
template <bool MARK>
BH_DEV void vz_scatter_row(uint32_t nv, float r0, float r1, float r2, uint32_t sh_floats, const uint32_t* __restrict__ global_from_compact,
                           const float* __restrict__ v_z, float* __restrict__ v_transforms, float* __restrict__ v_sh, float* __restrict__ v_raw_opac,
                           float* __restrict__ v_refine) {
    const uint32_t cg = blockIdx.x * 256u + threadIdx.x;
    if (cg >= nv) return;
    const float vz = v_z[cg];
    if (vz == 0.0f) return;
    const uint32_t gid = global_from_compact[cg];
    float* vt = v_transforms + (size_t)gid * 10;
    if (MARK) claim_grad_row(gid, sh_floats, vt, v_sh, v_raw_opac, v_refine);
    vt[0] = __builtin_fmaf(r0, vz, vt[0]);
    vt[1] = __builtin_fmaf(r1, vz, vt[1]);
    vt[2] = __builtin_fmaf(r2, vz, vt[2]);
}

__global__ __launch_bounds__(256) void depth_vz_scatter_kernel(uint32_t nv, float r0, float r1, float r2, const uint32_t* __restrict__ global_from_compact,
                                                               const float* __restrict__ v_z, float* __restrict__ v_transforms) {
    vz_scatter_row<false>(nv, r0, r1, r2, 0u, global_from_compact, v_z, v_transforms, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void depth_vz_scatter_marking_kernel(uint32_t nv, float r0, float r1, float r2, uint32_t sh_floats,
                                                                       const uint32_t* __restrict__ global_from_compact, const float* __restrict__ v_z,
                                                                       float* __restrict__ v_transforms, float* __restrict__ v_sh, float* __restrict__ v_raw_opac,
                                                                       float* __restrict__ v_refine) {
    vz_scatter_row<true>(nv, r0, r1, r2, sh_floats, global_from_compact, v_z, v_transforms, v_sh, v_raw_opac, v_refine);
}

}  // namespace

int launch_depth_forward(bh_ctx* ctx, const ForwardState& fs, uint32_t mode, float* out_depth) {
    const BhRenderOut& r = fs.out;
    const MapUniforms u = map_uniforms(ctx, fs.uniforms);
    if (u.num_tiles == 0) return 0;
    const bool smooth = fs.flags & BH_FLAG_SMOOTH_CUTOFF;
    switch (mode) {
        case BH_DEPTH_ACCUMULATED: launch_map_forward<DepthMap<BH_DEPTH_ACCUMULATED>>(ctx, u, smooth, r, r.depths_sorted, out_depth); break;
        case BH_DEPTH_EXPECTED: launch_map_forward<DepthMap<BH_DEPTH_EXPECTED>>(ctx, u, smooth, r, r.depths_sorted, out_depth); break;
        case BH_DEPTH_MEDIAN: launch_map_forward<DepthMap<BH_DEPTH_MEDIAN>>(ctx, u, smooth, r, r.depths_sorted, out_depth); break;
        default: return set_error(ctx, BH_ERR_INVALID_ARG, "render_depth: unknown depth mode");
    }
    BH_LAUNCH_CHECK(ctx, "depth_forward_kernel");
    return 0;
}

// The depth term of a backward, between K17 and K18: v_combined += its raw sums, *v_z_out = v_z = sum of v_D * w.
int launch_depth_backward(bh_ctx* ctx, const ForwardState& fs, const DepthTerm& term, float* v_combined, float** v_z_out) {
    const BhRenderOut& r = fs.out;
    const uint32_t nv = r.num_listed_splats;
    const MapUniforms u = map_uniforms(ctx, fs.uniforms);
    // SLOT_DEPTH: no input vector (depths_sorted is staged as it is) | v_z [Nv] | the frame's accumulated depth [H,W]
    MapScratch s;
    BH_TRY(map_scratch(ctx, SLOT_DEPTH, nv, 1, /*has_input=*/false, /*backward=*/true, (size_t)u.img_w * u.img_h, &s));
    *v_z_out = s.v;
    BH_HIP(ctx, hipMemsetAsync(s.v, 0, s.vec_floats * 4, ctx->stream));
    if (r.num_intersections == 0 || u.num_tiles == 0) return 0;
    BH_TRY(launch_depth_forward(ctx, fs, BH_DEPTH_ACCUMULATED, s.acc));
    using P = DepthMap<BH_DEPTH_ACCUMULATED>;
    const P::BwdMaps maps{r.out_img, s.acc, term.v_depth, term.mode == BH_DEPTH_EXPECTED ? 1u : 0u};
    launch_map_backward<P>(ctx, u, fs.flags & BH_FLAG_SMOOTH_CUTOFF, r, r.depths_sorted, maps, v_combined, s.v);
    BH_LAUNCH_CHECK(ctx, "depth_backward_kernel");
    return 0;
}

int launch_depth_vz_scatter(bh_ctx* ctx, const ForwardState& fs, const float* v_z, float* v_transforms, bool mark_rows, float* v_sh_coeffs,
                            float* v_raw_opacities, float* v_refine_weight) {
    const BhRenderOut& r = fs.out;
    const uint32_t nv = r.num_listed_splats;
    if (nv == 0 || r.num_intersections == 0) return 0;
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
    const bh::ForwardState* found = nullptr;
    BH_TRY(bh::find_saved_bwd_forward(ctx, saved, BH_ERR_INVALID_ARG, "render_depth", &found));
    const bh::ForwardState& fs = *found;
    if (fs.out.num_intersections == 0) return bh::clear_map_window(ctx, fs.uniforms, out_depth, 1);   // nothing listed: every mode is 0
    bh::ProfScope ps(ctx, "RenderDepth");
    return bh::launch_depth_forward(ctx, fs, mode, out_depth);
}

int bh_render_backward_depth_saved(bh_ctx* ctx, const BhRenderOut* saved, const float* v_output, const float* v_depth, uint32_t mode,
                                   const float* transforms, const float* sh_coeffs, const float* raw_opacities, float* v_transforms,
                                   float* v_sh_coeffs, float* v_raw_opacities, float* v_refine_weight) {
    bh::DepthTerm depth;
    depth.v_depth = v_depth;
    depth.mode = mode;
    bh::BackwardCall call{transforms, sh_coeffs, raw_opacities, v_transforms, v_sh_coeffs, v_raw_opacities, v_refine_weight};
    call.depth = &depth;
    return bh::backward_entry(ctx, "render_backward_depth_saved", BH_ERR_INVALID_ARG, bh::NEED_V_DEPTH, saved, v_output, call);
}

}  // extern "C"
