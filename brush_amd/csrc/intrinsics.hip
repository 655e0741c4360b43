// intrinsics.hip — brush_hip_intrinsics.h: the intrinsics pass behind K18 (and the pose pass of project.hip, whose per-splat chain it
// repeats as far as the gradient with respect to the 2-D covariance), the backward entries that run it, and the train step's attachment.
// bh_camera_set_intrinsics is next to bh_camera_setup_model in api.hip.
#include "../../include/brush_hip_intrinsics.h"
#include "context.h"
#include "device_camera.h"
#include "device_f64_sum.h"

namespace bh {

namespace {

// With mean2d = f (.) d(mean_c) + c and J = diag(fx, fy) J' (d, J' free of the intrinsics; the clamp limits are constants), the raw
// covariance is A00 = fx^2 a00, A01 = fx fy a01, A11 = fy^2 a11 and the blur adds a constant, so a splat contributes
//   v_fx = g0 xd + 2 (G00 A00 + G01 A01) / fx      v_fy = g1 yd + 2 (G11 A11 + G01 A01) / fy      v_cx = g0      v_cy = g1
// with G = inverse2x2_vjp's full symmetric matrix (G01 stands for both off-diagonal positions: A01 receives 2 G01).  (xd, yd) is
// the lens law evaluated with unit focals and a zero centre: fx xd + cx with fx = 1, cx = 0 is xd to the bit.
// The rows of v_combined are RasterizeGrads here (K18 has run); a row whose five geometry entries are zero gives zero.  The four f32
// contributions are widened to f64 and summed as the pose pass sums its twelve (device_f64_sum.h).
constexpr int INTR_WG = 256;
constexpr int INTR_WAVES = INTR_WG / 64;
constexpr int INTR_FINAL_CHUNKS = 256;

template <bool PINHOLE>
__global__ __launch_bounds__(INTR_WG) void intrinsics_grad_kernel(ViewUniforms u, uint32_t nv, bool mip, const float* __restrict__ transforms,
                                                                  const uint32_t* __restrict__ global_from_compact_gid,
                                                                  const float* __restrict__ v_combined, double* __restrict__ partials) {
    __shared__ double wave_rows[INTR_WAVES][4];
    const uint32_t cg = blockIdx.x * INTR_WG + threadIdx.x;
    float c[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float g[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    bool any = false;
    if (cg < nv) {
        const float* rg = v_combined + (size_t)cg * 10;
#pragma unroll
        for (int k = 0; k < 5; ++k) { g[k] = rg[k]; any = any || (g[k] != 0.0f); }
    }
    if (any) {
        const uint32_t gid = global_from_compact_gid[cg];
        float tr[10];
        {
            const float* trp = transforms + (size_t)gid * 10;
#pragma unroll
            for (int k = 0; k < 10; ++k) tr[k] = trp[k];
        }
        const Vec3A mean = v3(tr[0], tr[1], tr[2]);
        const Vec3A scl = v3(bh_expf(tr[7]), bh_expf(tr[8]), bh_expf(tr[9]));
        const Quat q = qnormalize(Quat{tr[3], tr[4], tr[5], tr[6]});
        const Vec3A mean_c = world_to_cam(mean, u);
        const Sym2 raw_cov = calc_cov2d<PINHOLE>(scl, q, mean_c, u);
        float filter_comp;
        const Sym2 cov = mip ? compensate_cov2d<true>(raw_cov, filter_comp) : compensate_cov2d<false>(raw_cov, filter_comp);
        const Sym2 conic_inv = sym2_inverse(cov);
        const Sym2 v_cov2d = inverse2x2_vjp(conic_inv, Sym2{g[2], g[3] * 0.5f, g[4]});
        ViewUniforms unit = u;
        unit.fx = 1.0f; unit.fy = 1.0f; unit.cx = 0.0f; unit.cy = 0.0f;
        float xd, yd;
        project_point<PINHOLE>(mean_c, unit, xd, yd);
        const float cross = v_cov2d.c01 * raw_cov.c01;
        c[0] = g[0] * xd + 2.0f * (v_cov2d.c00 * raw_cov.c00 + cross) / u.fx;
        c[1] = g[1] * yd + 2.0f * (v_cov2d.c11 * raw_cov.c11 + cross) / u.fy;
        c[2] = g[0];
        c[3] = g[1];
    }
    double s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = (double)c[k];
    dl_block_store<4, 4, INTR_WAVES>(s, wave_rows, partials);
}

// one block: the rows' four totals (dl_final_rows with 256 runs of 4)
__global__ __launch_bounds__(INTR_FINAL_CHUNKS * 4) void intrinsics_grad_final_kernel(uint32_t rows, const double* __restrict__ partials,
                                                                                     float* __restrict__ v_intrinsics) {
    __shared__ double runs[INTR_FINAL_CHUNKS][4];
    const double total = dl_final_rows<4, INTR_FINAL_CHUNKS, 8>(rows, partials, runs);
    if (threadIdx.x < 4) v_intrinsics[threadIdx.x] = (float)total;
}

}  // namespace

int launch_intrinsics_grad(bh_ctx* ctx, const ViewUniforms& u, uint32_t nv, bool mip, const float* transforms, const uint32_t* gid,
                           const float* v_combined, float* v_intrinsics) {
    if (nv == 0) {   // an empty view: four zeros
        BH_HIP(ctx, hipMemsetAsync(v_intrinsics, 0, 4 * 4, ctx->stream));
        return 0;
    }
    const uint32_t rows = (nv + INTR_WG - 1) / INTR_WG;
    auto* partials = (double*)ensure(ctx, SLOT_INTRINSICS, (size_t)rows * 4 * 8);
    if (!partials) return BH_ERR_OOM;
    const dim3 grid(rows), block(INTR_WG);
    if (u.model == CAM_PINHOLE) hipLaunchKernelGGL(intrinsics_grad_kernel<true>, grid, block, 0, ctx->stream, u, nv, mip, transforms, gid, v_combined, partials);
    else hipLaunchKernelGGL(intrinsics_grad_kernel<false>, grid, block, 0, ctx->stream, u, nv, mip, transforms, gid, v_combined, partials);
    BH_LAUNCH_CHECK(ctx, "intrinsics_grad_kernel");
    hipLaunchKernelGGL(intrinsics_grad_final_kernel, dim3(1), dim3(INTR_FINAL_CHUNKS * 4), 0, ctx->stream, rows, partials, v_intrinsics);
    BH_LAUNCH_CHECK(ctx, "intrinsics_grad_final_kernel");
    return 0;
}

}  // namespace bh

extern "C" {

int bh_render_backward_intrinsics_saved(bh_ctx* ctx, const BhRenderOut* saved, const float* v_output, const float* transforms,
                                        const float* sh_coeffs, const float* raw_opacities, float* v_transforms, float* v_sh_coeffs,
                                        float* v_raw_opacities, float* v_refine_weight, float* v_viewmat, float* v_intrinsics) {
    bh::BackwardCall call{transforms, sh_coeffs, raw_opacities, v_transforms, v_sh_coeffs, v_raw_opacities, v_refine_weight};
    call.v_viewmat = v_viewmat;
    call.v_intrinsics = v_intrinsics;
    return bh::backward_entry(ctx, "render_backward_intrinsics_saved", BH_ERR_STATE, bh::NEED_V_OUTPUT | bh::NEED_V_INTRINSICS, saved, v_output, call);
}

int bh_render_backward_camera_saved(bh_ctx* ctx, const BhRenderOut* saved, const float* v_output, const BhCameraGradTerms* terms,
                                    const float* transforms, const float* sh_coeffs, const float* raw_opacities, float* v_transforms,
                                    float* v_sh_coeffs, float* v_raw_opacities, float* v_refine_weight, float* v_viewmat, float* v_intrinsics) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    const bool any_term = terms && (terms->v_depth || terms->v_normal || terms->v_distortion);
    if (!any_term)
        return bh_render_backward_intrinsics_saved(ctx, saved, v_output, transforms, sh_coeffs, raw_opacities, v_transforms, v_sh_coeffs, v_raw_opacities,
                                                   v_refine_weight, v_viewmat, v_intrinsics);
    if (v_viewmat)
        return bh::set_error(ctx, BH_ERR_INVALID_ARG, "render_backward_camera_saved: the pose gradient is that of the colour term alone (v_viewmat must be NULL with a depth, normal or distortion cotangent)");
    bh::DepthTerm depth;
    depth.v_depth = terms->v_depth;
    depth.mode = terms->depth_mode;
    bh::NormalTerm normal;
    normal.v_normal = terms->v_normal;
    normal.mode = terms->normal_mode;
    bh::DistortionTerm dist;
    dist.kind = terms->distortion.kind;
    dist.near_z = terms->distortion.near_z;
    dist.far_z = terms->distortion.far_z;
    dist.v_distortion = terms->v_distortion;
    bh::BackwardCall call{transforms, sh_coeffs, raw_opacities, v_transforms, v_sh_coeffs, v_raw_opacities, v_refine_weight};
    call.depth = &depth;
    call.normal = &normal;
    call.distortion = &dist;
    call.v_intrinsics = v_intrinsics;
    return bh::backward_entry(ctx, "render_backward_camera_saved", BH_ERR_STATE, bh::NEED_V_INTRINSICS, saved, v_output, call);
}

int bh_train_set_intrinsics_grad(bh_ctx* ctx, float* v_intrinsics) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    ctx->terms.intrinsics_grad = v_intrinsics;
    return 0;
}

}  // extern "C"
