/* brush_hip_intrinsics.h — the gradient of a rendered frame with respect to its camera's intrinsics (focal lengths and principal
 * point), and the host arithmetic of an intrinsics update: an operator over the state a BH_FLAG_BWD_INFO forward saved, next to the
 * pose gradient of brush_hip_pose.h.  DESIGN.md §6w has the whole contract.
 *
 * Same conventions as brush_hip.h: 0 on success, <0 on error (bh_last_error), device pointers unless marked host.
 *
 * For all four lens models the pixel mean is  mean2d = f (.) d(mean_c) + c  and the projection Jacobian  J = diag(fx, fy) J',
 * where d (the distorted normalised coordinate) and J' are free of fx, fy, cx, cy.  Constants: the four lim_* clamp limits,
 * half_max_render_fov, dist[], and — as for the splat and pose gradients — the Mip opacity compensation and the frozen min_scale.
 *
 * v_intrinsics [4] f32 = (v_fx, v_fy, v_cx, v_cy): the gradient of <v_output, image>, plus whatever other cotangents the call
 * carries, with respect to BhCamera.fx, fy, cx, cy.  Per visible splat, from its RasterizeGrads row g (g0 g1 = v_xy, g2 g3 g4 =
 * the conic gradient):
 *   G  = inverse2x2_vjp(conic, {g2, g3 / 2, g4})   the gradient with respect to the blurred covariance as a full symmetric 2x2
 *                                                   matrix: G01 stands at both off-diagonal positions, so the symmetric entry
 *                                                   A01 receives 2 G01
 *   A  = the raw 2-D covariance before the blur (A00 ~ fx^2, A01 ~ fx fy, A11 ~ fy^2)
 *   (xd, yd) = d(mean_c), from the lens law itself (not (mean2d - c) / f)
 *   v_fx_i = g0 xd + 2 (G00 A00 + G01 A01) / fx        v_cx_i = g0
 *   v_fy_i = g1 yd + 2 (G11 A11 + G01 A01) / fy        v_cy_i = g1
 * A row whose five geometry entries are all zero contributes zero.  The four f32 contributions are widened to f64 and summed in a
 * fixed order, without atomics: the same RasterizeGrads rows give the same bits.  The output is always fully overwritten (an empty
 * view writes four zeros).
 *
 * The gradient is complete where the pose gradient is not: camera z, the rendered normals and the feature blend do not depend on
 * the intrinsics, so the depth, rendered-normal, distortion and feature cotangents reach them through the blend weights alone, and
 * those are accumulated into the rows this pass reads.
 *
 * Not built: gradients to dist[] (a gradient through the mean alone would be a wrong one, so none is returned); the clamp limits'
 * dependence on fx, cx; the intrinsics gradient with an environment map (the ray directions depend on the intrinsics) or with the
 * depth-to-normal stencil of the normal-consistency term (it uses fx, fy) — the train step refuses both; a device-side optimizer;
 * and the feature cotangent in bh_render_backward_camera_saved (bh_render_backward_features_saved has no camera outputs).
 */
#ifndef BRUSH_HIP_INTRINSICS_H
#define BRUSH_HIP_INTRINSICS_H

#include "brush_hip.h"
#include "brush_hip_distortion.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bh_render_backward_pose_saved plus the intrinsics gradient: the same arguments, forwards, error codes and the same bits in the
 * four splat outputs; v_intrinsics [4] as above.  v_viewmat [12] may be NULL (no pose pass); with it both camera gradients come from
 * one backward.  Queued on the ctx stream; no readback. */
int bh_render_backward_intrinsics_saved(bh_ctx* ctx, const BhRenderOut* saved /*host*/, const float* v_output, const float* transforms,
                                        const float* sh_coeffs, const float* raw_opacities, float* v_transforms /*[N,10]*/,
                                        float* v_sh_coeffs /*[N,C,3]*/, float* v_raw_opacities /*[N]*/, float* v_refine_weight /*[N]*/,
                                        float* v_viewmat /*[12] or NULL*/, float* v_intrinsics /*[4]*/);

/* The optional terms of bh_render_backward_camera_saved: a NULL cotangent is no term (its mode is not looked at). */
typedef struct BhCameraGradTerms {
    const float* v_depth;          /* [H,W] with depth_mode (brush_hip_depth.h), or NULL */
    const float* v_normal;         /* [H,W,3] with normal_mode (brush_hip_normal.h), or NULL */
    const float* v_distortion;     /* [H,W] with `distortion` (brush_hip_distortion.h), or NULL */
    uint32_t depth_mode;
    uint32_t normal_mode;
    BhDistortionConfig distortion;
} BhCameraGradTerms;

/* The general entry: bh_render_backward_intrinsics_saved with the optional depth, rendered-normal and distortion cotangents of
 * `terms` (host; NULL: none) beside v_output, which may then be NULL.  v_intrinsics is the gradient of the whole sum.  v_viewmat
 * must be NULL when a term is given: the pose pass does not carry the terms' gradients (BH_ERR_INVALID_ARG). */
int bh_render_backward_camera_saved(bh_ctx* ctx, const BhRenderOut* saved /*host*/, const float* v_output /*or NULL*/,
                                    const BhCameraGradTerms* terms /*host, or NULL*/, const float* transforms, const float* sh_coeffs,
                                    const float* raw_opacities, float* v_transforms, float* v_sh_coeffs, float* v_raw_opacities,
                                    float* v_refine_weight, float* v_viewmat /*[12] or NULL*/, float* v_intrinsics /*[4]*/);

/* Attaches an intrinsics-gradient buffer to bh_train_step: every subsequent step writes the intrinsics gradient of that step's whole
 * loss (LPIPS, depth, distortion and feature terms included) for that step's camera, and changes in nothing else.  With a tile-row
 * window the value is the window's partial sum.  NULL detaches: no write, no launch.  While a buffer is attached a step with an
 * environment map or an active normal-consistency term is refused (BH_ERR_STATE). */
int bh_train_set_intrinsics_grad(bh_ctx* ctx, float* v_intrinsics /*device [4]; NULL detaches*/);

/* Host only.  Writes fx, fy, cx, cy (rounded to f32) into *cam and recomputes lim_* and half_max_render_fov for the camera's model
 * exactly as bh_camera_setup_model does from the same values (the fields of view are bh_focal_to_fov of the f64 focals over
 * img_w, img_h).  Non-finite values or fx, fy <= 0 return -1 and leave *cam as it was. */
int bh_camera_set_intrinsics(BhCamera* cam /*host*/, double fx, double fy, double cx, double cy);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_INTRINSICS_H */
