/* brush_hip_pose.h — the gradient of a rendered frame with respect to its camera pose (what gsplat returns as v_viewmats), and
 * the host arithmetic of a pose update: an operator over the state a BH_FLAG_BWD_INFO forward saved.  DESIGN.md §6j has the
 * whole contract.
 *
 * Same conventions as brush_hip.h: 0 on success, <0 on error (bh_last_error), device pointers unless marked host.
 *
 * The camera is BhCamera.vm: W (3x3 world-to-camera rotation) and t (translation).  mean_c = W mean + t, cov_c = W Sigma W^T, and
 * the SH view direction is (mean - p) / |mean - p| with p = -W^T t: the cam_pos field is treated as that function of W and t.
 * Intrinsics, distortion coefficients and the Jacobian clamp limits are constants (the gradient with respect to fx, fy, cx, cy is
 * brush_hip_intrinsics.h's, and bh_render_backward_intrinsics_saved returns both from one backward); in Mip mode the opacity compensation is a
 * constant of the geometry, as it is for the splat gradients.
 *
 * v_viewmat [12] f32, in the layout of BhCamera.vm (column-major 3x4), is the gradient of <v_output, image> with respect to the
 * twelve entries taken as free variables:
 *   v_p = -sum v_mean_from_sh,   v_t = sum v_mean_c - W v_p,   v_W = sum (v_mean_c (x) mean + 2 vcc W Sigma) - t (x) v_p
 * over the visible splats.  The sum is taken in f64 in a fixed order, without atomics: the same RasterizeGrads rows give the same
 * bits.  The output is always fully overwritten (an empty view writes twelve zeros).
 */
#ifndef BRUSH_HIP_POSE_H
#define BRUSH_HIP_POSE_H

#include "brush_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bh_render_backward_saved plus the pose gradient: the same arguments, forwards, error codes and — under the conditions under
 * which bh_render_backward_saved repeats itself — the same bits in the four splat outputs; v_viewmat [12] as above.  Queued on the
 * ctx stream; no readback. */
int bh_render_backward_pose_saved(bh_ctx* ctx, const BhRenderOut* saved /*host*/, const float* v_output, const float* transforms,
                                  const float* sh_coeffs, const float* raw_opacities, float* v_transforms /*[N,10]*/,
                                  float* v_sh_coeffs /*[N,C,3]*/, float* v_raw_opacities /*[N]*/, float* v_refine_weight /*[N]*/,
                                  float* v_viewmat /*[12]*/);

/* Attaches a pose-gradient buffer to bh_train_step: every subsequent step writes the pose gradient of that step's whole loss
 * (everything that reaches v_output, LPIPS included) for that step's camera, and changes in nothing else.  With a tile-row window
 * the value is the window's partial sum (add the strips with bh_allreduce_sum_f32).  NULL detaches: no write, no launch. */
int bh_train_set_pose_grad(bh_ctx* ctx, float* v_viewmat /*device [12]; NULL detaches*/);

/* Host only, f64.  The twist (v_omega, v_tau) of v_viewmat at vm: the derivative of the loss along
 * W <- exp([omega]x) W, t <- exp([omega]x) t + tau at zero:  v_tau = v_t,  v_omega = axial(v_W W^T - W v_W^T) + t x v_t. */
int bh_pose_twist(const float vm[12] /*host*/, const float v_viewmat[12] /*host*/, double twist[6] /*host*/);

/* Host only, f64.  Left-multiplies the pose by the twist (omega, tau): W <- exp([omega]x) W, t <- exp([omega]x) t + tau,
 * re-orthonormalises W, and rewrites cam->vm and cam->cam_pos (= -W^T t) together.  A vm that is no pose (first two columns
 * zero or parallel) or a twist that is not finite returns -1 and leaves *cam as it was. */
int bh_camera_apply_twist(BhCamera* cam /*host*/, const double twist[6] /*host*/);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_POSE_H */
