/* brush_hip_depth.h — depth maps of a rendered frame, and their gradient (what gsplat calls RGB+D / RGB+ED): an operator over the
 * state a BH_FLAG_BWD_INFO forward saved (brush_hip.h BhRenderOut), on the GPU.  DESIGN.md §6i has the whole contract.
 *
 * Same conventions as brush_hip.h: 0 on success, <0 on error (bh_last_error), device pointers unless marked host.
 *
 * The depth of a splat is z, the camera-space z of its mean (row 2 of the view matrix applied to the mean: what
 * BhRenderOut.depths_sorted holds), for every lens model.  Per pixel, w_i = T_i * alpha_i is the colour blend's own weight: the
 * same alpha, 1/255 cut-off (hard or smooth), 0.999 clamp, saturation rule (the pixel is done WITHOUT a splat that would leave
 * T <= 1e-4) and list order, bit for bit.  Depth stops where colour stops, so the maps do not depend on the list policy of the
 * forward (complete lists, per-tile cuts, a near + far frame); a forward of a tile-row window writes its rows only.
 */
#ifndef BRUSH_HIP_DEPTH_H
#define BRUSH_HIP_DEPTH_H

#include "brush_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_DEPTH_ACCUMULATED 0u /* D = sum of w_i z_i, front to back, one fma per term; the background contributes 0 */
#define BH_DEPTH_EXPECTED 1u    /* D / A with A = 1 - T_final, the colour image's alpha; 0 where A == 0 */
#define BH_DEPTH_MEDIAN 2u      /* z of the contributing splat at which T first becomes <= 0.5; 0 where that never happens */

/* out_depth [H,W] f32 = the depth map `mode` of the forward `saved` — valid for the forwards bh_render_backward_saved accepts (the
 * ctx's most recent forward, or a retained one), BH_ERR_STATE otherwise.  BH_ERR_INVALID_ARG for an unknown mode or a forward
 * without BH_FLAG_BWD_INFO.  Queued on the ctx stream; no readback.  Leaves the saved state as it is: any number of calls, in any
 * order with the forward's backward, give the same bits. */
int bh_render_depth(bh_ctx* ctx, const BhRenderOut* saved /*host*/, uint32_t mode, float* out_depth /*[H,W]*/);

/* Gradients of <v_output, image> + <v_depth, depth(mode)> of the forward `saved`: bh_render_backward_saved with a depth term.
 * v_output [H,W,4] or NULL (depth term only); v_depth [H,W].  BH_DEPTH_ACCUMULATED or BH_DEPTH_EXPECTED (the chain through 1 / A
 * is part of the gradient); BH_DEPTH_MEDIAN has no gradient and is refused (BH_ERR_INVALID_ARG).  The four outputs are dense and
 * fully overwritten; v_refine_weight is the colour term's alone (zero without v_output). */
int bh_render_backward_depth_saved(bh_ctx* ctx, const BhRenderOut* saved /*host*/, const float* v_output /*or NULL*/, const float* v_depth,
                                   uint32_t mode, const float* transforms, const float* sh_coeffs, const float* raw_opacities,
                                   float* v_transforms /*[N,10]*/, float* v_sh_coeffs /*[N,C,3]*/, float* v_raw_opacities /*[N]*/,
                                   float* v_refine_weight /*[N]*/);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_DEPTH_H */
