/* brush_hip_normal.h — normal maps of a rendered frame, normals from a depth map, and their gradients: operators over the state a
 * BH_FLAG_BWD_INFO forward saved (brush_hip.h BhRenderOut), on the GPU.  DESIGN.md §6m has the whole contract.
 *
 * Same conventions as brush_hip.h and brush_hip_depth.h: 0 on success, <0 on error (bh_last_error), device pointers unless marked
 * host; a null ctx returns BH_ERR_INVALID_ARG before the device is touched.
 *
 * The normal of a splat.  `transforms` are the rendered ones: mean(3), quaternion wxyz(4), log-scale(3) — with a 3D filter the
 * folded ones.  k = the index of the smallest log-scale (the lowest index on an exact tie); n_w = column k of the rotation matrix
 * of the normalised quaternion (the matrix the projection builds); n_c = R_view n_w in camera space (R_view = BhCamera.vm,
 * column-major); with mean_c the camera-space mean, n = -n_c if n_c . mean_c > 0, else n_c: the normal faces the camera along the
 * ray to the mean.  The same for all four lens models.  k and the sign are piecewise constant: the normal's own gradient goes to
 * the quaternion only (through its normalisation), nothing to means or log-scales.
 *
 * The rendered normal map [H,W,3], camera space.  w_i = T_i * alpha_i is the colour blend's own weight, bit for bit, as in
 * brush_hip_depth.h: normals stop where colour stops, so the map does not depend on the list policy of the forward (complete
 * lists, per-tile cuts, a near + far frame); a forward of a tile-row window writes its rows only.
 *
 * Normals from a depth map [H,W] -> [H,W,3], pinhole cameras only.  d = depth[y,x] is z-depth;
 * P(x,y) = ((x + 0.5 - cx) / fx * d, (y + 0.5 - cy) / fy * d, d).  A pixel is valid when 1 <= x <= W-2, 1 <= y <= H-2 and d is
 * finite and > 0 at the pixel and at its four axis neighbours.  At a valid pixel gx = P(x+1,y) - P(x-1,y), gy = P(x,y+1) - P(x,y-1),
 * c = gy x gx, and the output is c / |c| (0 where |c| == 0): for a plane facing the camera c points at the camera (-z), the
 * orientation of the splat normals.  An invalid pixel is exactly 0.
 */
#ifndef BRUSH_HIP_NORMAL_H
#define BRUSH_HIP_NORMAL_H

#include "brush_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_NORMAL_ACCUMULATED 0u /* N = sum of w_i n_i, front to back, one fma per channel and term; the background contributes 0 */
#define BH_NORMAL_UNIT 1u        /* N / |N|; 0 where |N| == 0 */

/* out [N,3] = the normal of every splat as defined above: a pure function of the camera and the transforms, no visibility test. */
int bh_splat_normals(bh_ctx* ctx, const BhCamera* cam /*host*/, const float* transforms /*[N,10]*/, uint64_t n, float* out /*[N,3]*/);

/* out [H,W,3] f32 = the normal map `mode` of the forward `saved` — valid for the forwards bh_render_depth accepts (the ctx's most
 * recent forward, or a retained one), BH_ERR_STATE otherwise.  `transforms` [N,10] are the ones that forward rendered.
 * BH_ERR_INVALID_ARG for an unknown mode or a forward without BH_FLAG_BWD_INFO.  Queued on the ctx stream; no readback.  Leaves
 * the saved state as it is.  A forward with nothing listed clears the rows of its window. */
int bh_render_normal(bh_ctx* ctx, const BhRenderOut* saved /*host*/, const float* transforms, uint32_t mode, float* out /*[H,W,3]*/);

/* Gradients of <v_output, image> + <v_depth, depth(depth_mode)> + <v_normal, normal(normal_mode)> of the forward `saved` in one
 * backward.  v_output [H,W,4] or NULL; v_depth [H,W] or NULL (depth_mode as bh_render_backward_depth_saved: BH_DEPTH_MEDIAN is
 * refused); v_normal [H,W,3].  The four outputs are dense and fully overwritten; v_refine_weight is the colour term's alone. */
int bh_render_backward_normal_saved(bh_ctx* ctx, const BhRenderOut* saved /*host*/, const float* v_output /*or NULL*/,
                                    const float* v_depth /*or NULL*/, uint32_t depth_mode, const float* v_normal, uint32_t normal_mode,
                                    const float* transforms, const float* sh_coeffs, const float* raw_opacities,
                                    float* v_transforms /*[N,10]*/, float* v_sh_coeffs /*[N,C,3]*/, float* v_raw_opacities /*[N]*/,
                                    float* v_refine_weight /*[N]*/);

/* out [H,W,3] = the normals of the depth map `depth` [H,W] as defined above.  BH_ERR_INVALID_ARG for a camera that is no pinhole. */
int bh_depth_to_normal(bh_ctx* ctx, const BhCamera* cam /*host*/, const float* depth, uint32_t h, uint32_t w, float* out);

/* v_depth [H,W] = the gradient of <v_normal, depth_to_normal(depth)>: a gather (every pixel collects from the at most four valid
 * stencils that read it), no atomics: two calls give the same bits. */
int bh_depth_to_normal_backward(bh_ctx* ctx, const BhCamera* cam /*host*/, const float* depth, const float* v_normal /*[H,W,3]*/,
                                uint32_t h, uint32_t w, float* v_depth /*[H,W]*/);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_NORMAL_H */
