/* brush_hip_distortion.h — distortion maps of a rendered frame (2DGS's depth distortion, gsplat's `distloss`, the regulariser of
 * Mip-NeRF 360), their gradient, the loss and the term in bh_train_step: operators over the state a BH_FLAG_BWD_INFO forward saved
 * (brush_hip.h BhRenderOut), on the GPU.  DESIGN.md §6o has the whole contract.
 *
 * Same conventions as brush_hip.h: 0 on success, <0 on error (bh_last_error), device pointers unless marked host; a null ctx returns
 * BH_ERR_INVALID_ARG before the device is touched.
 *
 * Per pixel, over the contributing splats of the colour blend in the blend's order, with the blend's own weight w_i = alpha_eff_i * T_i
 * (brush_hip_depth.h: the same alpha, cut-off, clamp, saturation rule and list order, bit for bit) and a per-splat depth m_i:
 *
 *     dist = sum over i, sum over j < i of  w_i w_j (m_i - m_j)^2  =  A * M2 - M1^2
 *     A = sum w_i,   M1 = sum w_i m_i,   M2 = sum w_i m_i^2
 *
 * 2DGS's distortion map, unnormalised; the background contributes nothing.  m_i comes from z_i, the camera-space z of the splat's mean
 * (BhRenderOut.depths_sorted), for every lens model.  dist does not change when every m of a pixel is shifted by the same amount, and
 * the kernels use that: they fold m_i - r with r = the m of the pixel's first contributing splat (a constant of the pixel, no gradient),
 * because A * M2 - M1^2 of unshifted f32 sums loses the spread to cancellation once the depth is large against it.  A is the colour
 * image's alpha 1 - |T|, as BH_DEPTH_EXPECTED takes it.
 */
#ifndef BRUSH_HIP_DISTORTION_H
#define BRUSH_HIP_DISTORTION_H

#include "brush_hip_depth.h"
#include "brush_hip_normal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_DISTORTION_Z 0u   /* m = z */
#define BH_DISTORTION_NDC 1u /* m = far (z - near) / ((far - near) z): 2DGS's mapping, independent of the scene's scale; near > 0, far > near */

typedef struct BhDistortionConfig {
    uint32_t kind;  /* BH_DISTORTION_Z or BH_DISTORTION_NDC */
    float near_z;   /* BH_DISTORTION_NDC only (ignored for BH_DISTORTION_Z) */
    float far_z;
    uint32_t reserved; /* 0 */
} BhDistortionConfig;

typedef struct BhDistortionTermConfig {
    float weight;   /* of the term in the step's loss; <= 0 or not a number means no term */
    uint32_t kind;  /* BH_DISTORTION_Z or BH_DISTORTION_NDC */
    float near_z;   /* BH_DISTORTION_NDC only */
    float far_z;
} BhDistortionTermConfig;

#ifdef __cplusplus
static_assert(sizeof(BhDistortionConfig) == 16, "BhDistortionConfig layout");
static_assert(sizeof(BhDistortionTermConfig) == 16, "BhDistortionTermConfig layout");
#else
_Static_assert(sizeof(BhDistortionConfig) == 16, "BhDistortionConfig layout");
_Static_assert(sizeof(BhDistortionTermConfig) == 16, "BhDistortionTermConfig layout");
#endif

/* out [H,W] f32 = the distortion map of the forward `saved` — valid for the forwards bh_render_depth accepts (the ctx's most recent
 * forward, or a retained one), BH_ERR_STATE otherwise.  BH_ERR_INVALID_ARG for a null argument, an unknown kind, near <= 0 or
 * far <= near (NDC), or a forward without BH_FLAG_BWD_INFO.  A forward of a tile-row window writes its rows only; a frame that lists
 * nothing clears its window.  No atomics: any number of calls give the same bits.  Queued on the ctx stream; no readback. */
int bh_render_distortion(bh_ctx* ctx, const BhRenderOut* saved /*host*/, const BhDistortionConfig* cfg /*host*/, float* out /*[H,W]*/);

/* out [H,W,4] f32 = the moment map { A, M1', M2', r } of the same blend (M' = the sums of the shifted depths m_i - r): what the loss and
 * the backward read; dist = A * M2' - M1'^2.  Same rules as bh_render_distortion. */
int bh_render_distortion_moments(bh_ctx* ctx, const BhRenderOut* saved /*host*/, const BhDistortionConfig* cfg /*host*/, float* out /*[H,W,4]*/);

/* Gradients of <v_output, image> + <v_depth, depth(depth_mode)> + <v_normal, normal(normal_mode)> + <v_distortion, dist> of the forward
 * `saved` in ONE backward.  Every cotangent except v_distortion [H,W] may be NULL.  d dist / d w_i = m_i^2 A + M2 - 2 m_i M1 reaches
 * alpha and the geometry; d dist / d m_i = 2 w_i (m_i A - M1) reaches the means through dm/dz and row 2 of the view rotation (both
 * evaluated on the shifted depths).  The four outputs are dense and fully overwritten; v_refine_weight is the colour term's alone.
 * Refusals as bh_render_backward_normal_saved's and bh_render_distortion's. */
int bh_render_backward_distortion_saved(bh_ctx* ctx, const BhRenderOut* saved /*host*/, const float* v_output /*or NULL*/, const float* v_depth /*or NULL*/,
                                        uint32_t depth_mode, const float* v_normal /*or NULL*/, uint32_t normal_mode, const float* v_distortion /*[H,W]*/,
                                        const BhDistortionConfig* cfg /*host*/, const float* transforms, const float* sh_coeffs,
                                        const float* raw_opacities, float* v_transforms /*[N,10]*/, float* v_sh_coeffs /*[N,C,3]*/,
                                        float* v_raw_opacities /*[N]*/, float* v_refine_weight /*[N]*/);

/* loss [2] (device) = { c * sum(dist) as an f32, the number of pixels as an f32 }, c = weight / (H W) rounded to f32 ONCE on the host.
 * map: channels == 1: a distortion map [H,W]; channels == 4: a moment map [H,W,4] (dist = fmaf(A, M2', -(M1' * M1')) per pixel, as
 * bh_render_distortion stores it).  The sum is f64: per-block partials in a context slot, combined in a fixed order by one block, no
 * atomics — two calls give the same bits.  The gradient with respect to dist is the constant c.  weight <= 0 or not a number: loss is
 * all +0 and no pixel is read.  BH_ERR_INVALID_ARG for a null argument, h or w == 0, more than 2^31 - 1 pixels, channels other than 1
 * or 4.  Queued on the ctx stream: no readback, no synchronisation. */
int bh_distortion_loss(bh_ctx* ctx, const float* map, uint32_t h, uint32_t w, uint32_t channels, float weight, float* loss /*device [2]*/);

/* A distortion term in bh_train_step.  Sticky like bh_train_set_normal: the struct is copied; NULL, a weight <= 0 or a weight that is
 * not a number detaches.  BH_ERR_INVALID_ARG (nothing changes) for an unknown kind or bad near / far with a weight > 0.  A step with
 * nothing attached launches nothing new and gives the bits it gave without this header.
 * A step with the term works on its final frame (behind a second attempt with complete lists, if there was one), behind the normal term:
 * it renders the moment map, adds weight * sum(dist) / (H W) to its loss and passes the uniform cotangent weight / (H W) and the moment
 * map to the one backward it already runs (no [H,W] cotangent exists, the map is not rendered twice).
 * The step's loss is composed in f32 IN THIS ORDER:  (image term [+ lpips]) + depth_loss[0] + normal_loss[0] + distortion_loss[0]
 * An empty frame contributes 0 and launches none of this.
 * The step refuses (BH_ERR_INVALID_ARG, before any launch, step_count unchanged): a tile-row partition of the frame (image hook or
 * window); an attached pose-gradient buffer. */
int bh_train_set_distortion(bh_ctx* ctx, const BhDistortionTermConfig* cfg /*host; copied; NULL detaches*/);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_DISTORTION_H */
