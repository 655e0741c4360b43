/* brush_hip_depth_loss.h — depth supervision: a fused depth loss on an expected-depth map (brush_hip_depth.h), a depth term in
 * bh_train_step, and held-out depth metrics.  DESIGN.md §6l has the whole contract.
 *
 * Same conventions as brush_hip.h: 0 on success, <0 on error (bh_last_error), device pointers unless marked host.
 *
 * Definitions (E = a pixel of the expected-depth map, gt = the same pixel of the target):
 *   t = fmaf(scale, gt, offset), ONE f32 fma.
 *   A pixel is VALID when gt is finite, t > 0 and E > 0.  Expected depth is 0 where alpha is 0, so E > 0 excludes empty pixels
 *   without reading the image.  Invalid pixels contribute 0 to the loss and get v_depth = 0.
 *   BH_DEPTH_LOSS_L1:         l = |E - t|,    v_depth = sign(E - t) * c
 *   BH_DEPTH_LOSS_DISPARITY:  l = |1/E - t|,  v_depth = -sign(1/E - t) * c / E^2   (evaluated as -(s * c) / (E * E))
 *   with c = weight / (H W), rounded to f32 ONCE on the host ((float)((double)weight / (double)(H W))), and sign(0) = 0: the
 *   derivative of |x| at 0 is 0.  The sign is that of the f32 difference (E - t, or 1/E - t with 1/E the correctly rounded f32
 *   quotient).
 *   loss = c * sum over valid pixels of l: normalised by H W, NOT by the valid count (INRIA's (.. * mask).abs().mean()) — one
 *   pass, and a gradient that does not depend on a reduction.  l is an f32 per pixel; the sum is f64: per-block partials in a
 *   context slot, combined in a fixed order by one block, no float atomics — two calls give the same bits.
 */
#ifndef BRUSH_HIP_DEPTH_LOSS_H
#define BRUSH_HIP_DEPTH_LOSS_H

#include "brush_hip_depth.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_DEPTH_LOSS_L1        0u  /* gt holds depth z;        l = |E - t| */
#define BH_DEPTH_LOSS_DISPARITY 1u  /* gt holds inverse depth;  l = |1/E - t| */

typedef struct BhDepthTarget {
    const float* gt;      /* [H,W] f32 device */
    uint32_t h, w;
    uint32_t kind;
    float weight;         /* of the term in the step's loss; <= 0 means no term */
    float scale, offset;  /* t = fmaf(scale, gt, offset): per-view alignment of a monocular prior (INRIA's depth_params); 1, 0 for metric depth */
} BhDepthTarget;

#ifdef __cplusplus
static_assert(sizeof(BhDepthTarget) == 32, "BhDepthTarget layout");
#else
_Static_assert(sizeof(BhDepthTarget) == 32, "BhDepthTarget layout");
#endif

/* loss [2] (device) = { weight * sum(l) / (H W) as an f32, the number of valid pixels as an f32 };  v_depth [H,W] or NULL = dloss / dE.
 * weight <= 0 (or not a number): both outputs are all +0 — the count too, no pixel is looked at.
 * BH_ERR_INVALID_ARG for a null argument, h or w == 0 and an unknown kind.  Queued on the ctx stream: no readback, no
 * synchronisation.  v_depth may not alias depth or gt. */
int bh_depth_loss_value_and_grad(bh_ctx* ctx, const float* depth /*[H,W], an expected-depth map*/, const BhDepthTarget* target /*host*/,
                                 float* loss /*device [2]*/, float* v_depth /*[H,W] or NULL*/);

/* A depth term in bh_train_step.  Sticky like bh_train_set_pose_grad: the struct is copied (the gt pointer must stay valid through
 * the steps that use it), NULL detaches; set it before a step whose view has a depth map and detach it before one that has none.
 * A step with no target, or with weight <= 0, launches nothing new and gives the bits it gave without this header.
 * A step with a target renders the expected depth of its final frame (behind a second attempt with complete lists, if there was
 * one), runs the loss above on it and passes v_depth to the backward it already runs.  The step's loss is composed in f32 IN THIS
 * ORDER:    loss = (image term  [+ lpips_weight * LPIPS])  + depth_loss[0]
 * Depth is not a colour: an exposure table does not touch it.
 * The step refuses (BH_ERR_INVALID_ARG, before any launch, step_count unchanged): a target whose h, w differ from the camera's;
 * an unknown kind; a tile-row partition of the frame (image hook or window: the term needs the whole frame on this rank); an
 * attached pose-gradient buffer (the pose pass does not see the path v_z -> row 2 of the view matrix). */
int bh_train_set_depth(bh_ctx* ctx, const BhDepthTarget* target /*host; copied; NULL detaches*/);

/* Held-out depth metrics of an expected-depth map against a target; kind, scale, offset and validity as above, weight ignored.
 * z_t = t for BH_DEPTH_LOSS_L1 and 1 / t (f32) for BH_DEPTH_LOSS_DISPARITY.  metrics [4] (device, f32):
 *   [0] abs-rel: mean over valid pixels of |E - z_t| / z_t       [1] RMSE over valid pixels of E - z_t
 *   [2] share of valid pixels with max(E / z_t, z_t / E) < 1.25  [3] the valid count
 * Per-pixel terms are formed in f64 from the f32 E and z_t; the sums are f64 and deterministic.  No valid pixel: the first three are 0. */
int bh_eval_depth_metrics(bh_ctx* ctx, const float* depth /*[H,W]*/, const BhDepthTarget* target /*host*/, float* metrics /*device [4]*/);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_DEPTH_LOSS_H */
