/* brush_hip_normal_loss.h — the normal-consistency regulariser (2DGS): a fused loss between the rendered normal map of a frame
 * (brush_hip_normal.h) and the normals of its expected-depth map, and the term in bh_train_step.  DESIGN.md §6n has the whole contract.
 *
 * Same conventions as brush_hip.h: 0 on success, <0 on error (bh_last_error), device pointers unless marked host; a null ctx returns
 * BH_ERR_INVALID_ARG before the device is touched.
 *
 * Definitions (p = a pixel; N = the BH_NORMAL_ACCUMULATED map, A = the alpha of the colour image, both read as given):
 *   u(p) = the depth-derived normal of brush_hip_normal.h: the same stencil, the same validity rule (1 <= x <= W-2, 1 <= y <= H-2,
 *   depth finite and > 0 at the pixel and at its four axis neighbours), c / |c| with 0 where |c| == 0 — the library's one copy of it.
 *   A pixel is VALID when its stencil is valid.  Invalid pixels contribute 0 to the loss and get v_normal = 0.
 *   dot = fmaf(N.z, u.z, fmaf(N.y, u.y, N.x * u.x));   l = A * (1 - dot)       (f32, in this order)
 *   A is a CONSTANT of the term: no gradient reaches the image.  This is 2DGS's 1 - N . (A_detached u) summed over the frame, without
 *   its constant: the gradients are the same.
 *   c = weight / (H W), rounded to f32 ONCE on the host ((float)((double)weight / (double)(H W))).
 *   loss = c * sum over valid pixels of l.  l is an f32 per pixel; the sum is f64: per-block partials in a context slot, combined in a
 *   fixed order by one block, no float atomics — two calls give the same bits.
 *   v_normal(p) = (-(c * A)) * u   per component at a valid pixel, +0 elsewhere.
 *   v_depth(p)  = the gather of bh_depth_to_normal_backward with the cotangent v_u(q) = (-(c * A(q))) * N(q) at each of the at most
 *   four valid stencils q that read p — left neighbour's, right neighbour's, upper, lower, added in this order from +0.  v_u is formed
 *   from `normal` and `image` on the fly: no cotangent map exists in memory.  Invalid neighbourhoods give exactly 0.
 */
#ifndef BRUSH_HIP_NORMAL_LOSS_H
#define BRUSH_HIP_NORMAL_LOSS_H

#include "brush_hip_normal.h"
#include "brush_hip_depth_loss.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct BhNormalTermConfig {
    float weight;          /* of the term in the step's loss; <= 0 means no term */
    uint32_t reserved[3];  /* 0 */
} BhNormalTermConfig;

#ifdef __cplusplus
static_assert(sizeof(BhNormalTermConfig) == 16, "BhNormalTermConfig layout");
#else
_Static_assert(sizeof(BhNormalTermConfig) == 16, "BhNormalTermConfig layout");
#endif

/* loss [2] (device) = { c * sum(l) as an f32, the number of valid pixels as an f32 };  v_normal [H,W,3] = dloss / dN;
 * v_depth [H,W] = dloss / d depth: overwritten, or — accumulate_v_depth != 0 — added to what v_depth holds with ONE f32 add per pixel.
 * weight <= 0 (or not a number): loss and v_normal are all +0, no pixel is read, v_depth is all +0 or, under accumulate, untouched.
 * BH_ERR_INVALID_ARG for a null argument, h or w == 0, more than 2^31 - 1 pixels, a camera that is no pinhole, and v_normal or v_depth
 * overlapping an input or each other.  Queued on the ctx stream: no readback, no synchronisation. */
int bh_normal_consistency_value_and_grad(bh_ctx* ctx, const BhCamera* cam /*host, pinhole*/,
                                         const float* normal /*[H,W,3] BH_NORMAL_ACCUMULATED map*/, const float* depth /*[H,W] expected depth*/,
                                         const float* image /*[H,W,4]; only alpha is read, as a constant*/, uint32_t h, uint32_t w, float weight,
                                         uint32_t accumulate_v_depth, float* loss /*device [2]*/, float* v_normal /*[H,W,3]*/, float* v_depth /*[H,W]*/);

/* A normal-consistency term in bh_train_step.  Sticky like bh_train_set_depth: the struct is copied, NULL detaches.  A step with nothing
 * attached, or with weight <= 0, launches nothing new and gives the bits it gave without this header.
 * A step with the term works on its final frame (behind a second attempt with complete lists, if there was one): it renders the expected
 * depth (once, shared with an attached depth target), renders the accumulated normal map from the transforms the step rendered (with a
 * 3D filter the folded ones), runs the operator above on them and the frame's image (accumulate_v_depth = 1 when the depth loss has
 * already written v_depth) and passes v_depth (expected mode) and v_normal (accumulated mode) to the one backward it already runs.
 * The step's loss is composed in f32 IN THIS ORDER:    loss = (image term  [+ lpips_weight * LPIPS])  + depth_loss[0]  + normal_loss[0]
 * An empty frame contributes 0 and launches none of this.
 * The step refuses (BH_ERR_INVALID_ARG, before any launch, step_count unchanged): a camera that is no pinhole; a tile-row partition of
 * the frame (image hook or window); an attached pose-gradient buffer. */
int bh_train_set_normal(bh_ctx* ctx, const BhNormalTermConfig* cfg /*host; copied; NULL detaches*/);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_NORMAL_LOSS_H */
