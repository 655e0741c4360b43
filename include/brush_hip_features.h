/* brush_hip_features.h — feature maps of a rendered frame: the blend of caller-owned per-splat vectors with any channel count
 * (semantic logits, identity encodings, distilled image features; what gsplat renders as colors [N, D]), the gradient back into
 * those vectors and into the splats, and two fused losses on such a map.  An operator over the state a BH_FLAG_BWD_INFO forward
 * saved (brush_hip.h BhRenderOut), on the GPU.  DESIGN.md §6r has the whole contract.
 *
 * Same conventions as brush_hip.h: 0 on success, <0 on error (bh_last_error), device pointers unless marked host.
 *
 * Layout: features [N, C] f32, row-major, indexed by the global splat id; maps [H, W, C] f32; 1 <= C <= BH_FEATURE_MAX_CHANNELS.
 *
 * Per pixel, w_i = T_i * alpha_i is the colour blend's own weight: the same alpha, 1/255 cut-off (hard or smooth), 0.999 clamp,
 * saturation rule and list order as bh_render_depth (brush_hip_depth.h), bit for bit.  Every channel is folded front to back by ONE
 * explicit fmaf(f, w, acc) per term, as the colour channels are: a feature map whose first three channels hold the projected rgb
 * of a degree-0 scene over a black background IS the colour image, bit for bit, whatever the other channels hold.  Nothing is
 * clamped (features may be negative), the background contributes nothing.
 *
 * A feature term inside bh_train_step and the row carry through a refine are brush_hip_feature_train.h.
 *
 * Not built: a feature term combined with a depth / normal / distortion cotangent or with the pose gradient in one backward ENTRY
 * POINT (the train step's own backward carries the depth, normal, distortion and feature terms together); a normalised F / A mode.
 */
#ifndef BRUSH_HIP_FEATURES_H
#define BRUSH_HIP_FEATURES_H

#include "brush_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_FEATURE_MAX_CHANNELS 256u

/* out [H,W,C] f32 = sum of w_i features[i, :] over the contributing splats of the forward `saved` — valid for the forwards
 * bh_render_depth accepts (the ctx's most recent forward, or a retained one; BH_ERR_STATE otherwise, BH_ERR_INVALID_ARG for a
 * forward without BH_FLAG_BWD_INFO).  BH_ERR_INVALID_ARG for a null argument, channels == 0 or > BH_FEATURE_MAX_CHANNELS.  Queued
 * on the ctx stream; no readback, no atomics: any number of calls give the same bits, whatever the forward's list policy.  A forward
 * of a tile-row window writes its rows only; a frame that lists nothing clears its window. */
int bh_render_features(bh_ctx* ctx, const BhRenderOut* saved /*host*/, const float* features /*[N,C]*/, uint32_t channels,
                       float* out /*[H,W,C]*/);

/* Gradients of <v_output, image> + <v_map, feature map> of the forward `saved`: bh_render_backward_saved with a feature term.
 * v_output [H,W,4] or NULL (feature term only); v_map [H,W,C].  The four usual outputs are dense and fully overwritten;
 * v_refine_weight is the colour term's alone (zero without v_output).  v_features [N,C] = sum over pixels of w_ip v_map[p, :], dense
 * and fully overwritten: rows of splats the frame did not list are +0. */
int bh_render_backward_features_saved(bh_ctx* ctx, const BhRenderOut* saved /*host*/, const float* v_output /*or NULL*/, const float* features /*[N,C]*/,
                                      uint32_t channels, const float* v_map /*[H,W,C]*/, const float* transforms, const float* sh_coeffs,
                                      const float* raw_opacities, float* v_transforms /*[N,10]*/, float* v_sh_coeffs /*[N,K,3]*/,
                                      float* v_raw_opacities /*[N]*/, float* v_refine_weight /*[N]*/, float* v_features /*[N,C]*/);

/* The fused losses of a feature map F [H,W,C] against a target.
 *
 * BH_FEATURE_LOSS_L1 (distillation): target = f32 [H,W,C].  A pixel is VALID when all its C target values are finite.
 *   d_c = F_c - t_c, ONE f32 subtraction;  l = sum over c of |d_c|, each |d_c| converted to f64 and added in channel order;
 *   v_map_c = sign(d_c) * c_w with sign(0) = 0;  c_w = weight / (H W C).
 * BH_FEATURE_LOSS_CROSS_ENTROPY (segmentation): target = uint8 [H,W] labels.  A pixel is VALID when label < C (255 is the
 *   conventional "ignore").  m = max over c of F_c (f32, exact);  x_c = (double)F_c - (double)m (exact in f64 for finite logits);
 *   e_c = exp(x_c), the f64 exp of the device math library;  s = sum of e_c in channel order (f64);
 *   l = log(s) + ((double)m - (double)F_label), the f64 log;  v_map_c = c_w * (float)(e_c / s - [c == label]): the bracket in
 *   f64, rounded to f32 ONCE, then one f32 product;  c_w = weight / (H W).  No exp overflows: every x_c <= 0.
 * c_w is rounded to f32 ONCE on the host ((float)((double)weight / (double)count)).
 * loss = { (float)((double)c_w * sum over valid pixels of l), the number of valid pixels }: the sum is f64, per-block partials in
 * a context slot combined in a fixed order by one block, no float atomics — two calls give the same bits.  Invalid pixels
 * contribute 0 and get v_map = +0 in every channel. */
#define BH_FEATURE_LOSS_L1            0u
#define BH_FEATURE_LOSS_CROSS_ENTROPY 1u

typedef struct BhFeatureTarget {
    const void* target;   /* device: f32 [H,W,C] (L1) or uint8 [H,W] (cross-entropy) */
    uint32_t h, w;
    uint32_t channels;    /* C of the map */
    uint32_t kind;
    float weight;         /* <= 0 (or not a number) means no term */
    uint32_t reserved;
} BhFeatureTarget;

#ifdef __cplusplus
static_assert(sizeof(BhFeatureTarget) == 32, "BhFeatureTarget layout");
#else
_Static_assert(sizeof(BhFeatureTarget) == 32, "BhFeatureTarget layout");
#endif

/* loss [2] (device) as above; v_map [H,W,C] or NULL = dloss / dF.  weight <= 0 (or not a number): both outputs are all +0 — the
 * count too, nothing is read.  BH_ERR_INVALID_ARG for a null argument, h or w == 0, channels == 0 or > BH_FEATURE_MAX_CHANNELS and
 * an unknown kind.  Queued on the ctx stream: no readback, no synchronisation.  v_map may not alias map or the target. */
int bh_feature_loss_value_and_grad(bh_ctx* ctx, const float* map /*[H,W,C]*/, const BhFeatureTarget* target /*host*/, float* loss /*device [2]*/,
                                   float* v_map /*[H,W,C] or NULL*/);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_FEATURES_H */
