/* brush_hip_lift.h — mask lifting: what the user holds in image space (a lasso in a viewer, a SAM mask per view, a segmentation
 * rendered from a feature field) turned into a choice of splats.  For every splat, the weight with which it reached the pixels of
 * each label of a 2-D label map, summed over views:
 *
 *     votes[i, l] = sum over views, sum over pixels p of w_ip * [label(p) == l]
 *
 * followed by a per-splat argmax (bh_lift_assign) or threshold (bh_lift_select) — the scatter of SAGA, Gaussian Grouping, FlashSplat
 * and SuperSplat's selection tools — and, from the same pass over the lists, the two per-splat statistics contribution-based pruning
 * uses (RadSplat, LightGaussian): the largest weight a splat ever had at a pixel and the number of pixels it reached.  Operators
 * over the state a BH_FLAG_BWD_INFO forward saved (brush_hip.h BhRenderOut), on the GPU.  DESIGN.md §6u has the whole contract.
 *
 * Same conventions as brush_hip.h: 0 on success, <0 on error (bh_last_error), device pointers unless marked host.
 *
 * THE WEIGHT.  w_ip is the colour blend's own weight: the one f32 product alpha_eff * T of bh_render_features
 * (brush_hip_features.h), with the same alpha, 1/255 cut-off (hard or smooth), 0.999 clamp, saturation rule and list order, bit for
 * bit: the pass is the forward's replay, with the forward's early exit.
 *
 * A VOTE is the weight in fixed point: q = (uint32_t)rintf(w * 16777216.0f).  The product by 2^24 is exact, so this is ONE rounding,
 * half to even; 0 < w <= 0.999, so q < 2^24.  Sums are integer additions: independent of order, so two calls, two list policies or
 * two tile orders give the same bits, and a numpy restatement reproduces them exactly from the f32 weights.
 *
 * BOUNDS.  A tile's 256 pixels sum to at most 256 * 0.999 * 2^24 < 2^32: the per-tile sums are u32.  A votes entry is exact while a
 * splat's summed weight over all accumulated views is below 2^40 (2^64 / 2^24); the Python mirror reads the table as int64 and so
 * asks for less than 2^39.  The conversions to double (bh_lift_assign's share, bh_lift_select's share test, weights = votes / 2^24)
 * are exact while a row's total is below 2^53 in raw units, i.e. a summed weight below 2^29: eight hours of 1080p frames that a
 * splat covers completely at full weight.
 *
 * Not built: votes inside bh_train_step; multi-GPU accumulation (the tables are integers: an all-reduce of them by sum — max for
 * max_weight — is exact, whatever the order); soft labels (a per-pixel distribution is a cotangent: bh_render_backward_features_saved);
 * per-label maxima; feature fields through the compaction (the indices bh_decimate_to_count returns serve FeatureField.gather).
 */
#ifndef BRUSH_HIP_LIFT_H
#define BRUSH_HIP_LIFT_H

#include "brush_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_LIFT_MAX_LABELS 256u
#define BH_LIFT_IGNORE_LABEL 255u         /* the conventional "ignore" of a label map, as in the cross-entropy target */
#define BH_LIFT_UNASSIGNED 255u           /* bh_lift_assign: the splat got no label */
#define BH_LIFT_ANY_LABEL 0xFFFFFFFFu     /* BhLiftSelect.label: no share test */
#define BH_LIFT_VOTE_ONE 16777216.0f      /* a weight of 1 in raw units (2^24) */

/* One view's votes, ADDED to the caller's tables.  `saved`: valid for the forwards bh_render_features accepts (the ctx's most
 * recent forward, or a retained one; BH_ERR_STATE otherwise, BH_ERR_INVALID_ARG for a forward without BH_FLAG_BWD_INFO), under any
 * list policy: near and far lists, a tile-row window (its rows vote), a frame that lists nothing (the tables stay as they are).
 *   labels       uint8 [H,W], or NULL: every pixel has label 0.  A pixel whose label is >= num_labels (255 by convention) votes
 *                nowhere; it still counts in max_weight and pixel_count, which describe the render, not the labelling.
 *   votes        uint64 [N, num_labels], row-major by global splat id: votes[i, l] += sum of q over the pixels of label l.
 *   max_weight   f32 [N] or NULL: max_weight[i] = max(max_weight[i], max over pixels of w_ip), by an unsigned integer maximum on the
 *                floats' bits (weights are positive): exact and independent of order.  The table must hold non-negative floats.
 *   pixel_count  uint32 [N] or NULL: += the number of (pixel, splat) terms that contributed.
 * Rows of splats the frame did not list are not touched.  Queued on the ctx stream: no readback, no scratch.  Refused before any
 * launch with BH_ERR_INVALID_ARG: a null saved or votes, num_labels == 0 or > BH_LIFT_MAX_LABELS, a votes, max_weight or
 * pixel_count that overlaps labels or another of the three. */
int bh_lift_accumulate(bh_ctx* ctx, const BhRenderOut* saved /*host*/, const uint8_t* labels /*[H,W] or NULL*/, uint32_t num_labels,
                       uint64_t* votes /*[N,L], added to*/, float* max_weight /*[N] or NULL, max-ed into*/,
                       uint32_t* pixel_count /*[N] or NULL, added to*/);

/* From votes to a label per splat.  total = the integer sum of the row; labels_out[i] = the argmax of the row, ties to the LOWEST
 * label; BH_LIFT_UNASSIGNED when total == 0 or total < (uint64_t)rint((double)min_weight * 2^24) (computed once on the host; a
 * min_weight that is not > 0 means 0).  share_out[i] = (float)((double)votes[i, best] / (double)total), +0 where unassigned.
 * With num_labels == 256 label 255 and "unassigned" share a value: share_out tells them apart (> 0 where assigned).
 * BH_ERR_INVALID_ARG for a null votes or labels_out with n > 0 and for num_labels == 0 or > BH_LIFT_MAX_LABELS. */
int bh_lift_assign(bh_ctx* ctx, const uint64_t* votes /*[N,L]*/, uint32_t n, uint32_t num_labels, float min_weight,
                   uint8_t* labels_out /*[N]*/, float* share_out /*[N] or NULL*/);

/* From votes and statistics to keep [N] = 1.0 / 0.0, which is what bh_decimate_to_count takes as scores: with target_count = the
 * number kept, its stable order makes it the compaction, rows in source order (as a region crop does, brush_hip_scene.h).
 * Every test that is asked for must pass; `invert` then flips the result.
 *   votes given (total = the row's integer sum): total > 0 and total >= (uint64_t)rint((double)min_weight * 2^24);
 *   label != BH_LIFT_ANY_LABEL: (double)votes[i, label] >= (double)min_share * (double)total — one f64 product, one compare;
 *   min_max_weight > 0: max_weight[i] >= min_max_weight;     min_pixels > 0: pixel_count[i] >= min_pixels.
 * A test whose table is NULL is refused (BH_ERR_INVALID_ARG), not skipped: a label or a min_weight > 0 without votes, min_max_weight
 * > 0 without max_weight, min_pixels > 0 without pixel_count; so are a label >= num_labels, a min_share, min_weight or min_max_weight
 * that is not a number, num_labels == 0 or > BH_LIFT_MAX_LABELS with votes, a null sel, and a null keep with n > 0. */
typedef struct BhLiftSelect {
    uint32_t label;
    float min_share;
    float min_weight;
    float min_max_weight;
    uint32_t min_pixels;
    uint32_t invert;
} BhLiftSelect;

#ifdef __cplusplus
static_assert(sizeof(BhLiftSelect) == 24, "BhLiftSelect layout");
#else
_Static_assert(sizeof(BhLiftSelect) == 24, "BhLiftSelect layout");
#endif

int bh_lift_select(bh_ctx* ctx, const uint64_t* votes /*[N,L] or NULL*/, const float* max_weight /*[N] or NULL*/,
                   const uint32_t* pixel_count /*[N] or NULL*/, uint32_t n, uint32_t num_labels, const BhLiftSelect* sel /*host*/,
                   float* keep /*[N]*/);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_LIFT_H */
