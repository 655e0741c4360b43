/* brush_hip_feature_train.h — feature fields trained jointly with the splats: a feature term inside bh_train_step (the blend of
 * brush_hip_features.h, one of its fused losses, the gradient into the vectors AND into the splats, one Adam step on the vectors) and
 * the row carry that takes any per-splat table through a refine.  What Feature-3DGS, Gaussian Grouping and gsplat's colors [N, D]
 * do: features that follow the geometry through densification.  DESIGN.md §6s has the whole contract.
 *
 * Same conventions as brush_hip.h: 0 on success, <0 on error (bh_last_error), device pointers unless marked host.
 *
 * Not built: a pose gradient with the term; tile-partitioned frames; mask-keyed compaction of the feature exchange (v_features
 * travels dense); an update that visits only the listed rows; a normalised F / A mode; features in the held-out evaluation.
 */
#ifndef BRUSH_HIP_FEATURE_TRAIN_H
#define BRUSH_HIP_FEATURE_TRAIN_H

#include "brush_hip_features.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A feature field: caller-owned, like BhTrainState.  features / m1 / m2 are device [n, channels] f32 each; the moments start at
 * zero with step = 0. */
typedef struct BhFeatureField {
    float *features, *m1, *m2;
    uint32_t n, channels;            /* channels: 1 .. BH_FEATURE_MAX_CHANNELS */
    uint32_t step;                   /* Adam updates applied so far; the next one uses t = step + 1 */
    float lr, beta1, beta2, eps;
    uint32_t reserved;
} BhFeatureField;

#ifdef __cplusplus
static_assert(sizeof(BhFeatureField) == 56, "BhFeatureField layout");
#else
_Static_assert(sizeof(BhFeatureField) == 56, "BhFeatureField layout");
#endif

/* Attaches a field and a target to the ctx's train steps (sticky, like bh_train_set_depth; both structs are host memory and are
 * copied).  field == NULL detaches both.  target == NULL, or one whose weight is <= 0 or not a number: no term — such a step launches
 * nothing new and touches neither the field nor its step count.
 *
 * A step with the term, on its final frame (behind a possible second attempt) and behind the distortion term: the feature map of
 * `features` is blended ONCE, the fused loss of `target` is added to the step's loss in f32 (order: image (+ LPIPS, + TV), depth,
 * normal, distortion, feature), the step's ONE backward carries the term — its gradient into the splats joins the colour term's
 * before the update — and v_features [n, channels] is left dense in a ctx slot.  With a gradient hook or a communicator v_features
 * is summed by one more "sum `count` floats at `p`" call (n * channels floats, behind the gradient exchange), then features / m1 / m2
 * take one Adam step with t = step + 1 on grad_scale * v_features (the arithmetic of bh_adam_step with the full second moment).  The
 * library's copy of `step` advances with every successful step that applied the term; a new call replaces the copy.  A frame that
 * lists nothing: the map is all +0, the loss is still evaluated, v_features is all +0 and the update still runs (Adam moves on its
 * moments).
 *
 * Refused by bh_train_step before anything is queued (BH_ERR_INVALID_ARG, the text names the feature term): a tile-row window or an
 * image hook; an attached pose-gradient buffer; field.n != state->n (the carry below was forgotten after a refine); a target whose
 * h, w differ from the camera's.
 *
 * BH_ERR_INVALID_ARG here: a null pointer inside a non-null field; channels == 0 or > BH_FEATURE_MAX_CHANNELS; a target whose
 * channels differ from the field's, that has no target pointer, or whose loss kind is unknown. */
int bh_train_set_features(bh_ctx* ctx, const BhFeatureField* field /*host, or NULL*/, const BhFeatureTarget* target /*host, or NULL*/);

/* Carries the rows of a per-splat table [N, channels] f32 through the pending refine plan: valid after bh_refine_plan and before the
 * bh_refine_apply that consumes it (BH_ERR_STATE otherwise); N is the planned state's n, `out` has the plan's total_splats rows.
 * For every old row i the plan keeps: out[new_row[i]] = in[i]; if the plan splits it as well: out[n_keep + child_slot[i]] = in[i].
 * Every row of `out` is written exactly once: no atomics, the same bits on every call.  Queued on the ctx stream; no readback.
 * BH_ERR_INVALID_ARG for a null pointer, channels == 0 or > 4096 and an unknown mode.  `out` may not alias `in`. */
#define BH_CARRY_COPY       0u   /* kept rows gathered in order; a split parent's row goes to the parent's new row AND to its child */
#define BH_CARRY_ZERO_SPLIT 1u   /* kept unsplit rows gathered; both halves of a split are +0 (what refine does to Adam moments) */
#define BH_CARRY_MAX_CHANNELS 4096u
int bh_refine_carry_rows(bh_ctx* ctx, const float* in /*[N,channels]*/, float* out /*[total_splats,channels]*/, uint32_t channels, uint32_t mode);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_FEATURE_TRAIN_H */
