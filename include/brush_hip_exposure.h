/* brush_hip_exposure.h — per-view exposure compensation: a learned affine colour transform per training view (the 3x4 exposure
 * matrix of the INRIA trainer, gsplat's app_opt), applied to the rasterizer's image before the loss, with its parameters, their
 * Adam moments and the update itself on the device.  DESIGN.md §6k has the whole contract.
 *
 * Same conventions as brush_hip.h: 0 on success, <0 on error (bh_last_error), device pointers unless marked host.  Every call is
 * queued on the ctx stream; only the bh_exposure_get_* calls read back (they synchronise the stream).  A bad view index, a NULL
 * pointer or an image side of zero is BH_ERR_INVALID_ARG and leaves the table untouched.
 *
 * A view's exposure is m[12] f32, row-major 3x4: m[4 r + c], r = output channel, c = input channel, c = 3 the offset.  On an
 * image x [h,w,4] f32 (the background already composited, as BhRenderOut.out_img):
 *   y_r = fma(m[4r], x_0, fma(m[4r+1], x_1, fma(m[4r+2], x_2, m[4r+3])))   r = 0, 1, 2;     y_3 = x_3
 * and for a cotangent v' on y:
 *   v_c = sum_r m[4r+c] v'_r   c = 0, 1, 2;   v_3 = v'_3;     v_m[4r+c] = sum_p v'_r(p) x_c(p),   v_m[4r+3] = sum_p v'_r(p)
 * The identity (1,0,0,0, 0,1,0,0, 0,0,1,0) returns x and v' unchanged.  v_m is summed in f64 (the products are exact there) in
 * a fixed order without atomics: the same x, v' and image size give the same twelve bits from run to run.
 *
 * A table holds V views: param [V,12] f32 (the identity at creation), grad [V,12] f32 (the last v_m written for the row), Adam
 * moments m1, m2 [V,12] f64 and a step count per row.  Views are numbered from 1 (row i is view id i + 1, as SceneLoader
 * numbers its views; 0 is "unknown view").  The update is plain Adam in f64 on the device, on the f64 sum g before it is rounded
 * into grad:
 *   t += 1;  m1 = b1 m1 + (1 - b1) g;  m2 = b2 m2 + (1 - b2) g^2;
 *   param = f32(param - lr (m1 / (1 - b1^t)) / (sqrt(m2 / (1 - b2^t)) + eps))
 * Only the row of the view that was rendered moves.
 *
 * Data parallel over cameras: a table belongs to one process and nothing in it is all-reduced, so a view must stay with one rank
 * (SceneLoader's split by rank does that).
 */
#ifndef BRUSH_HIP_EXPOSURE_H
#define BRUSH_HIP_EXPOSURE_H

#include "brush_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bh_exposure bh_exposure;

/* A table of n_views (> 0) identity rows with zero moments and counts, lr = 1e-3, beta1 = 0.9, beta2 = 0.999, eps = 1e-8, on the
 * ctx's device.  The ctx owns it: bh_destroy frees what bh_exposure_destroy has not.  Destroying a table that is attached to the
 * train step detaches it first. */
int bh_exposure_create(bh_ctx* ctx, uint32_t n_views, bh_exposure** table /*host*/);
int bh_exposure_destroy(bh_ctx* ctx, bh_exposure* table);

/* Rows first_view .. first_view + count - 1 (view ids, from 1) as count * 12 host floats: checkpoints.  set_params leaves the
 * rows' moments and counts alone. */
int bh_exposure_set_params(bh_ctx* ctx, bh_exposure* table, uint32_t first_view, uint32_t count, const float* host /*[count,12]*/);
int bh_exposure_get_params(bh_ctx* ctx, bh_exposure* table, uint32_t first_view, uint32_t count, float* host /*[count,12]*/);
int bh_exposure_get_grad(bh_ctx* ctx, bh_exposure* table, uint32_t first_view, uint32_t count, float* host /*[count,12]*/);
/* One row's Adam state; bh_exposure_set_state puts it back (resuming from a checkpoint). */
int bh_exposure_get_state(bh_ctx* ctx, bh_exposure* table, uint32_t view, double* m1 /*host [12]*/, double* m2 /*host [12]*/,
                          uint32_t* t /*host*/);
int bh_exposure_set_state(bh_ctx* ctx, bh_exposure* table, uint32_t view, const double* m1 /*host [12]*/,
                          const double* m2 /*host [12]*/, uint32_t t);

/* Held on the host and passed to every following update by value (call it when a schedule moves lr).  lr >= 0, 0 <= beta < 1,
 * eps > 0.  lr = 0 leaves param bit for bit while moments and counts still advance. */
int bh_exposure_set_adam(bh_ctx* ctx, bh_exposure* table, double lr, double beta1, double beta2, double eps);

/* out = y(img) with the row of `view`; out may equal img. */
int bh_exposure_apply(bh_ctx* ctx, bh_exposure* table, uint32_t view, const float* img_hwc4, uint32_t h, uint32_t w, float* out_hwc4);
/* v_img = v(v_exposed) with the row of `view` as it is when the call is queued on the device, grad[view] = v_m of (img_hwc4,
 * v_exposed), and — update != 0 — one Adam step of param[view] on it.  v_img may equal v_exposed. */
int bh_exposure_backward(bh_ctx* ctx, bh_exposure* table, uint32_t view, const float* img_hwc4, const float* v_exposed, uint32_t h,
                         uint32_t w, float* v_img, int update);

/* Attaches the table to bh_train_step on this ctx: every following step applies the row of batch->view_id to its rendered frame
 * before the loss (and the LPIPS term), sends A^T v' into the render backward (and the pose gradient, if attached) and updates
 * that row.  batch->view_id == 0 or > n_views, a tile-row window or an image hook fail with BH_ERR_INVALID_ARG before anything is
 * queued: the term needs the whole frame on this rank.  NULL detaches: the step is exactly as without, no launch. */
int bh_train_set_exposure(bh_ctx* ctx, bh_exposure* table /*NULL detaches*/);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_EXPOSURE_H */
