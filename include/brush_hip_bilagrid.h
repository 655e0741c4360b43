/* brush_hip_bilagrid.h — per-view bilateral grids: a learned, spatially and tonally varying affine colour transform per training view
 * ("Bilateral Guided Radiance Field Processing"; gsplat's lib_bilagrid behind --use_bilateral_grid), sliced on the rasterizer's image
 * before the loss, with the grids, their Adam moments and the update itself on the device.  It is the exposure table
 * (brush_hip_exposure.h) with a matrix that varies over (x, y, luminance).  DESIGN.md §6p has the whole contract.
 *
 * Same conventions as brush_hip.h: 0 on success, <0 on error (bh_last_error), device pointers unless marked host.  Every call is
 * queued on the ctx stream; only the bh_bilagrid_get_* calls read back (they synchronise the stream; so do create, set_params and
 * set_state, which hand over host arrays of up to megabytes and return once those may be freed).  A bad view index, a NULL
 * pointer or an image side of zero is BH_ERR_INVALID_ARG and leaves the table untouched.
 *
 * A view's grid is g[Hg][Wg][L][12] f32, the coefficient index fastest; the twelve coefficients are a row-major 3x4 matrix m[4 r + c]
 * (r = output channel, c = input channel, c = 3 the offset), as in brush_hip_exposure.h.  The identity grid holds
 * (1,0,0,0, 0,1,0,0, 0,0,1,0) in every cell.  Hg, Wg, L >= 1 (gsplat's defaults: 16, 16, 8).  gsplat's tensor grids[v, k, l, j, i] is
 * this g[j][i][l][k].
 *
 * For pixel (px, py) of an image x [h,w,4] f32 (the background already composited, as BhRenderOut.out_img) the coordinates are f32,
 * every operation rounded on its own (no contraction), so that a float32 restatement reproduces them bit for bit:
 *   fx  = (float(px) + 0.5f) * sx,   sx = float(Wg-1) / float(w)        (sx, sy computed once on the host in f32)
 *   fy  = (float(py) + 0.5f) * sy,   sy = float(Hg-1) / float(h)
 *   lum = (x0*0.299f + x1*0.587f) + x2*0.114f
 *   fz  = min(max(lum, 0), 1) * float(L-1)
 *   i0 = min(floor(fx), max(Wg-2, 0)),  i1 = min(i0+1, Wg-1),  tx = fx - i0      (likewise j0, j1, ty from fy and l0, l1, tz from fz)
 * which is grid_sample(mode="bilinear", align_corners=True, padding_mode="border") at gsplat's pixel-centre coordinates: x and y
 * never leave the grid, only z clamps.  Forward:
 *   A(p) = sum over the 8 corners of w_y w_x w_z g[j][i][l][:]           (weights 1 - t and t)
 *   y_r = A[4r] x_0 + A[4r+1] x_1 + A[4r+2] x_2 + A[4r+3]   r = 0, 1, 2;     y_3 = x_3
 * A is evaluated in f32 as nested interpolations along z, then x, then y, each anchored at the nearer vertex: a + s (b - a) with
 * s = min(t, 1 - t) <= 1/2.  Equal vertices interpolate exactly, so a constant grid is reproduced bit for bit: the identity grid
 * returns x and, for a luminance strictly inside (0, 1), v' unchanged.
 * For a cotangent v' on y, with o[4r+k] = v'_r x_k (x_3 taken as 1 in o):
 *   v_g[j][i][l][q] = sum_p w(p; j,i,l) o_q(p)
 *   v_c = sum_r A[4r+c] v'_r + lumcoef_c (L-1) inside sum_q (dA_q/dfz) o_q   c = 0, 1, 2;     v_3 = v'_3
 * dA/dfz is the same 8-corner sum with -1 and +1 in place of 1 - tz and tz; inside = (lum > 0 && lum < 1): no gradient through a
 * clamped coordinate (torch's border rule).  v_g is summed in f64 in a fixed order without atomics: the same x, v', image size and
 * grid size give the same bits from run to run, in place or out of place, and a vertex no pixel reaches gets an exact zero.
 *
 * Total variation of one view's grid (gsplat's total_variation_loss with a batch of one):
 *   TV = sum over d in {z, y, x} of sum (g[+1 along d] - g)^2 / count_d,   count_d = the number of such differences over all twelve
 * coefficients; a dimension of size 1 contributes 0.  Its gradient is the exact derivative.  Deviation from gsplat, which regularises
 * every view's grid on every step: only the rendered view's grid is regularised here, because only that row moves.
 *
 * A table holds V views: param [V,Hg,Wg,L,12] f32 (the identity at creation), grad of the same shape (the last gradient written for
 * the row, the TV term's included), Adam moments m1, m2 of the same shape in f32 and a step count per row.  Views are numbered from 1
 * (0 is "unknown view").  The update is Adam in f64 on the f64 gradient sum g before it is rounded into grad:
 *   t += 1;  a = b1 m1 + (1 - b1) g;  b = b2 m2 + (1 - b2) g^2;  m1 = f32(a);  m2 = f32(b)
 *   param = f32(param - lr (a / (1 - b1^t)) / (sqrt(b / (1 - b2^t)) + eps))           (a, b unrounded)
 * Only the row of the view that was rendered moves.  Data parallel over cameras: a table belongs to one process and nothing in it is
 * all-reduced, so a view must stay with one rank.
 */
#ifndef BRUSH_HIP_BILAGRID_H
#define BRUSH_HIP_BILAGRID_H

#include "brush_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bh_bilagrid bh_bilagrid;

/* A table of n_views (> 0) identity grids of grid_h x grid_w x grid_l cells (each 1 .. 1024, at most 2^22 floats per view) with zero
 * moments and counts, lr = 2e-3, beta1 = 0.9, beta2 = 0.999, eps = 1e-15 (gsplat's), on the ctx's device.  The ctx owns it: bh_destroy
 * frees what bh_bilagrid_destroy has not.  Destroying a table that is attached to the train step detaches it first. */
int bh_bilagrid_create(bh_ctx* ctx, uint32_t n_views, uint32_t grid_w, uint32_t grid_h, uint32_t grid_l, bh_bilagrid** table /*host*/);
int bh_bilagrid_destroy(bh_ctx* ctx, bh_bilagrid* table);
/* n_views, grid_w, grid_h, grid_l of a table; any out pointer may be NULL. */
int bh_bilagrid_dims(bh_ctx* ctx, bh_bilagrid* table, uint32_t* n_views /*host*/, uint32_t* grid_w /*host*/, uint32_t* grid_h /*host*/,
                     uint32_t* grid_l /*host*/);

/* Rows first_view .. first_view + count - 1 (view ids, from 1) as count * Hg Wg L 12 host floats: checkpoints.  set_params leaves the
 * rows' moments and counts alone. */
int bh_bilagrid_set_params(bh_ctx* ctx, bh_bilagrid* table, uint32_t first_view, uint32_t count, const float* host);
int bh_bilagrid_get_params(bh_ctx* ctx, bh_bilagrid* table, uint32_t first_view, uint32_t count, float* host);
int bh_bilagrid_get_grad(bh_ctx* ctx, bh_bilagrid* table, uint32_t first_view, uint32_t count, float* host);
/* One row's Adam state (m1, m2: Hg Wg L 12 host floats each); bh_bilagrid_set_state puts it back (resuming from a checkpoint). */
int bh_bilagrid_get_state(bh_ctx* ctx, bh_bilagrid* table, uint32_t view, float* m1 /*host*/, float* m2 /*host*/, uint32_t* t /*host*/);
int bh_bilagrid_set_state(bh_ctx* ctx, bh_bilagrid* table, uint32_t view, const float* m1 /*host*/, const float* m2 /*host*/, uint32_t t);

/* Held on the host and passed to every following update by value (call it when a schedule moves lr).  lr >= 0, 0 <= beta < 1,
 * eps > 0.  lr = 0 leaves param bit for bit while moments and counts still advance. */
int bh_bilagrid_set_adam(bh_ctx* ctx, bh_bilagrid* table, double lr, double beta1, double beta2, double eps);

/* out = y(img) with the grid of `view`; out may equal img.  h * w < 2^31. */
int bh_bilagrid_slice(bh_ctx* ctx, bh_bilagrid* table, uint32_t view, const float* img_hwc4, uint32_t h, uint32_t w, float* out_hwc4);
/* v_img = v(v_sliced) with the grid of `view` as it is when the call is queued on the device, grad[view] = v_g of (img_hwc4,
 * v_sliced) + tv_weight dTV/dg (tv_weight >= 0), and — update != 0 — one Adam step of param[view] on it.  v_img may equal v_sliced. */
int bh_bilagrid_backward(bh_ctx* ctx, bh_bilagrid* table, uint32_t view, const float* img_hwc4, const float* v_sliced, uint32_t h, uint32_t w,
                         float* v_img, float tv_weight, int update);
/* value_dev[0] = TV of the grid of `view` (an f64 sum in a fixed order, rounded to f32); nothing is read back. */
int bh_bilagrid_tv(bh_ctx* ctx, bh_bilagrid* table, uint32_t view, float* value_dev);

/* Attaches the table to bh_train_step on this ctx: every following step slices its rendered frame with the grid of batch->view_id
 * before the loss (and the LPIPS term), adds tv_weight TV(grid) to the loss (tv_weight >= 0; 0 = no term, no launch), sends v_img into
 * the render backward (and the pose gradient, if attached) and updates that grid.  batch->view_id == 0 or > n_views, a tile-row
 * window, an image hook or an exposure table attached at the same time (the two are alternatives) fail with BH_ERR_INVALID_ARG before
 * anything is queued.  NULL detaches: the step is exactly as without, no launch. */
int bh_train_set_bilagrid(bh_ctx* ctx, bh_bilagrid* table /*NULL detaches*/, float tv_weight);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_BILAGRID_H */
