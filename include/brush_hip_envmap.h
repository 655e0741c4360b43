/* brush_hip_envmap.h — environment maps: a learned cubemap behind the splats (the "sky" of splatfacto-w, Street Gaussians and other
 * outdoor trainers; gsplat's per-pixel `backgrounds`), composited behind a rendered frame, with its gradient, its Adam moments and
 * the update itself on the device, and a term in bh_train_step.  DESIGN.md §6v has the whole contract.
 *
 * Same conventions as brush_hip.h: 0 on success, <0 on error (bh_last_error), device pointers unless marked host.  Every call is
 * queued on the ctx stream; the bh_envmap_get_* calls read back (they synchronise the stream), and so does bh_envmap_backward for
 * its one refusal that depends on data (below).  A NULL pointer, an image side of zero, h * w >= 2^31 or a camera that is not a
 * pinhole is BH_ERR_INVALID_ARG and leaves the map untouched.
 *
 * A map is E[6, R, R, 3] f32: six faces of R x R texels of linear rgb, unclamped, 1 <= R <= 1024.  The arithmetic below is the
 * specification: tests/envmap_ref.py restates it in numpy and the kernels reproduce it bit for bit (the library is built with
 * -ffp-contract=off: every fma below is one, nothing else is fused; / and sqrt are correctly rounded).  All of it is f32 unless
 * marked.
 *
 *   ray of pixel (x, y), pinhole only (the convention of the depth-map normals, brush_hip_normal.h), not normalised:
 *     dx = (((float)x + 0.5) - cx) / fx,   dy = (((float)y + 0.5) - cy) / fy              (d_cam = (dx, dy, 1))
 *     d_i = fma(vm[3i+1], dy, vm[3i] * dx) + vm[3i+2]      i = 0, 1, 2                    (d = R_wc^T d_cam: column i of BhCamera.vm)
 *   face: axis = 0; if |d_1| > |d_axis| axis = 1; if |d_2| > |d_axis| axis = 2 (ties go to the lower axis); major = d_axis;
 *     face = 2 axis + (major < 0), in world axes: +X, -X, +Y, -Y, +Z, -Z;
 *     (s, t) = (a, b) / |major| with (a, b) = (d_1, d_2) for X, (d_2, d_0) for Y, (d_0, d_1) for Z.
 *     This table is this library's own: there are no OpenGL flips, and a cubemap of another convention has to be re-laid.
 *   texel: u = fma(s, R/2, R/2) - 0.5, then u = min(max(u, 0), R - 1) (a NaN becomes 0); i0 = floor(u), i1 = min(i0 + 1, R - 1),
 *     fu = u - i0; v, j0, j1, fv likewise from t.  Taps k = 0..3 are the texels (i0,j0) (i1,j0) (i0,j1) (i1,j1) — texel (i, j) of
 *     face f is E[f, j, i, :] — with weights w_0 = (1-fu)(1-fv), w_1 = fu (1-fv), w_2 = (1-fu) fv, w_3 = fu fv.
 *     E_c(d) = fma(w_3, e_3c, fma(w_2, e_2c, fma(w_1, e_1c, w_0 e_0c))).
 *     Lookups clamp to the face's edge: the seam at a cube edge stays below one texel of blur.
 *   composite, with A = img_a:    out_c = fma(1 - A, E_c(d), img_c)   c = r, g, b;     out_a = A
 *   gradient to the frame, for a cotangent v_out on out:
 *     v_img_c = v_out_c;     v_img_a = v_out_a - (float)(v_out_b E'_b + (v_out_g E'_g + v_out_r E'_r))
 *     with the sum and E'_c = w_3 e_3c + (w_2 e_2c + (w_1 e_1c + w_0 e_0c)) in f64, every operation rounded on its own (a product
 *     w e of two f32 is exact there): the sky's term carries one f32 rounding, whatever the colours cancel
 *   gradient to the table: exact, free of the order of summation and the same from run to run — a sum of 64-bit integers:
 *     m = max |v_out_c| over every pixel and c = r, g, b;  e = the binary exponent of m (2^(e-1) <= m < 2^e);
 *     L = ceil(log2(h w));  S = 2^(61 - e - L);
 *     every (pixel with 1 - A != 0, channel c, tap k):  g = (1 - A) v_out_c,  q = llrint((double)(g w_k) S)  (half to even)
 *     v_E[texel of k, c] = (float)((double)(the sum of q, an int64) / S)
 *     H W 2^e S <= 2^61: the sum cannot overflow.  m = 0: v_E is all +0.  A texel no pixel reaches gets +0.
 *     A non-finite m (a NaN or an infinity in v_out's rgb): bh_envmap_backward returns BH_ERR_INVALID_ARG after the pass that
 *     found it (one 4-byte readback) and nothing is written: not v_img, not the gradient, no update.  (bh_train_step does not read
 *     back: there the same condition turns the term's kernels into no-ops on the device.)
 *   Adam on every texel, in f32, from the f32 moments m1, m2 and the step count t (host copies of t and of the two bias
 *   corrections go to the kernel by value; the device keeps t beside the moments for bh_envmap_get_state):
 *     t += 1;  c1 = (float)(1 - beta1^t),  c2 = (float)(1 - beta2^t)   (f64, the power by squaring: p = 1, b = beta; while t: if t & 1:
 *                                                                      p = p b;  b = b b;  t >>= 1)
 *     m1 = (float)beta1 m1 + (float)(1 - beta1) g;     m2 = (float)beta2 m2 + ((float)(1 - beta2) g) g
 *     E = E - (float)lr ((m1 / c1) / (sqrt(m2 / c2) + (float)eps))
 *   the bias correction of the bilateral grid's update (brush_hip_bilagrid.h).  A texel with g = 0 and zero moments does not move:
 *   0 / (0 + eps).
 *
 * Not built: fisheye and distorted cameras (no unprojection exists for them), a pose gradient with the term (the lookup depends on
 * the rotation), tile-partitioned frames, filtering across faces, mip levels, the map in bh_eval_view and in PLY export, several
 * maps per scene.
 */
#ifndef BRUSH_HIP_ENVMAP_H
#define BRUSH_HIP_ENVMAP_H

#include "brush_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bh_envmap bh_envmap;

#define BH_ENVMAP_MAX_RESOLUTION 1024u

/* A map of resolution 1 .. BH_ENVMAP_MAX_RESOLUTION, all zero (black: the frame composited over it is the frame), with zero moments
 * and count, lr = 1e-3, beta1 = 0.9, beta2 = 0.999, eps = 1e-15, on the ctx's device.  The ctx owns it: bh_destroy frees what
 * bh_envmap_destroy has not.  Destroying a map that is attached to the train step detaches it first. */
int bh_envmap_create(bh_ctx* ctx, uint32_t resolution, bh_envmap** map /*host*/);
int bh_envmap_destroy(bh_ctx* ctx, bh_envmap* map);

/* The whole table as 6 R R 3 host floats: checkpoints.  set_params leaves the moments and the count alone. */
int bh_envmap_set_params(bh_ctx* ctx, bh_envmap* map, const float* host /*[6,R,R,3]*/);
int bh_envmap_get_params(bh_ctx* ctx, bh_envmap* map, float* host /*[6,R,R,3]*/);
/* v_E of the last bh_envmap_backward (or train step) on the map; zeros before the first. */
int bh_envmap_get_grad(bh_ctx* ctx, bh_envmap* map, float* host /*[6,R,R,3]*/);
/* The Adam state; bh_envmap_set_state puts it back (resuming from a checkpoint). */
int bh_envmap_get_state(bh_ctx* ctx, bh_envmap* map, float* m1 /*host [6,R,R,3]*/, float* m2 /*host [6,R,R,3]*/, uint32_t* t /*host*/);
int bh_envmap_set_state(bh_ctx* ctx, bh_envmap* map, const float* m1 /*host [6,R,R,3]*/, const float* m2 /*host [6,R,R,3]*/, uint32_t t);

/* Held on the host and passed to every following update by value (call it when a schedule moves lr).  lr >= 0, 0 <= beta < 1,
 * eps > 0.  lr = 0 leaves the table bit for bit while moments and count still advance. */
int bh_envmap_set_adam(bh_ctx* ctx, bh_envmap* map, double lr, double beta1, double beta2, double eps);

/* out = img over the map, seen through `cam` (host; only vm, fx, fy, cx, cy and model are read: h and w are the arguments'); out may
 * equal img. */
int bh_envmap_composite(bh_ctx* ctx, bh_envmap* map, const BhCamera* cam /*host*/, const float* img_hwc4, uint32_t h, uint32_t w,
                        float* out_hwc4);
/* v_img = the gradient to the frame (v_img may equal v_out), the map's gradient = v_E of (img_hwc4's alpha, v_out), and — update
 * != 0 — one Adam step of the table on it.  img_hwc4 is the frame that was composited (its alpha is all that is read). */
int bh_envmap_backward(bh_ctx* ctx, bh_envmap* map, const BhCamera* cam /*host*/, const float* img_hwc4, const float* v_out, uint32_t h,
                       uint32_t w, float* v_img, int update);

/* Attaches the map to bh_train_step on this ctx: every following step composites its rendered frame (render it on a black
 * background) over the map before the loss — the LPIPS term, an exposure table or a bilateral grid then act on the composited
 * frame —, sends the gradient to the frame into the render backward (the sky pulls alpha down) and updates the table.  When the
 * step exchanges gradients (a hook or a communicator) v_E is summed over the ranks by one more call of the same kind, 6 R R 3
 * floats, and the update takes grad_scale times the sum.  A camera that is not a pinhole, a tile-row window or an image hook, a
 * pose-gradient buffer, or a target with real alpha (has_alpha without alpha_is_mask) fail with BH_ERR_INVALID_ARG before anything
 * is queued.  NULL detaches: the step is exactly as without, no launch. */
int bh_train_set_envmap(bh_ctx* ctx, bh_envmap* map /*NULL detaches*/);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_ENVMAP_H */
