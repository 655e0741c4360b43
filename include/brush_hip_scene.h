/* brush_hip_scene.h — scene editing: a similarity transform of a splat scene (means, rotations, scales, the 3D-filter floor and the
 * spherical harmonics of degree >= 1, which are expressed in world axes and have to turn with the scene), the same transform of a
 * camera, and a region select (oriented box or ellipsoid, an opacity floor) whose output bh_decimate_to_count compacts.
 * DESIGN.md §6t has the whole contract.
 *
 * Same conventions as brush_hip.h: 0 on success, <0 on error (bh_last_error), device pointers unless marked host; a null ctx returns
 * BH_ERR_INVALID_ARG before the device is touched.  The four record / camera functions are host arithmetic in f64: no ctx, no device.
 *
 * The map is x' = s R x + t with R a proper rotation and s > 0.  The transformed scene rendered from the transformed camera is the
 * image of the original scene from the original camera: camera-space coordinates are s times the old ones, which no lens model of
 * brush_hip.h sees (all four project x/z, y/z or the angle of the ray).
 */
#ifndef BRUSH_HIP_SCENE_H
#define BRUSH_HIP_SCENE_H

#include "brush_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Filled by bh_scene_transform_make / _compose / _invert only: the f64 fields are the transform, every f32 field is derived from them
 * and is what the kernel reads. */
typedef struct BhSceneTransform {
    double q[4];        /* unit quaternion (w,x,y,z) of R, w >= 0 */
    double t[3];
    double s;
    float rot[9];       /* R row-major, (float) of the f64 matrix of q */
    float quat[4];      /* (float) q */
    float trans[3];
    float scale;
    float log_scale;    /* (float) ln s */
    float sh_rot[164];  /* D_1 3x3 at 0, D_2 5x5 at 9, D_3 7x7 at 34, D_4 9x9 at 83, row-major */
    uint32_t reserved[2];
} BhSceneTransform;

#define BH_REGION_BOX 0u
#define BH_REGION_ELLIPSOID 1u

typedef struct BhSceneRegion {
    uint32_t kind;         /* BH_REGION_BOX (oriented box) or BH_REGION_ELLIPSOID */
    uint32_t invert;       /* != 0: keep what the geometric test rejects */
    float center[3];
    float half_extent[3];  /* > 0 */
    float rot[9];          /* row-major, region axes in world: column i is axis i */
    float min_raw_opacity; /* -inf: none */
    uint32_t reserved;     /* 0 */
} BhSceneRegion;

#ifdef __cplusplus
static_assert(sizeof(BhSceneTransform) == 800, "BhSceneTransform layout");
static_assert(sizeof(BhSceneRegion) == 76, "BhSceneRegion layout");
#else
_Static_assert(sizeof(BhSceneTransform) == 800, "BhSceneTransform layout");
_Static_assert(sizeof(BhSceneRegion) == 76, "BhSceneRegion layout");
#endif

/* Host only, f64.  The record of x' = scale * R(quat) x + trans; the quaternion is normalised here (and negated when w < 0).
 * sh_rot: D_l is defined by its effect — with a' = D_l a per band and channel, sum_k a'_k Y_k(d) = sum_k a_k Y_k(R^T d) for every unit d,
 * Y the basis of the renderer (its constants and signs) taken in f64; all four bands are always filled.
 * BH_ERR_INVALID_ARG (out untouched) for a null argument, a zero or non-finite quaternion, a non-finite translation, or a scale
 * that is not a finite number > 0. */
int bh_scene_transform_make(const double quat_wxyz[4] /*host*/, const double trans[3] /*host*/, double scale, BhSceneTransform* out /*host*/);

/* Host only, f64, from the f64 fields; every field of out is refilled (out may be a or b).  compose: out = a after b (b is applied
 * first).  invert: out undoes a.  BH_ERR_INVALID_ARG for a null argument or a record whose f64 fields are no transform (also: a
 * product whose scale leaves the finite numbers > 0). */
int bh_scene_transform_compose(const BhSceneTransform* a /*host*/, const BhSceneTransform* b /*host*/, BhSceneTransform* out /*host*/);
int bh_scene_transform_invert(const BhSceneTransform* a /*host*/, BhSceneTransform* out /*host*/);

/* Host only, f64.  The camera that sees the transformed scene as `in` saw the original: with W, tv of vm and p = cam_pos,
 * W' = W R^T, tv' = s tv - W R^T t, cam_pos' = s R p + t; everything else is copied (out may be in). */
int bh_camera_apply_scene_transform(const BhCamera* in /*host*/, const BhSceneTransform* T /*host*/, BhCamera* out /*host*/);

/* The scene moved by T.  transforms [N,10] (means, quaternion wxyz, log-scales), sh_coeffs [N,num_coeffs,3] or NULL (then out_sh is
 * ignored), min_scale [N] or NULL (then out_min_scale is ignored); num_coeffs in {1,4,9,16,25}.  Opacities do not change.
 * Each output either IS its input (in place) or must not overlap it; an output that overlaps any other argument is refused too
 * (BH_ERR_INVALID_ARG before a launch, nothing written).  n == 0 launches nothing.  An identity record (q = (1,0,0,0), t = 0, s = 1)
 * is a copy, or nothing in place: the output bits are the input bits.
 * f32, every multiply and add rounded on its own (no fma), in this order, from the record's f32 fields:
 *   mean'_i = ((rot[3i] x + rot[3i+1] y) + rot[3i+2] z) * scale + trans_i
 *   quaternion' = quat (x) q, the Hamilton product, unnormalised like the input:
 *     w' = ((W w - X x) - Y y) - Z z     x' = ((W x + X w) + Y z) - Z y     y' = ((W y - X z) + Y w) + Z x     z' = ((W z + X y) - Y x) + Z w
 *   log_scale'_i = log_scale_i + log_scale        min_scale' = min_scale * scale
 *   SH: row 0 is copied; band l: out[l^2+k][c] = sum_j D_l[k][j] in[l^2+j][c], j ascending: the first product, then one multiply and one
 *   add per term.
 * A row with a non-finite entry gives what IEEE gives in its own outputs and disturbs no other row.
 * Base pointers need only the 4-byte alignment of a float; 16-byte aligned ones take 16-byte loads and stores.
 * Queued on the ctx stream: no readback, no scratch. */
int bh_splats_transform(bh_ctx* ctx, const BhSceneTransform* T /*host*/, uint32_t n, uint32_t num_coeffs, const float* transforms,
                        const float* sh_coeffs /*or NULL*/, const float* min_scale /*or NULL*/, float* out_transforms /*[N,10]*/,
                        float* out_sh /*[N,num_coeffs,3]*/, float* out_min_scale /*[N]*/);

/* keep [N] = 1.0f where the splat is selected, 0.0f elsewhere: what bh_decimate_to_count takes as scores — that call with
 * target_count = *count is the stable compaction (ties keep ascending index).
 *   d_i = mean_i - center_i,   p_i = ((rot[i] dx + rot[3+i] dy) + rot[6+i] dz)     (the point in the region's frame, f32, no fma)
 *   box: |p_i| <= half_extent_i for all i        ellipsoid: ((p_0/h_0)^2 + (p_1/h_1)^2) + (p_2/h_2)^2 <= 1   (true divides)
 * invert flips the geometric test.  Whatever invert says: a non-finite mean is never kept, and with raw_opacities given neither is a
 * splat whose raw opacity is below min_raw_opacity or NaN.
 * count (host, nullable): the number of kept splats, an integer reduction in a fixed order (no atomics); when given the call blocks
 * until it is there.  BH_ERR_INVALID_ARG for a null argument, an unknown kind, a half extent that is not a finite number > 0, a
 * centre or axis that is not finite, or a NaN floor. */
int bh_splats_select_region(bh_ctx* ctx, const BhSceneRegion* region /*host*/, const float* transforms, const float* raw_opacities /*or NULL*/,
                            uint32_t n, float* keep /*[N]*/, uint32_t* count /*host, or NULL*/);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_SCENE_H */
