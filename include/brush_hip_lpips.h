/* brush_hip_lpips.h — LPIPS (VGG16 perceptual distance) of libbrush_hip.so: the reference's LpipsModel::lpips
 * (crates/lpips/src/lib.rs) and the lpips_loss_weight term of SplatTrainer::step (brush-train/src/config.rs:92,
 * train.rs:153, 265-273), forward and data gradient on the GPU in exact f32 (f32-input MFMA, no 16-bit operands).
 *
 * Same conventions as brush_hip.h: 0 on success, <0 on error (bh_last_error), device pointers unless marked host,
 * asynchronous on the ctx stream.
 *
 * Parameters, canonical order (BH_LPIPS_PARAM_COUNT floats, host): the 13 convs in forward order (blocks of 2, 2, 3, 3, 3
 * convs, 3 -> 64 -> 64 | 128 128 | 256 256 256 | 512 512 512 | 512 512 512 channels), each as weight [Cout][Cin][3][3]
 * (OIHW) then bias [Cout] (14,714,688 floats); then the 5 bias-free 1x1 heads, [C] each, C = 64, 128, 256, 512, 512
 * (1,472 floats).
 *
 * Device memory, counted from the shapes (not measured; P = h * w): bh_lpips_value_and_grad and the train step's term keep
 * pred's 13 conv outputs, its 4 pooled block inputs, GT's 5 block outputs and two P x 64 scratch / gradient buffers, about
 * 556 P floats: 4.6 GB at 1920x1080, 18.4 GB at 3840x2160.  bh_lpips_forward keeps the 5 block outputs of each image and the
 * two buffers, about 378 P floats (3.1 GB at 1080p).  The scratch is the ctx's arena (grow-only); the model itself holds two
 * packings of the weights, 118 MB.
 */
#ifndef BRUSH_HIP_LPIPS_H
#define BRUSH_HIP_LPIPS_H

#include "brush_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_LPIPS_PARAM_COUNT 14716160u

typedef struct bh_lpips bh_lpips;

/* Upload and repack `count` (== BH_LPIPS_PARAM_COUNT, else BH_ERR_INVALID_ARG and NULL) canonical parameters onto the
 * ctx's device.  Blocking.  The model may be used by any ctx on the same device. */
bh_lpips* bh_lpips_create(bh_ctx* ctx, const float* params /*host*/, uint64_t count);
void bh_lpips_destroy(bh_lpips* model);

/* value[0] = LPIPS(img_hwc4 rgb, unpack_gt_rgb(gt_packed, composite_bg)).  img_hwc4 [h,w,4] f32 (alpha ignored, 16-byte
 * aligned); gt_packed [h,w] rgba8; composite_bg host [3] or NULL: GT rgb + (1 - a) * bg.  h, w >= 16 (block 5 has a pixel).
 * Does not block. */
int bh_lpips_forward(bh_ctx* ctx, const bh_lpips* model, const float* img_hwc4, const uint32_t* gt_packed, uint32_t h, uint32_t w,
                     const float* composite_bg /*host [3] or NULL*/, float* value);
/* As bh_lpips_forward, and v_output [h,w,4] += weight * dLPIPS/dimg on rgb (alpha untouched).  value is LPIPS unweighted. */
int bh_lpips_value_and_grad(bh_ctx* ctx, const bh_lpips* model, const float* img_hwc4, const uint32_t* gt_packed, uint32_t h, uint32_t w,
                            const float* composite_bg /*host [3] or NULL*/, float weight, float* value, float* v_output);

/* Attach (model, weight > 0) the lpips_loss_weight term to bh_train_step on this ctx: the step adds weight * LPIPS(frame rgb,
 * GT composited with the step's own background when train.rs would) to the loss and stats->loss, and its gradient to dL/dimg
 * before the render backward.  NULL or weight 0: the step is exactly as without.  A step with a tile-row partition (image
 * hook, strips over ranks, or any tile-row window) and a non-zero weight fails with BH_ERR_INVALID_ARG.  The model must
 * outlive its attachment. */
int bh_train_set_lpips(bh_ctx* ctx, const bh_lpips* model /*NULL detaches*/, float weight);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_LPIPS_H */
