/* brush_hip_image.h — the image half of the reference's LoadImage::load (brush-dataset/src/load_image.rs:60-131) on the GPU:
 * mask merge, resampling to the training resolution, then the packing of view_to_packed_data, in the upload ring of
 * brush_hip.h (bh_uploader_*), plus the resampling operator on its own.
 *
 * Same conventions as brush_hip.h: 0 on success, <0 on error (bh_last_error / bh_uploader_last_error), device pointers unless
 * marked host.
 *
 * Resampling is image::imageops::resize of the image crate 0.25, restated exactly (DESIGN.md §6h has the whole contract): a
 * vertical pass into an f32 intermediate, then a horizontal pass back to u8; per pass, output o reads source taps
 * [left, right) around c = (o + 0.5) * src / dst with weights k((i - c + 0.5) / max(src / dst, 1)) normalised by their sum;
 * t = t + v * w per tap in f32 without FMA; round half away from zero after a clamp to [0, 255].  The weight tables are
 * computed on the host (f32, the C library's sinf) and uploaded with the launch, so the result is bit-exact.  The same size
 * is a copy.  Alpha is filtered like any other channel.
 */
#ifndef BRUSH_HIP_IMAGE_H
#define BRUSH_HIP_IMAGE_H

#include "brush_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_FILTER_LANCZOS3 0u /* image::imageops::FilterType::Lanczos3 (support 3) */
#define BH_FILTER_TRIANGLE 1u /* FilterType::Triangle (support 1) */

/* One view for bh_uploader_commit_view.  The slot (bh_uploader_begin) holds the decoded image at byte 0, rows tight, RGB8 or
 * RGBA8; with a mask, mask_w * mask_h bytes of one channel at mask_offset (the caller reduces an RGBA mask to its alpha and a
 * colour mask to luma, load_image.rs:84-92).  Image plus mask must fit the slot's 4 * max_pixels bytes: an RGBA view with a
 * full-size mask needs max_pixels >= 1.25 x its pixel count. */
typedef struct BhViewLoad {
    uint32_t w, h, channels;     /* source image: channels 3 or 4 */
    uint32_t mask_w, mask_h;     /* 0 x 0: no mask.  Another size than w x h is Triangle-resized to it first */
    int32_t invert_mask;         /* alpha = 255 - mask (LoadDatasetConfig invert_masks) */
    uint64_t mask_offset;        /* byte offset of the mask in the slot, >= w * h * channels */
    uint32_t max_resolution;     /* long-edge cap (config.rs default 1920); 0: no cap */
    float scale;                 /* LOD image scale (LoadImage::with_scale), > 0 */
    int32_t premultiply;         /* AlphaMode::Transparent: premultiply when the view has alpha */
    uint32_t reserved;           /* must be 0 (else BH_ERR_INVALID_ARG), for a later meaning */
} BhViewLoad;

/* LoadImage::output_scale and the size load() resizes to (host only): cap = max / max(w, h, max) in f32, s = min(cap * scale,
 * 1); s < 1 gives each side as (uint32)max(side * s, 1), else the size is unchanged.  max_resolution 0: cap = 1.  w, h > 0,
 * scale finite and > 0, else BH_ERR_INVALID_ARG. */
int bh_view_output_size(uint32_t w, uint32_t h, uint32_t max_resolution, float scale, uint32_t* out_w /*host*/, uint32_t* out_h /*host*/);

/* dst [nh][nw][channels] = resize(src [h][w][channels], nw, nh, filter), channels 1, 3 or 4, on the ctx stream.  The weight
 * tables (the same cache as bh_uploader_commit_view's) travel through pinned memory; the f32 intermediate (w * nh * channels
 * floats) is the ctx's arena.  Does not block unless the arena grows or the previous call's tables have not reached the device
 * yet.  src and dst must not overlap. */
int bh_resize_u8(bh_ctx* ctx, const uint8_t* src, uint32_t w, uint32_t h, uint32_t channels, uint8_t* dst, uint32_t nw, uint32_t nh,
                 uint32_t filter);

/* bh_uploader_commit for a decoded view: on the copy stream, the H2D copy of image and mask, the mask merge (Triangle resize of
 * the mask to w x h when its size differs; alpha = mask or 255 - mask; the view becomes RGBA), the Lanczos3 resize to
 * bh_view_output_size, and the pack of view_to_packed_data.  bh_uploader_acquire then returns the output size, and has_alpha is
 * true for RGBA input or a merged mask.  w * h <= max_pixels.  The resample scratch is the uploader's, shared by its slots and
 * grown on demand (the copy stream orders them).  The weight tables come from a process-wide cache keyed by (source size, output
 * size, filter), built on the calling thread on a miss and before the ring's lock is taken. */
int bh_uploader_commit_view(bh_uploader* up, int slot, const BhViewLoad* desc /*host*/);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_IMAGE_H */
