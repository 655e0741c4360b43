/* brush_hip_compressed_ply.h — SuperSplat / PlayCanvas "compressed.ply" export of libbrush_hip.so: the format the library
 * already reads (bh_splats_from_ply, BhPlyInfo.compressed; the reference's import.rs:407-600 and quant.rs), written on the GPU.
 *
 * Same conventions as brush_hip.h: 0 on success, <0 on error (bh_last_error), device pointers unless marked host.
 *
 * File (DESIGN.md §6g has the whole contract): binary_little_endian, the comment lines of bh_splat_to_ply's header, then
 *   element chunk ceil(n / 256)   18 float: min_x min_y min_z max_x max_y max_z, min_scale_x..z max_scale_x..z, min_r..b max_r..b
 *   element vertex n              4 uint: packed_position (11-10-11) packed_rotation (2-10-10-10) packed_scale (11-10-11) packed_color (8-8-8-8)
 *   element sh n                  3K uchar f_rest_0 .. f_rest_{3K-1}, [channel][coeff] order, K = (d+1)^2 - 1 (absent when d = 0)
 * Rows are in Morton order of a 10-bit cell grid over the finite position box (a stable sort: equal cells keep input order); each
 * chunk of 256 file rows quantises position, log-scale and colour against its own ranges of finite values.  Body bytes:
 * 72 ceil(n/256) + 16 n + 3K n.
 */
#ifndef BRUSH_HIP_COMPRESSED_PLY_H
#define BRUSH_HIP_COMPRESSED_PLY_H

#include "brush_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Protocol of bh_splat_to_ply: *written = bytes of the file; out == NULL is a size query (launches nothing, reads no tensor);
 * cap < *written is BH_ERR_INVALID_ARG; sh_degree 0..4; n == 0 writes a header with zero-count elements.  min_scale (device [n]
 * or NULL): the 3D-filter floor is baked first, as bh_splat_to_ply does.  order (device [n] or NULL): file row -> input row.
 * Returns after the body has been copied into out. */
int bh_splat_to_compressed_ply(bh_ctx* ctx, const float* transforms, const float* sh_coeffs, const float* raw_opacities, const float* min_scale,
                               uint32_t n, uint32_t sh_degree, int render_mip, const float* up_axis /*host [3] or NULL*/,
                               uint32_t* order /*optional device [n]: file row -> input row*/, void* out /*host*/, uint64_t cap,
                               uint64_t* written /*host*/);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_COMPRESSED_PLY_H */
