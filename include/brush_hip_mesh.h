/* brush_hip_mesh.h — mesh extraction: fusion of depth maps into a truncated signed distance field (TSDF; KinectFusion, Open3D's
 * ScalableTSDFVolume rule on a dense grid), its zero level set by marching tetrahedra, and a triangle-mesh PLY — the last stage of the
 * 2DGS / GOF / PGSR / RaDe-GS pipelines the depth, normal and distortion operators serve, on the GPU.  DESIGN.md §6q has the whole
 * contract.
 *
 * Same conventions as brush_hip.h: 0 on success, <0 on error (bh_last_error), device pointers unless marked host; a null ctx returns
 * BH_ERR_INVALID_ARG before the device is touched.  The caller owns every buffer, the volume's included.
 *
 * THE VOLUME.  nx x ny x nz samples at  p(i,j,k) = origin + voxel_size * (float)(i,j,k)  (one multiply, one add per axis), x fastest in
 * memory: sample (i,j,k) has the linear index s = (k ny + j) nx + i.  tw[s] = { T, W }: the truncated signed distance in units of
 * `trunc` (negative behind the surface, 1 where nothing was seen) and the weight; rgb[s] the running mean colour.
 *
 * INTEGRATION (bh_tsdf_integrate).  All arithmetic is f32, every multiply, add and divide rounded on its own (no fma), so a float32
 * restatement reproduces it bit for bit.  Per sample, for the views in the order given:
 *   1. p as above.
 *   2. X = ((vm[0] px + vm[3] py) + vm[6] pz) + vm[9]          vm = BhCamera.vm, column-major 3x4
 *      Y = ((vm[1] px + vm[4] py) + vm[7] pz) + vm[10]
 *      Z = ((vm[2] px + vm[5] py) + vm[8] pz) + vm[11]         the z of BhRenderOut.depths_sorted and bh_render_depth
 *   3. skip unless Z > depth_min
 *   4. u = fx * (X / Z) + cx,  v = fy * (Y / Z) + cy;  skip unless 0 <= u < (float)W and 0 <= v < (float)H (a NaN skips);
 *      the pixel is (floor(u), floor(v)): pixel x has its centre at x + 0.5 (brush_hip_normal.h)
 *   5. d = depth[pixel];  skip unless d is finite, d > 0 (0 is "no depth", brush_hip_depth.h) and d <= depth_max (+inf allowed)
 *   6. with an image: skip if image[pixel].a < alpha_min
 *   7. sdf = d - Z;  skip if sdf < -trunc;  s = min(1, sdf / trunc)
 *   8. Wn = W + 1;  T = (W * T + s) / Wn;  with an image and rgb: c = (W * c + image.rgb) / Wn per channel;  W = min(Wn, max_weight)
 * A skipped view leaves the sample's bits alone.  One launch takes up to BH_TSDF_MAX_BATCH views: each sample is read once, updated
 * by the views in order in registers and written once (only if a view touched it), so the volume crosses memory once per 8 views;
 * the result is bit for bit that of single-view calls in the same order.  n_views > BH_TSDF_MAX_BATCH become consecutive launches.
 *
 * EXTRACTION (bh_tsdf_extract_count, bh_tsdf_extract): marching tetrahedra on the Freudenthal (Kuhn) split of each cube, iso value 0.
 *   inside = T < 0 (exactly 0 is outside);  observed = W > 0;  a cube is valid iff its 8 corners are observed; only valid cubes emit.
 *   The cube with min corner c = (i,j,k), i < nx-1, j < ny-1, k < nz-1, has 6 tetrahedra, one per permutation of the axes in
 *   lexicographic order:  0 xyz  1 xzy  2 yxz  3 yzx  4 zxy  5 zyx;  tetrahedron pi has the vertices
 *       v0 = c,  v1 = c + e_pi0,  v2 = v1 + e_pi1,  v3 = c + (1,1,1)
 *   (xyz, yzx, zxy are positively oriented, the other three negatively).  The edges of this triangulation from a sample p go to p + d,
 *   d in THIS order:  0 (1,0,0)  1 (0,1,0)  2 (0,0,1)  3 (1,1,0)  4 (1,0,1)  5 (0,1,1)  6 (1,1,1);  p owns these seven.
 *   VERTICES.  An owned edge carries a vertex iff its endpoints differ in `inside` and at least one valid cube contains both (the
 *   cubes with min corner p - a, a in {0,1}^3, a_axis = 0 wherever d_axis = 1).  Every vertex is referenced.  With a = the owner,
 *   b = the other end:  t = Ta / (Ta - Tb),  vertex = pa + t * (pb - pa) per axis,  colour = ca + t * (cb - ca)  (f32, no fma; pa, pb as
 *   in integration).  Order: by owner linear index, then by d.
 *   TRIANGLES.  Per tetrahedron, m = the 4-bit mask of inside vertices (bit n = v_n inside); its edges are numbered
 *       0 v0v1   1 v0v2   2 v0v3   3 v1v2   4 v1v3   5 v2v3
 *   and a positively oriented tetrahedron emits (each triple one triangle of edge numbers; a split quad's diagonal is the first
 *   triple's first and last entry):
 *       m  1: 0 1 2            m 14: 0 2 1
 *       m  2: 0 4 3            m 13: 0 3 4
 *       m  4: 5 1 3            m 11: 5 3 1
 *       m  8: 5 4 2            m  7: 5 2 4
 *       m  3: 1 2 4, 1 4 3     m 12: 1 3 4, 1 4 2
 *       m  5: 0 3 5, 0 5 2     m 10: 0 2 5, 0 5 3
 *       m  9: 0 1 5, 0 5 4     m  6: 0 4 5, 0 5 1
 *   m 0 and 15 emit nothing.  A negatively oriented tetrahedron emits the same triples with their last two entries exchanged.  The
 *   triangles are counter-clockwise seen from the positive (outside) side.  Order: by cube (min corner's linear index), then
 *   tetrahedron 0..5, then first / second triple.  A vertex is computed once, so the triangles around it agree and the mesh is closed
 *   wherever the field is observed.  No atomics: the same volume gives the same bytes.
 *   Scratch: 12 bytes per sample in a context slot (the edge mask and triangle count, and one running count each for vertices and
 *   triangles), grown on demand and kept until bh_destroy.  Vertex and triangle counts must stay below 2^32.
 */
#ifndef BRUSH_HIP_MESH_H
#define BRUSH_HIP_MESH_H

#include "brush_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_TSDF_MAX_BATCH 8u /* views per launch of bh_tsdf_integrate */

typedef struct BhTsdfGrid {
    float origin[3];     /* position of sample (0,0,0) */
    float voxel_size;    /* > 0 */
    uint32_t nx, ny, nz; /* samples per axis, each >= 2; nx * ny * nz <= 2^31 - 1 */
    float trunc;         /* truncation distance, > 0 (usually 4 voxels) */
    float max_weight;    /* >= 1: W saturates here */
    uint32_t reserved;   /* 0 */
    float* tw;           /* device [nz,ny,nx,2] f32: { T, W } */
    float* rgb;          /* device [nz,ny,nx,3] f32, or NULL: no colour */
} BhTsdfGrid;

typedef struct BhTsdfIntegrateConfig {
    float depth_min;   /* a sample is seen by a view only at Z > depth_min */
    float depth_max;   /* depths above this are ignored; +inf allowed */
    float alpha_min;   /* with an image: pixels of lower alpha are ignored */
    uint32_t reserved; /* 0 */
} BhTsdfIntegrateConfig;

#ifdef __cplusplus
static_assert(sizeof(BhTsdfGrid) == 56, "BhTsdfGrid layout");
static_assert(sizeof(BhTsdfIntegrateConfig) == 16, "BhTsdfIntegrateConfig layout");
#else
_Static_assert(sizeof(BhTsdfGrid) == 56, "BhTsdfGrid layout");
_Static_assert(sizeof(BhTsdfIntegrateConfig) == 16, "BhTsdfIntegrateConfig layout");
#endif

/* Every entry point that takes a grid refuses (BH_ERR_INVALID_ARG, before the device is touched): a null grid or tw, a dimension
 * below 2, more than 2^31 - 1 samples, voxel_size or trunc that is not a finite number > 0, max_weight below 1 or not a number. */

/* T = 1, W = 0, rgb = 0 in every sample.  Queued on the ctx stream. */
int bh_tsdf_clear(bh_ctx* ctx, const BhTsdfGrid* grid /*host*/);

/* Fuses n_views depth maps into the volume by the rule above, in the order given.  cams[v].img_w x img_h is the size of depths[v]
 * [H,W] f32 and images[v] [H,W,4] f32 (BhRenderOut.out_img); images == NULL: no alpha test and no colour (grid->rgb is left alone);
 * with images every entry must be non-null.  Pinhole cameras only; another model, a tile-row window on a camera, an image side of 0 or
 * more than 2^31 - 1 pixels is BH_ERR_INVALID_ARG and nothing is launched.  n_views == 0 does nothing.  Queued on the ctx stream: no
 * readback, no atomics; the host arrays may be freed on return. */
int bh_tsdf_integrate(bh_ctx* ctx, const BhTsdfGrid* grid /*host*/, uint32_t n_views, const BhCamera* cams /*host [n_views]*/,
                      const float* const* depths /*host [n_views] of device [H,W]*/, const float* const* images /*host [n_views] of device [H,W,4], or NULL*/,
                      const BhTsdfIntegrateConfig* cfg /*host*/);

/* The numbers of vertices and triangles of the volume's zero level set.  Blocking (one readback), like bh_splat_to_ply's size query. */
int bh_tsdf_extract_count(bh_ctx* ctx, const BhTsdfGrid* grid /*host*/, uint32_t* n_vertices /*host*/, uint32_t* n_triangles /*host*/);

/* The mesh itself: vertices [cap_v,3] f32, colours [cap_v,3] f32 (NULL: none; non-null needs grid->rgb), triangles [cap_t,3] u32
 * indices into vertices.  It classifies and scans again: no count call has to precede it.  The two counts are always returned; a
 * capacity below them is BH_ERR_INVALID_ARG and nothing is written.  A count of zero allows a null output.  Blocking. */
int bh_tsdf_extract(bh_ctx* ctx, const BhTsdfGrid* grid /*host*/, float* vertices /*[cap_v,3]*/, float* colours /*[cap_v,3] or NULL*/,
                    uint32_t* triangles /*[cap_t,3]*/, uint32_t cap_v, uint32_t cap_t, uint32_t* n_vertices /*host*/, uint32_t* n_triangles /*host*/);

/* A triangle mesh as a PLY file:
 *     ply / format binary_little_endian 1.0 / comment Exported from Brush / element vertex n_v / property float x, y, z
 *     [ / property uchar red, green, blue ] / element face n_t / property list uchar uint vertex_indices / end_header
 * A vertex row is 12 bytes (15 with colours: each channel clamped to [0,1] — not a number counts as 0 —, times 255, rounded half to
 * even); a face row is the byte 3 and three u32.  out == NULL is the size query (*written = the size; no device work).  Otherwise
 * the rows are packed on the device and arrive with one device-to-host copy; cap < the size is BH_ERR_INVALID_ARG.  Blocking. */
int bh_mesh_to_ply(bh_ctx* ctx, const float* vertices /*[n_v,3]*/, const float* colours /*[n_v,3] or NULL*/, uint32_t n_v,
                   const uint32_t* triangles /*[n_t,3]*/, uint32_t n_t, void* out /*host, or NULL*/, uint64_t cap, uint64_t* written /*host*/);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_MESH_H */
