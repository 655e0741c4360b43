/* brush_hip_sparse_mesh.h — sparse TSDF volumes: the fusion rule and the iso-surface contract of brush_hip_mesh.h on 8x8x8 blocks that
 * are allocated only around the observed surfaces (Open3D's ScalableTSDFVolume idea, with a bitmap and a rank array where Open3D has a
 * hash table), so that the voxel sizes real captures are fused at (4-10 mm over metres) fit.  DESIGN.md §6x has the whole contract.
 *
 * Same conventions as brush_hip_mesh.h: 0 on success, <0 on error (bh_last_error), device pointers unless marked host; a null ctx
 * returns BH_ERR_INVALID_ARG before the device is touched; the caller owns every buffer; every refusal happens before a launch.
 *
 * THE VOLUME.  A virtual grid of nx x ny x nz samples at  p(i,j,k) = origin + voxel_size * (float)(i,j,k), exactly the dense volume's
 * positions, cut into blocks of BH_SPTSDF_BLOCK^3 samples: NBX = ceil(nx / 8), NBY, NBZ likewise; block (bx,by,bz) has the key
 * (bz NBY + by) NBX + bx.  Samples of a boundary block with i >= nx (j >= ny, k >= nz) do not exist: they are never integrated and
 * stay at W = 0.  Limits: every dimension >= 2 and <= 8192; at most 2^30 virtual blocks; allocated blocks * 512 <= 2^31 - 1.
 *   bits  [n_words] u32   one bit per virtual block (bit key % 32 of word key / 32), n_words = ceil(NBX NBY NBZ / 32)
 *   rank  [n_words] u32   the number of set bits in earlier words
 *   keys  [n_blocks] u32  the keys of the allocated blocks, ascending
 *   tw    [n_blocks,8,8,8,2] f32  { T, W } per sample; local x fastest, then y, then z
 *   rgb   [n_blocks,8,8,8,3] f32, or NULL: the running mean colour
 * An allocated block's pool slot is  rank[key / 32] + popcount(bits[key / 32] & ((1 << key % 32) - 1)):  pool order is key order, there
 * is no hash table and nothing depends on scheduling.
 *
 * THE LIFE OF A VOLUME.  mark_clear; mark (any number of times); commit (-> n_blocks); the caller allocates keys, tw, rgb for n_blocks
 * and sets vol.n_blocks; clear; integrate (any number of times); extract / to_dense.  Marking after a commit needs mark_clear first
 * (and a new commit, clear and integration: a volume does not grow).
 *
 * MARKING (bh_sptsdf_mark): ray points through the truncation band — Open3D's rule, made exact.  All arithmetic f32, every operation
 * rounded on its own (no fma).  On the host:  step = 4.0f * voxel_size;  M = the smallest integer with (float)M * step >= 2.0f * trunc
 * (M > 64 is BH_ERR_INVALID_ARG).  Per view and per pixel (x, y):
 *   1. d = depth[pixel]; skip unless d is finite, d > 0 and d <= depth_max;  with images: skip if alpha < alpha_min
 *   2. rx = (((float)x + 0.5f) - cx) / fx,  ry = (((float)y + 0.5f) - cy) / fy
 *   3. for m = 0 .. M:  z = (d - trunc) + (float)m * step;  skip unless z > 0;  X = rx * z,  Y = ry * z;
 *        pw_a = ((vm[3a] * X + vm[3a+1] * Y) + vm[3a+2] * z) + cam_pos[a]          (BhCamera.vm's rotation transposed, plus cam_pos)
 *        g_a = (pw_a - origin_a) / voxel_size;  skip unless 0 <= g_a < (float)n_a on all three axes (a NaN skips)
 *        the block is (uint32_t)(g_a * 0.125f) per axis: set its bit.
 * Bits are set with an atomic OR on 32-bit words (a wave first ORs together what its lanes would set in the same word): the feature's
 * only atomic, idempotent, so the bitmap has the same bits from run to run.
 *
 * COMMIT (bh_sptsdf_commit).  A block is allocated iff a marked block lies within Chebyshev distance `dilate` (0, 1 or 2) of it inside
 * the grid; the dilated bitmap replaces `bits`, `rank` is filled, the count is read back (blocking).
 *
 * INTEGRATION (bh_sptsdf_integrate): steps 1-8 of brush_hip_mesh.h on every existing sample of every allocated block, p from the
 * sample's global index (i,j,k): a sample ends with the bits the dense volume would hold after the same views in the same order.
 *
 * EXTRACTION (bh_sptsdf_extract_count, bh_sptsdf_extract): the contract of brush_hip_mesh.h unchanged (inside = T < 0, a cube is valid
 * iff its 8 corners have W > 0, the seven owned edges, the vertex and colour formulas, the case table, the orientation); samples of
 * unallocated blocks count as W = 0.  Order: vertices by pool slot, then by local index (lz 8 + ly) 8 + lx, then by d; triangles by
 * owner cube in the same order, then tetrahedron, then triple.  No atomics.  Scratch: 12 bytes per allocated sample in a context slot.
 *
 * WHAT IS PROMISED.  The allocated set is what the marking and dilation rules say, and every allocated sample and the mesh equal the
 * dense path's on the dense volume bh_sptsdf_to_dense produces, bit for bit.  The mesh equals that of DENSE FUSION of the same views
 * when all marking precedes all integration and the allocation contains every block that holds a sample some view gave sdf < trunc,
 * and those blocks' 26 neighbours; ray marking does not guarantee that for every input (a pixel footprint wider than a block can miss
 * one).
 */
#ifndef BRUSH_HIP_SPARSE_MESH_H
#define BRUSH_HIP_SPARSE_MESH_H

#include "brush_hip_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BH_SPTSDF_BLOCK 8u        /* samples per block and axis */
#define BH_SPTSDF_MAX_DIM 8192u   /* samples per axis of the virtual grid */
#define BH_SPTSDF_MAX_STEPS 64u   /* the largest M of bh_sptsdf_mark */

typedef struct BhSparseTsdf {
    float origin[3];     /* position of sample (0,0,0) */
    float voxel_size;    /* > 0 */
    uint32_t nx, ny, nz; /* samples per axis of the virtual grid, each 2 .. 8192 */
    float trunc;         /* truncation distance, > 0 (usually 4 voxels) */
    float max_weight;    /* >= 1: W saturates here */
    uint32_t n_blocks;   /* allocated blocks (what bh_sptsdf_commit returned); 0 before a commit */
    uint32_t* bits;      /* device [n_words] */
    uint32_t* rank;      /* device [n_words] */
    uint32_t* keys;      /* device [n_blocks] */
    float* tw;           /* device [n_blocks,8,8,8,2] f32: { T, W } */
    float* rgb;          /* device [n_blocks,8,8,8,3] f32, or NULL: no colour */
} BhSparseTsdf;

#ifdef __cplusplus
static_assert(sizeof(BhSparseTsdf) == 80, "BhSparseTsdf layout");
#else
_Static_assert(sizeof(BhSparseTsdf) == 80, "BhSparseTsdf layout");
#endif

/* Every entry point refuses (BH_ERR_INVALID_ARG, before the device is touched): a null vol, bits or rank, a dimension below 2 or
 * above 8192, more than 2^30 virtual blocks, voxel_size or trunc that is not a finite number > 0, max_weight below 1 or not a number.
 * clear, integrate, extract_count, extract and to_dense also refuse a volume before its commit (n_blocks == 0, null keys or tw) and
 * n_blocks * 512 > 2^31 - 1. */

/* Zeroes bits.  Queued on the ctx stream. */
int bh_sptsdf_mark_clear(bh_ctx* ctx, const BhSparseTsdf* vol /*host*/);

/* Marks the blocks near the surfaces the depth maps show, by the rule above.  Cameras, depths, images, cfg and their refusals are those
 * of bh_tsdf_integrate (cfg->depth_min is not used); M > 64 is refused too.  Only bits is touched.  Queued on the ctx stream. */
int bh_sptsdf_mark(bh_ctx* ctx, const BhSparseTsdf* vol /*host*/, uint32_t n_views, const BhCamera* cams /*host [n_views]*/,
                   const float* const* depths /*host [n_views] of device [H,W]*/, const float* const* images /*host [n_views] of device [H,W,4], or NULL*/,
                   const BhTsdfIntegrateConfig* cfg /*host*/);

/* Dilates bits by `dilate` blocks (0, 1 or 2; anything else is BH_ERR_INVALID_ARG), fills rank and returns the number of allocated
 * blocks; more than (2^31 - 1) / 512 of them is BH_ERR_INVALID_ARG (the count is still returned).  Scratch: 12 bytes per word of bits
 * in a context slot.  Blocking (one readback), like bh_tsdf_extract_count. */
int bh_sptsdf_commit(bh_ctx* ctx, const BhSparseTsdf* vol /*host*/, uint32_t dilate, uint32_t* n_blocks /*host*/);

/* After the caller has allocated keys, tw and rgb for vol->n_blocks = the committed count: writes keys from bits and rank, and T = 1,
 * W = 0, rgb = 0 in every sample of the pool.  Queued on the ctx stream. */
int bh_sptsdf_clear(bh_ctx* ctx, const BhSparseTsdf* vol /*host*/);

/* bh_tsdf_integrate on the allocated blocks: same arguments, same refusals, up to BH_TSDF_MAX_BATCH views per launch.  Queued. */
int bh_sptsdf_integrate(bh_ctx* ctx, const BhSparseTsdf* vol /*host*/, uint32_t n_views, const BhCamera* cams /*host [n_views]*/,
                        const float* const* depths /*host [n_views] of device [H,W]*/, const float* const* images /*host [n_views] of device [H,W,4], or NULL*/,
                        const BhTsdfIntegrateConfig* cfg /*host*/);

/* As bh_tsdf_extract_count and bh_tsdf_extract: the counts are always returned, a capacity below them is BH_ERR_INVALID_ARG and nothing
 * is written, colours need vol->rgb.  Blocking. */
int bh_sptsdf_extract_count(bh_ctx* ctx, const BhSparseTsdf* vol /*host*/, uint32_t* n_vertices /*host*/, uint32_t* n_triangles /*host*/);
int bh_sptsdf_extract(bh_ctx* ctx, const BhSparseTsdf* vol /*host*/, float* vertices /*[cap_v,3]*/, float* colours /*[cap_v,3] or NULL*/,
                      uint32_t* triangles /*[cap_t,3]*/, uint32_t cap_v, uint32_t cap_t, uint32_t* n_vertices /*host*/, uint32_t* n_triangles /*host*/);

/* Writes the window of the virtual grid that starts at sample (i0,j0,k0) and has the size of `dense` into that dense volume: allocated
 * samples bit for bit (rgb too where both volumes have it), everything else — unallocated blocks, samples that do not exist, the
 * part of a window that leaves the virtual grid — as T = 1, W = 0, rgb = 0.  Only dense->nx, ny, nz, tw and rgb are read (dimensions
 * >= 2, at most 2^31 - 1 samples).  Queued on the ctx stream. */
int bh_sptsdf_to_dense(bh_ctx* ctx, const BhSparseTsdf* vol /*host*/, uint32_t i0, uint32_t j0, uint32_t k0, const BhTsdfGrid* dense /*host*/);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_SPARSE_MESH_H */
