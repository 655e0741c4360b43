// sparse_tsdf.hip — sparse TSDF volumes (include/brush_hip_sparse_mesh.h): the dense volume's fusion rule and
// iso-surface contract (device_tsdf.h: one copy of both) on 8x8x8 blocks allocated only around the observed surfaces.  Not in the
// reference.
//
// The index is a bitmap over the virtual blocks and a rank array (set bits in earlier words): a block's pool slot is rank + popcount,
// pool order is key order, and nothing depends on scheduling.  Marking sets bits with an atomic OR (idempotent; a wave first ORs
// together what its lanes would set in one word, and skips the atomic when the word already holds them) — the only atomic here.
// Commit dilates the bitmap one axis at a time (a box is separable), a word per thread; a word whose sources are all zero — nearly
// every word — is written without looking at a bit.
//
// Integration: a workgroup takes a pool block, a wave owns z-slices of it (64 consecutive pool entries, 512 contiguous bytes of tw);
// the cameras come from the kernel arguments, the sample's load / fuse / store is tsdf_fuse_at, the dense kernel's.  No rejection of
// whole blocks against a view: none was shown to leave every bit alone.
//
// Extraction is the dense path's three phases (classify, two inclusive scans over n_blocks * 512 entries, emit) without atomics.
// Classify stages the {observed, inside} bits of a block's 10x10x10 neighbourhood in LDS (1000 bytes) — the up to 26 neighbour blocks
// are looked up once per workgroup through bits and rank — where the dense kernel pays 27 scattered loads per sample.
//
// The clear kernel and the host side of clear, integrate, extract_count and extract are the dense volume's (device_tsdf.h:
// tsdf_clear_samples, tsdf_check_fields, tsdf_integrate_batches, tsdf_extract_run); this unit supplies its struct, its check and its
// launches.  Marking, commit, keys and to_dense have no dense twin.
#include <cmath>
#include <string>

#include "../../include/brush_hip_sparse_mesh.h"
#include "context.h"
#include "device_math.h"
#include "device_tsdf.h"

namespace bh {

constexpr uint32_t SP_NONE = 0xFFFFFFFFu;
constexpr uint32_t SP_MAX_POOL_BLOCKS = 0x7FFFFFFFu / 512u;
constexpr uint32_t SP_MAX_WGS = 1u << 20;

struct SpVolDev {
    float ox, oy, oz, vs;
    uint32_t nx, ny, nz;
    uint32_t nbx, nby, nbz;
    uint32_t total, n_words;   // virtual blocks, words of bits
    float trunc, max_weight;
    uint32_t n_blocks;
    uint32_t* bits;
    uint32_t* rank;
    uint32_t* keys;
    float2* tw;
    float* rgb;
};

// the pool slot of block `key`, or SP_NONE (unallocated, or beyond the pool the caller declared)
BH_DEV uint32_t sp_slot_of(const SpVolDev& g, const uint32_t key) {
    const uint32_t word = g.bits[key >> 5], b = key & 31u;
    if (!((word >> b) & 1u)) return SP_NONE;
    const uint32_t slot = g.rank[key >> 5] + (uint32_t)__popc(word & ((1u << b) - 1u));
    return slot < g.n_blocks ? slot : SP_NONE;
}

// the slot of the block at (bx + ox, by + oy, bz + oz), or SP_NONE
BH_DEV uint32_t sp_neighbour_slot(const SpVolDev& g, const uint32_t bx, const uint32_t by, const uint32_t bz, const int ox, const int oy, const int oz) {
    const int x = (int)bx + ox, y = (int)by + oy, z = (int)bz + oz;
    if (x < 0 || y < 0 || z < 0 || x >= (int)g.nbx || y >= (int)g.nby || z >= (int)g.nbz) return SP_NONE;
    return sp_slot_of(g, ((uint32_t)z * g.nby + (uint32_t)y) * g.nbx + (uint32_t)x);
}

// the block coordinates of `key`
BH_DEV void sp_block_coords(const SpVolDev& g, const uint32_t key, uint32_t& bx, uint32_t& by, uint32_t& bz) {
    const uint32_t rest = key / g.nbx;
    bx = key % g.nbx; by = rest % g.nby; bz = rest / g.nby;
}

// where the sample (x, y, z) of the virtual grid, or of a block, lies in its block's 512 pool entries
BH_DEV uint32_t sp_local_index(const uint32_t x, const uint32_t y, const uint32_t z) { return ((z & 7u) * 8u + (y & 7u)) * 8u + (x & 7u); }

// ---- marking ----------------------------------------------------------------------------------------------------------------------
struct SpMarkView {
    float r[9];     // BhCamera.vm's rotation (column-major)
    float pos[3];   // BhCamera.cam_pos
    float fx, fy, cx, cy;
    uint32_t w, h;
    const float* depth;
    const float* image;   // [H,W,4] or NULL
};

struct SpMarkBatch {
    SpMarkView v[BH_TSDF_MAX_BATCH];
};
static_assert(sizeof(SpMarkBatch) == 88 * BH_TSDF_MAX_BATCH, "SpMarkBatch is passed by value");

// Sets the bit of `key` (SP_NONE: none) for every lane of the wave; all 64 lanes call it together.
BH_DEV void sp_wave_mark(uint32_t* bits, const uint32_t key) {
    const uint32_t word = key >> 5, bit = key == SP_NONE ? 0u : 1u << (key & 31u);
    bool pending = key != SP_NONE;
    for (;;) {
        const unsigned long long live = __ballot(pending);
        if (live == 0ull) break;
        const int leader = __ffsll((long long)live) - 1;
        const uint32_t w0 = (uint32_t)__shfl((int)word, leader);
        const bool mine = pending && word == w0;
        uint32_t v = mine ? bit : 0u;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v |= (uint32_t)__shfl_xor((int)v, off);
        // (a stale read only costs the atomic it could have saved: bits go from 0 to 1 and never back while marking)
        if ((int)__lane_id() == leader && (bits[w0] & v) != v) atomicOr(&bits[w0], v);
        if (mine) pending = false;
    }
}

__global__ __launch_bounds__(256) void sptsdf_mark_kernel(const SpVolDev g, const SpMarkBatch b, const float depth_max, const float alpha_min, const uint32_t M,
                                                          const float step) {
    const SpMarkView& cam = b.v[blockIdx.y];
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    bool live = p < cam.w * cam.h;
    float d = 0.0f;
    if (live) {
        d = cam.depth[p];
        live = is_finite_f32(d) && d > 0.0f && d <= depth_max;
        if (live && cam.image) live = !(cam.image[(size_t)p * 4 + 3] < alpha_min);
    }
    const uint32_t x = p % cam.w, y = p / cam.w;
    const float rx = (((float)x + 0.5f) - cam.cx) / cam.fx, ry = (((float)y + 0.5f) - cam.cy) / cam.fy;
    const float z0 = d - g.trunc;
    const float org[3] = {g.ox, g.oy, g.oz};
    const float dims[3] = {(float)g.nx, (float)g.ny, (float)g.nz};
    for (uint32_t m = 0; m <= M; ++m) {   // (wave-uniform: every lane stays for sp_wave_mark)
        uint32_t key = SP_NONE;
        const float z = z0 + (float)m * step;
        if (live && z > 0.0f) {
            const float X = rx * z, Y = ry * z;
            uint32_t blk[3];
            bool in = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float pw = ((cam.r[3 * a] * X + cam.r[3 * a + 1] * Y) + cam.r[3 * a + 2] * z) + cam.pos[a];
                const float ga = (pw - org[a]) / g.vs;
                in = in && ga >= 0.0f && ga < dims[a];   // (a NaN fails both)
                blk[a] = in ? (uint32_t)(ga * 0.125f) : 0u;
            }
            if (in) key = (blk[2] * g.nby + blk[1]) * g.nbx + blk[0];
        }
        sp_wave_mark(g.bits, key);
    }
}

// ---- commit -----------------------------------------------------------------------------------------------------------------------
// One axis of the box dilation by r: out(key) = OR of in(key + d * stride), |d| <= r, where the block's coordinate along the axis,
// (key / stride) % n_axis, stays inside 0 .. n_axis - 1.  A thread writes one word.
__global__ __launch_bounds__(256) void sptsdf_dilate_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const uint32_t n_words, const uint32_t total,
                                                            const uint32_t stride, const uint32_t n_axis, const int r) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= n_words) return;
    uint32_t any = 0;
    for (int d = -r; d <= r; ++d) {   // the words that hold a source of one of this word's 32 keys
        long long lo = (long long)w * 32 + (long long)d * (long long)stride, hi = lo + 31;
        if (hi < 0 || lo >= (long long)total) continue;
        if (lo < 0) lo = 0;
        if (hi >= (long long)total) hi = (long long)total - 1;
        for (long long ww = lo >> 5; ww <= hi >> 5; ++ww) any |= in[ww];
    }
    uint32_t res = 0;
    if (any) {
        for (uint32_t b = 0; b < 32u; ++b) {
            const uint32_t key = w * 32u + b;
            if (key >= total) break;
            const int c = (int)((key / stride) % n_axis);
            for (int d = -r; d <= r; ++d) {
                if (c + d < 0 || c + d >= (int)n_axis) continue;
                const uint32_t src = (uint32_t)((long long)key + (long long)d * (long long)stride);
                if ((in[src >> 5] >> (src & 31u)) & 1u) {
                    res |= 1u << b;
                    break;
                }
            }
        }
    }
    out[w] = res;
}

__global__ __launch_bounds__(256) void sptsdf_popcount_kernel(const uint32_t* __restrict__ bits, uint32_t* __restrict__ cnt, const uint32_t n_words) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w < n_words) cnt[w] = (uint32_t)__popc(bits[w]);
}

// ---- clear ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sptsdf_keys_kernel(const SpVolDev g) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= g.n_words) return;
    uint32_t word = g.bits[w], slot = g.rank[w];
    while (word) {
        const uint32_t b = (uint32_t)__ffs((int)word) - 1u;
        word &= word - 1u;
        if (slot < g.n_blocks) g.keys[slot] = w * 32u + b;
        ++slot;
    }
}

// ---- integration ------------------------------------------------------------------------------------------------------------------
// COLOUR: the volume has rgb and the batch has images (then every view has one)
template <bool COLOUR>
__global__ __launch_bounds__(256) void sptsdf_integrate_kernel(const SpVolDev g, const TsdfBatch b, const uint32_t n_views, const float depth_min, const float depth_max,
                                                               const float alpha_min) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t blk = blockIdx.x; blk < g.n_blocks; blk += gridDim.x) {
        const uint32_t key = g.keys[blk];
        uint32_t bx, by, bz;
        sp_block_coords(g, key, bx, by, bz);
        const uint32_t i = bx * 8u + (lane & 7u), j = by * 8u + (lane >> 3);
        if (i >= g.nx || j >= g.ny) continue;
        const float px = g.ox + g.vs * (float)i, py = g.oy + g.vs * (float)j;
        for (uint32_t lz = wave; lz < 8u; lz += 4u) {   // a wave owns the slices lz = wave, wave + 4
            const uint32_t k = bz * 8u + lz;
            if (k >= g.nz) break;
            const float pz = g.oz + g.vs * (float)k;
            const size_t s = (size_t)blk * 512u + lz * 64u + lane;
            tsdf_fuse_at<COLOUR>(g.tw, g.rgb, s, px, py, pz, b, n_views, depth_min, depth_max, alpha_min, g.trunc, g.max_weight);
        }
    }
}

// ---- extraction -------------------------------------------------------------------------------------------------------------------
// One workgroup per pool block.  info as in tsdf.hip, at the sample's pool index.
__global__ __launch_bounds__(256) void sptsdf_classify_kernel(const SpVolDev g, uint32_t* __restrict__ info, uint32_t* __restrict__ vcnt, uint32_t* __restrict__ tcnt) {
    __shared__ uint32_t s_slot[27];
    __shared__ uint8_t s_nb[1000];   // the block's 10x10x10 neighbourhood: observed | inside << 1
    for (uint32_t blk = blockIdx.x; blk < g.n_blocks; blk += gridDim.x) {
        const uint32_t key = g.keys[blk];
        uint32_t bx, by, bz;
        sp_block_coords(g, key, bx, by, bz);
        if (threadIdx.x < 27u) {
            const int t = (int)threadIdx.x;
            s_slot[t] = sp_neighbour_slot(g, bx, by, bz, t % 3 - 1, (t / 3) % 3 - 1, t / 9 - 1);
        }
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < 1000u; e += 256u) {
            const int lx = (int)(e % 10u) - 1, ly = (int)((e / 10u) % 10u) - 1, lz = (int)(e / 100u) - 1;   // -1 .. 8
            const uint32_t slot = s_slot[(((lz + 8) >> 3) * 3 + ((ly + 8) >> 3)) * 3 + ((lx + 8) >> 3)];
            uint8_t byte = 0;
            // (a neighbour block that exists has coordinates >= 0; the sample itself must exist too)
            if (slot != SP_NONE && (int)(bx * 8u) + lx < (int)g.nx && (int)(by * 8u) + ly < (int)g.ny && (int)(bz * 8u) + lz < (int)g.nz) {
                const float2 t = g.tw[(size_t)slot * 512u + sp_local_index((uint32_t)lx, (uint32_t)ly, (uint32_t)lz)];
                byte = (uint8_t)((t.y > 0.0f ? 1u : 0u) | (t.x < 0.0f ? 2u : 0u));
            }
            s_nb[e] = byte;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t q = 0; q < 2u; ++q) {
            const uint32_t local = threadIdx.x + q * 256u;
            const int lx = (int)(local & 7u), ly = (int)((local >> 3) & 7u), lz = (int)(local >> 6);
            uint32_t obs = 0, ins = 0;
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const uint32_t v = s_nb[((lz + 1 + dz) * 10 + (ly + 1 + dy)) * 10 + (lx + 1 + dx)];
                        obs |= (v & 1u) << nb_bit(dx, dy, dz);
                        ins |= (v >> 1) << nb_bit(dx, dy, dz);
                    }
            tsdf_store_class(info, vcnt, tcnt, (size_t)blk * 512u + local, tsdf_classify_word(obs, ins));
        }
        __syncthreads();   // (the next block's staging overwrites s_slot and s_nb)
    }
}

__global__ __launch_bounds__(256) void sptsdf_emit_kernel(const SpVolDev g, const uint32_t* __restrict__ info, const uint32_t* __restrict__ vinc,
                                                          const uint32_t* __restrict__ tinc, float* __restrict__ vertices, float* __restrict__ colours,
                                                          uint32_t* __restrict__ triangles) {
    __shared__ uint32_t s_slot[8];   // the blocks at (+0|1, +0|1, +0|1)
    for (uint32_t blk = blockIdx.x; blk < g.n_blocks; blk += gridDim.x) {
        const uint32_t key = g.keys[blk];
        uint32_t bx, by, bz;
        sp_block_coords(g, key, bx, by, bz);
        if (threadIdx.x < 8u) {
            const int t = (int)threadIdx.x;
            s_slot[t] = t == 0 ? blk : sp_neighbour_slot(g, bx, by, bz, t & 1, (t >> 1) & 1, t >> 2);
        }
        __syncthreads();
        for (uint32_t q = 0; q < 2u; ++q) {
            const uint32_t local = threadIdx.x + q * 256u;
            const size_t s = (size_t)blk * 512u + local;
            const uint32_t word = info[s];
            if ((word & 0xFF7Fu) == 0u) continue;
            const uint32_t lx = local & 7u, ly = (local >> 3) & 7u, lz = local >> 6;
            tsdf_emit_sample(g.ox, g.oy, g.oz, g.vs, bx * 8u + lx, by * 8u + ly, bz * 8u + lz, s, word, g.tw, g.rgb, info, vinc, tinc, vertices, colours, triangles,
                             [&](uint32_t c) {
                                 const uint32_t x = lx + (c & 1u), y = ly + ((c >> 1) & 1u), z = lz + (c >> 2);
                                 const uint32_t slot = s_slot[(x >> 3) | (y >> 3) << 1 | (z >> 3) << 2];
                                 // (an edge or a cube that emits has observed ends, so their blocks are allocated; never index with SP_NONE)
                                 return slot == SP_NONE ? s : (size_t)slot * 512u + sp_local_index(x, y, z);
                             });
        }
        __syncthreads();
    }
}

// ---- to dense ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sptsdf_to_dense_kernel(const SpVolDev g, const uint32_t i0, const uint32_t j0, const uint32_t k0, const uint32_t dnx,
                                                              const uint32_t dny, const uint32_t n, float2* __restrict__ dtw, float* __restrict__ drgb) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    const uint64_t i = (uint64_t)i0 + s % dnx, j = (uint64_t)j0 + (s / dnx) % dny, k = (uint64_t)k0 + s / (dnx * dny);
    float2 tw = make_float2(1.0f, 0.0f);
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    if (i < g.nx && j < g.ny && k < g.nz) {
        const uint32_t slot = sp_slot_of(g, (((uint32_t)k >> 3) * g.nby + ((uint32_t)j >> 3)) * g.nbx + ((uint32_t)i >> 3));
        if (slot != SP_NONE) {
            const size_t src = (size_t)slot * 512u + sp_local_index((uint32_t)i, (uint32_t)j, (uint32_t)k);
            tw = g.tw[src];
            if (g.rgb && drgb) {
                c0 = g.rgb[src * 3]; c1 = g.rgb[src * 3 + 1]; c2 = g.rgb[src * 3 + 2];
            }
        }
    }
    dtw[s] = tw;
    if (drgb) {
        drgb[(size_t)s * 3] = c0; drgb[(size_t)s * 3 + 1] = c1; drgb[(size_t)s * 3 + 2] = c2;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static int sp_check_vol(bh_ctx* ctx, const BhSparseTsdf* v, const char* who, bool committed, SpVolDev* dev) {
    const std::string w(who);
    if (!v || !v->bits || !v->rank) return set_error(ctx, BH_ERR_INVALID_ARG, w + ": null volume, bits or rank");
    const uint32_t nbx = (v->nx + 7u) / 8u, nby = (v->ny + 7u) / 8u, nbz = (v->nz + 7u) / 8u;
    const uint64_t total = (uint64_t)nbx * nby * nbz;
    if (v->nx >= 2u && v->ny >= 2u && v->nz >= 2u) {   // (a side below 2 is tsdf_check_fields' first refusal, ahead of the size limits)
        if (v->nx > BH_SPTSDF_MAX_DIM || v->ny > BH_SPTSDF_MAX_DIM || v->nz > BH_SPTSDF_MAX_DIM)
            return set_error(ctx, BH_ERR_INVALID_ARG, w + ": a dimension of the grid above 8192");
        if (total > (1ull << 30)) return set_error(ctx, BH_ERR_INVALID_ARG, w + ": more than 2^30 virtual blocks");
    }
    BH_TRY(tsdf_check_fields(ctx, w, v->nx, v->ny, v->nz, v->voxel_size, v->trunc, v->max_weight));
    if (committed) {
        if (v->n_blocks == 0u || !v->keys || !v->tw) return set_error(ctx, BH_ERR_INVALID_ARG, w + ": a volume before its commit (no blocks, or null keys or tw)");
        if (v->n_blocks > SP_MAX_POOL_BLOCKS) return set_error(ctx, BH_ERR_INVALID_ARG, w + ": more than 2^31 - 1 allocated samples");
        if (v->n_blocks > total) return set_error(ctx, BH_ERR_INVALID_ARG, w + ": more allocated blocks than the grid has");
    }
    *dev = SpVolDev{v->origin[0], v->origin[1], v->origin[2], v->voxel_size, v->nx, v->ny, v->nz, nbx, nby, nbz, (uint32_t)total, (uint32_t)((total + 31u) / 32u),
                    v->trunc, v->max_weight, committed ? v->n_blocks : 0u, v->bits, v->rank, v->keys, reinterpret_cast<float2*>(v->tw), v->rgb};
    return 0;
}

static uint32_t sp_wgs(uint32_t n_blocks) { return n_blocks < SP_MAX_WGS ? n_blocks : SP_MAX_WGS; }

// bh_sptsdf_extract and bh_sptsdf_extract_count: the sparse volume's two launches for tsdf_extract_run
static int sp_extract_vol(bh_ctx* ctx, const BhSparseTsdf* vol, const char* who, float* vertices, float* colours, uint32_t* triangles, uint32_t cap_v, uint32_t cap_t,
                          uint32_t* n_vertices, uint32_t* n_triangles, bool count_only) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    SpVolDev g;
    BH_TRY(sp_check_vol(ctx, vol, who, true, &g));
    const dim3 launch(sp_wgs(g.n_blocks)), block(256);
    static const char* const prof[3] = {"SpTsdfClassify", "SpTsdfScan", "SpTsdfEmit"};
    return tsdf_extract_run(
        ctx, who, SLOT_SPTSDF, g.n_blocks * 512u, g.rgb != nullptr,
        [&](uint32_t* info, uint32_t* vcnt, uint32_t* tcnt) {
            hipLaunchKernelGGL(sptsdf_classify_kernel, launch, block, 0, ctx->stream, g, info, vcnt, tcnt);
            BH_LAUNCH_CHECK(ctx, "sptsdf_classify_kernel");
            return 0;
        },
        [&](const uint32_t* info, const uint32_t* vinc, const uint32_t* tinc) {
            hipLaunchKernelGGL(sptsdf_emit_kernel, launch, block, 0, ctx->stream, g, info, vinc, tinc, vertices, colours, triangles);
            BH_LAUNCH_CHECK(ctx, "sptsdf_emit_kernel");
            return 0;
        },
        vertices, colours, triangles, cap_v, cap_t, n_vertices, n_triangles, count_only, prof);
}

}  // namespace bh

using namespace bh;

extern "C" {

int bh_sptsdf_mark_clear(bh_ctx* ctx, const BhSparseTsdf* vol) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    SpVolDev g;
    BH_TRY(sp_check_vol(ctx, vol, "sptsdf_mark_clear", false, &g));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    BH_HIP(ctx, hipMemsetAsync(g.bits, 0, (size_t)g.n_words * 4, ctx->stream));
    return 0;
}

int bh_sptsdf_mark(bh_ctx* ctx, const BhSparseTsdf* vol, uint32_t n_views, const BhCamera* cams, const float* const* depths, const float* const* images,
                   const BhTsdfIntegrateConfig* cfg) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    SpVolDev g;
    BH_TRY(sp_check_vol(ctx, vol, "sptsdf_mark", false, &g));
    if (!cfg) return set_error(ctx, BH_ERR_INVALID_ARG, "sptsdf_mark: null config");
    const float step = 4.0f * g.vs, band = 2.0f * g.trunc;
    uint32_t M = 0;
    while (M <= BH_SPTSDF_MAX_STEPS && !((float)M * step >= band)) ++M;
    if (M > BH_SPTSDF_MAX_STEPS) return set_error(ctx, BH_ERR_INVALID_ARG, "sptsdf_mark: more than 64 steps of 4 voxels through the band of 2 trunc");
    if (n_views == 0) return 0;
    BH_TRY(tsdf_check_views(ctx, "sptsdf_mark", n_views, cams, depths, images));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    ProfScope ps(ctx, "SpTsdfMark");
    for (uint32_t first = 0; first < n_views; first += BH_TSDF_MAX_BATCH) {
        const uint32_t count = n_views - first < BH_TSDF_MAX_BATCH ? n_views - first : BH_TSDF_MAX_BATCH;
        SpMarkBatch b{};
        uint32_t pixels = 0;
        for (uint32_t v = 0; v < count; ++v) {
            const BhCamera& c = cams[first + v];
            SpMarkView& t = b.v[v];
            for (int e = 0; e < 9; ++e) t.r[e] = c.vm[e];
            for (int a = 0; a < 3; ++a) t.pos[a] = c.cam_pos[a];
            t.fx = c.fx; t.fy = c.fy; t.cx = c.cx; t.cy = c.cy;
            t.w = c.img_w; t.h = c.img_h;
            t.depth = depths[first + v];
            t.image = images ? images[first + v] : nullptr;
            if (c.img_w * c.img_h > pixels) pixels = c.img_w * c.img_h;
        }
        hipLaunchKernelGGL(sptsdf_mark_kernel, dim3((pixels + 255u) / 256u, count), dim3(256), 0, ctx->stream, g, b, cfg->depth_max, cfg->alpha_min, M, step);
        BH_LAUNCH_CHECK(ctx, "sptsdf_mark_kernel");
    }
    return 0;
}

int bh_sptsdf_commit(bh_ctx* ctx, const BhSparseTsdf* vol, uint32_t dilate, uint32_t* n_blocks) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    SpVolDev g;
    BH_TRY(sp_check_vol(ctx, vol, "sptsdf_commit", false, &g));
    if (dilate > 2u) return set_error(ctx, BH_ERR_INVALID_ARG, "sptsdf_commit: dilate must be 0, 1 or 2");
    if (!n_blocks) return set_error(ctx, BH_ERR_INVALID_ARG, "sptsdf_commit: null count pointer");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nw = g.n_words;
    auto* scratch = (uint32_t*)ensure(ctx, SLOT_SPTSDF, nw * 12);
    if (!scratch) return BH_ERR_OOM;
    uint32_t *a = scratch, *b = scratch + nw, *cnt = scratch + 2 * nw;
    const dim3 grid((g.n_words + 255u) / 256u), block(256);
    ProfScope ps(ctx, "SpTsdfCommit");
    if (dilate) {
        hipLaunchKernelGGL(sptsdf_dilate_kernel, grid, block, 0, ctx->stream, g.bits, a, g.n_words, g.total, 1u, g.nbx, (int)dilate);
        hipLaunchKernelGGL(sptsdf_dilate_kernel, grid, block, 0, ctx->stream, a, b, g.n_words, g.total, g.nbx, g.nby, (int)dilate);
        hipLaunchKernelGGL(sptsdf_dilate_kernel, grid, block, 0, ctx->stream, b, g.bits, g.n_words, g.total, g.nbx * g.nby, g.nbz, (int)dilate);
        BH_LAUNCH_CHECK(ctx, "sptsdf_dilate_kernel");
    }
    hipLaunchKernelGGL(sptsdf_popcount_kernel, grid, block, 0, ctx->stream, g.bits, cnt, g.n_words);
    BH_LAUNCH_CHECK(ctx, "sptsdf_popcount_kernel");
    BH_TRY(prefix_sum(ctx, cnt, nullptr, g.n_words, g.rank, /*exclusive=*/true));
    uint32_t last[2] = {0, 0};
    BH_HIP(ctx, hipMemcpyAsync(&last[0], g.rank + (nw - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    BH_HIP(ctx, hipMemcpyAsync(&last[1], cnt + (nw - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    BH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_blocks = last[0] + last[1];
    if (*n_blocks > SP_MAX_POOL_BLOCKS) return set_error(ctx, BH_ERR_INVALID_ARG, "sptsdf_commit: more than 2^31 - 1 allocated samples");
    return 0;
}

int bh_sptsdf_clear(bh_ctx* ctx, const BhSparseTsdf* vol) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    SpVolDev g;
    BH_TRY(sp_check_vol(ctx, vol, "sptsdf_clear", true, &g));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(sptsdf_keys_kernel, dim3((g.n_words + 255u) / 256u), dim3(256), 0, ctx->stream, g);
    BH_LAUNCH_CHECK(ctx, "sptsdf_keys_kernel");
    return tsdf_clear_samples(ctx, g.tw, g.rgb, g.n_blocks * 512u);
}

int bh_sptsdf_integrate(bh_ctx* ctx, const BhSparseTsdf* vol, uint32_t n_views, const BhCamera* cams, const float* const* depths, const float* const* images,
                        const BhTsdfIntegrateConfig* cfg) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    SpVolDev g;
    BH_TRY(sp_check_vol(ctx, vol, "sptsdf_integrate", true, &g));
    const dim3 launch(sp_wgs(g.n_blocks)), block(256);
    return tsdf_integrate_batches(ctx, "sptsdf_integrate", "SpTsdfIntegrate", n_views, cams, depths, images, cfg, g.rgb != nullptr,
                                  [&](bool colour, const TsdfBatch& b, uint32_t count) {
                                      hipLaunchKernelGGL(colour ? sptsdf_integrate_kernel<true> : sptsdf_integrate_kernel<false>, launch, block, 0, ctx->stream, g, b,
                                                         count, cfg->depth_min, cfg->depth_max, cfg->alpha_min);
                                  });
}

int bh_sptsdf_extract_count(bh_ctx* ctx, const BhSparseTsdf* vol, uint32_t* n_vertices, uint32_t* n_triangles) {
    return sp_extract_vol(ctx, vol, "sptsdf_extract_count", nullptr, nullptr, nullptr, 0, 0, n_vertices, n_triangles, /*count_only=*/true);
}

int bh_sptsdf_extract(bh_ctx* ctx, const BhSparseTsdf* vol, float* vertices, float* colours, uint32_t* triangles, uint32_t cap_v, uint32_t cap_t,
                      uint32_t* n_vertices, uint32_t* n_triangles) {
    return sp_extract_vol(ctx, vol, "sptsdf_extract", vertices, colours, triangles, cap_v, cap_t, n_vertices, n_triangles, /*count_only=*/false);
}

int bh_sptsdf_to_dense(bh_ctx* ctx, const BhSparseTsdf* vol, uint32_t i0, uint32_t j0, uint32_t k0, const BhTsdfGrid* dense) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    SpVolDev g;
    BH_TRY(sp_check_vol(ctx, vol, "sptsdf_to_dense", true, &g));
    if (!dense || !dense->tw) return set_error(ctx, BH_ERR_INVALID_ARG, "sptsdf_to_dense: null dense grid");
    BH_TRY(tsdf_check_dense_dims(ctx, "sptsdf_to_dense", "dense ", dense->nx, dense->ny, dense->nz));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t n = dense->nx * dense->ny * dense->nz;
    hipLaunchKernelGGL(sptsdf_to_dense_kernel, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, g, i0, j0, k0, dense->nx, dense->ny, n,
                       reinterpret_cast<float2*>(dense->tw), dense->rgb);
    BH_LAUNCH_CHECK(ctx, "sptsdf_to_dense_kernel");
    return 0;
}

}  // extern "C"
