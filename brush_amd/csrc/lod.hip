// lod.hip — LOD decimation: PUP sensitivity scores and decimate_to_count.
//
// Reference: brush-train/src/lod.rs (paths under the reference's crates/), called at every LOD boundary from
// brush-process/src/train_stream.rs:248-303:
//   compute_pup_scores (lod.rs:78-142)  per training view a forward + backward with an L1-only loss; the per-splat 6-vector
//                                       J = [dL/dmean (3), dL/dlog_scale (3)] enters H += J Jᵀ, summed over the views
//   log_det_6x6        (lod.rs:44-70)   score = log det H by an f32 Cholesky (-inf when H is not positive definite)
//   decimate_to_count  (lod.rs:13-38)   the target_count highest-scored splats, score-descending
//
// MI355X shape.  The reference holds H as an [N,6,6] f32 tensor (144 MB at 1 M splats) and adds a broadcast outer product of
// the whole tensor per view.  Here H is its 21 lower-triangle entries as planes of N floats ([21,N]: entry (i,k), i >= k, is
// plane i(i+1)/2 + k), so the accumulate's 21 read-modify-writes and the log-det's 21 loads are coalesced across lanes.  Per view
// only the splats that reached a pixel get a gradient; every other row of v_transforms is zero, and adding +-0 to an accumulator
// that starts at +0 changes nothing, bit for bit: the kernel skips such rows.
// The ordered top-k maps each score to a u32 key whose ascending stable radix sort is the reference's stable descending
// sort_by, then gathers the kept rows.
#include "context.h"

namespace bh {

constexpr int LOD_WG = 256;
constexpr uint32_t LOD_MAX_BLOCKS = 2048;   // memory-bound passes: grid-stride beyond this
constexpr int PUP_PLANES = 21;

static uint32_t lod_blocks(uint64_t work) {
    const uint64_t b = (work + LOD_WG - 1) / LOD_WG;
    return (uint32_t)(b < LOD_MAX_BLOCKS ? (b ? b : 1) : LOD_MAX_BLOCKS);
}

// lod.rs:120-126: outer = j_col * j_row; hessian_accum = hessian_accum + outer — one f32 multiply, then one f32 add (the build has
// -ffp-contract=off: no FMA).  rows == NULL: rows 0..count-1; else the `count` listed rows (ids >= n are ignored).
__global__ __launch_bounds__(LOD_WG) void pup_accumulate_kernel(const float* __restrict__ v_transforms, uint32_t n,
                                                                const uint32_t* __restrict__ rows, uint32_t count, float* __restrict__ hessian) {
    for (uint32_t t = blockIdx.x * LOD_WG + threadIdx.x; t < count; t += gridDim.x * LOD_WG) {
        const uint32_t r = rows ? rows[t] : t;
        if (r >= n) continue;
        const float* g = v_transforms + (size_t)r * 10;
        const float j[6] = {g[0], g[1], g[2], g[7], g[8], g[9]};
        // a row of +-0 adds +-0 everywhere: skipping it is bit-identical (the sum starts at +0 and never becomes -0)
        if (j[0] == 0.0f && j[1] == 0.0f && j[2] == 0.0f && j[3] == 0.0f && j[4] == 0.0f && j[5] == 0.0f) continue;
        float* h = hessian + r;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int k = 0; k <= i; ++k) {
                float* p = h + (size_t)(i * (i + 1) / 2 + k) * n;   // 64-bit offsets: 21 N passes 2^31 at ~100 M splats
                const float outer = j[i] * j[k];
                *p = *p + outer;
            }
        }
    }
}

// log_det_6x6 (lod.rs:44-70) in its loop order, f32, no FMA; divide and sqrt correctly rounded (the hipcc default).  A pivot
// `diag <= 0` gives -inf; a NaN pivot fails that test and propagates, as in the reference.
__global__ __launch_bounds__(LOD_WG) void pup_scores_kernel(const float* __restrict__ hessian, uint32_t n, float* __restrict__ scores) {
    const uint32_t s = blockIdx.x * LOD_WG + threadIdx.x;
    if (s >= n) return;
    float m[PUP_PLANES];
#pragma unroll
    for (int e = 0; e < PUP_PLANES; ++e) m[e] = hessian[(size_t)e * n + s];
    float l[PUP_PLANES];   // lower triangle of L, same packing
    float score = 0.0f;
    bool pd = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        if (pd) {
            float sum = 0.0f;
#pragma unroll
            for (int k = 0; k < j; ++k) {
                const float p = l[j * (j + 1) / 2 + k] * l[j * (j + 1) / 2 + k];
                sum = sum + p;
            }
            const float diag = m[j * (j + 1) / 2 + j] - sum;
            if (diag <= 0.0f) {
                pd = false;
            } else {
                const float ljj = sqrtf(diag);
                l[j * (j + 1) / 2 + j] = ljj;
#pragma unroll
                for (int i = j + 1; i < 6; ++i) {
                    float si = 0.0f;
#pragma unroll
                    for (int k = 0; k < j; ++k) {
                        const float p = l[i * (i + 1) / 2 + k] * l[j * (j + 1) / 2 + k];
                        si = si + p;
                    }
                    l[i * (i + 1) / 2 + j] = (m[i * (i + 1) / 2 + j] - si) / ljj;
                }
            }
        }
    }
    if (pd) {
        float log_det = 0.0f;
#pragma unroll
        for (int i = 0; i < 6; ++i) log_det = log_det + logf(l[i * (i + 1) / 2 + i]);
        score = 2.0f * log_det;
    } else {
        score = -__builtin_inff();
    }
    scores[s] = score;
}

// Key whose ascending stable sort is sort_by(|a, b| b.partial_cmp(a).unwrap_or(Equal)) (Rust's sort_by is stable): descending
// score, ties in ascending index.  -0 and +0 compare equal there and get one key; NaN sorts after -inf (a documented choice: the
// reference compares NaN as Equal to everything, which leaves its order unspecified).
BH_DEV uint32_t descending_key(float x) {
    if (x != x) return 0xFFFFFFFFu;
    if (x == 0.0f) x = 0.0f;
    const uint32_t u = __float_as_uint(x);
    const uint32_t ascending = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // monotone in x; -inf -> 0x007FFFFF, +inf -> 0xFF800000
    return ~ascending;                                                        // non-NaN keys lie in [0x007FFFFF, 0xFF800000]
}

__global__ __launch_bounds__(LOD_WG) void score_keys_kernel(const float* __restrict__ scores, uint32_t n, uint32_t* __restrict__ keys) {
    for (uint32_t i = blockIdx.x * LOD_WG + threadIdx.x; i < n; i += gridDim.x * LOD_WG) keys[i] = descending_key(scores[i]);
}

// Tensor::select(0, keep) of every per-splat tensor (lod.rs:33-37), plus min_scale.  Element-parallel: the writes are coalesced.
__global__ __launch_bounds__(LOD_WG) void lod_gather_kernel(const uint32_t* __restrict__ ids, uint32_t count, uint32_t c3,
                                                            const float* __restrict__ transforms, const float* __restrict__ sh,
                                                            const float* __restrict__ raw_opac, const float* __restrict__ min_scale,
                                                            float* __restrict__ out_t, float* __restrict__ out_sh, float* __restrict__ out_o,
                                                            float* __restrict__ out_ms, uint32_t* __restrict__ keep_idx) {
    const uint64_t stride = (uint64_t)gridDim.x * LOD_WG, t0 = (uint64_t)blockIdx.x * LOD_WG + threadIdx.x;
    for (uint64_t e = t0; e < (uint64_t)count * 10; e += stride) out_t[e] = transforms[(size_t)ids[e / 10] * 10 + e % 10];
    for (uint64_t e = t0; e < (uint64_t)count * c3; e += stride) out_sh[e] = sh[(size_t)ids[e / c3] * c3 + e % c3];
    for (uint64_t e = t0; e < count; e += stride) {
        const uint32_t src = ids[e];
        out_o[e] = raw_opac[src];
        if (min_scale) out_ms[e] = min_scale[src];
        if (keep_idx) keep_idx[e] = src;
    }
}

__global__ __launch_bounds__(LOD_WG) void iota_kernel(uint32_t* __restrict__ out, uint32_t n) {
    for (uint32_t i = blockIdx.x * LOD_WG + threadIdx.x; i < n; i += gridDim.x * LOD_WG) out[i] = i;
}

static int launch_pup_accumulate(bh_ctx* ctx, const float* v_transforms, uint32_t n, const uint32_t* rows, uint32_t count, float* hessian) {
    if (count == 0 || n == 0) return 0;
    hipLaunchKernelGGL(pup_accumulate_kernel, dim3(lod_blocks(count)), dim3(LOD_WG), 0, ctx->stream, v_transforms, n, rows, count, hessian);
    BH_LAUNCH_CHECK(ctx, "pup_accumulate_kernel");
    return 0;
}

}  // namespace bh

using namespace bh;

extern "C" {

int bh_pup_accumulate(bh_ctx* ctx, const float* v_transforms, uint32_t n, const uint32_t* rows, uint32_t m, float* hessian) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (n > 0 && (!v_transforms || !hessian)) return set_error(ctx, BH_ERR_INVALID_ARG, "pup_accumulate: null argument");
    if (rows && m > 0 && n == 0) return set_error(ctx, BH_ERR_INVALID_ARG, "pup_accumulate: a row list for an empty scene");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    ProfScope ps(ctx, "PupAccumulate");
    return launch_pup_accumulate(ctx, v_transforms, n, rows, rows ? m : n, hessian);
}

int bh_pup_accumulate_view(bh_ctx* ctx, const BhCamera* cam, uint32_t n, uint32_t sh_degree, const float* transforms, const float* sh_coeffs,
                           const float* raw_opacities, const float* min_scale, uint32_t flags, const uint32_t* gt_packed, float* hessian) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!cam || !gt_packed) return set_error(ctx, BH_ERR_INVALID_ARG, "pup_accumulate_view: null argument");
    if (n > 0 && (!transforms || !sh_coeffs || !raw_opacities || !hessian)) return set_error(ctx, BH_ERR_INVALID_ARG, "pup_accumulate_view: null splat tensor");
    if (sh_degree > 4) return set_error(ctx, BH_ERR_INVALID_ARG, "sh_degree must be 0..4");
    if (n == 0) return 0;
    BH_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t W = cam->img_w, H = cam->img_h, C = (sh_degree + 1) * (sh_degree + 1);
    const size_t hw = (size_t)W * H;
    auto* grads = (float*)ensure(ctx, SLOT_LOD_GRADS, (size_t)n * (12 + 3 * C) * 4);
    auto* loss = (float*)ensure(ctx, SLOT_LOD_LOSS, (hw * 4 + 4) * 4);
    if (!grads || !loss) return BH_ERR_OOM;
    float* v_t = grads;
    float* v_sh = v_t + (size_t)n * 10;
    float* v_op = v_sh + (size_t)n * 3 * C;
    float* v_rf = v_op + n;
    float* v_output = loss + 4;   // (16-byte aligned)

    // gaussian_splats.rs:379-386: the renderer sees fold_min_scale(params) when the splats carry a floor
    const float* r_t = transforms;
    const float* r_o = raw_opacities;
    if (min_scale) {
        auto* folded = (float*)ensure(ctx, SLOT_LOD_FOLDED, (size_t)n * 11 * 4);
        if (!folded) return BH_ERR_OOM;
        ProfScope ps(ctx, "FoldMinScale");
        BH_TRY(launch_fold_min_scale(ctx, transforms, raw_opacities, min_scale, n, folded, folded + (size_t)n * 10));
        r_t = folded;
        r_o = folded + (size_t)n * 10;
    }
    // lod.rs:98: render_splats(.., Vec3::ZERO) — complete lists, background 0
    const float bg[3] = {0.0f, 0.0f, 0.0f};
    BhRenderOut ro;
    BH_TRY(bh_render_forward(ctx, cam, n, sh_degree, r_t, sh_coeffs, r_o, bg, BH_FLAG_BWD_INFO | (flags & BH_FLAG_MIP), &ro));
    {
        // lod.rs:102-110: image_loss(pred_rgb, gt, l1 1, ssim 0, no composite, no mask).mean() — mean over H, W, 3
        ProfScope ps(ctx, "PupLoss");
        BhLossConfig lc{};
        lc.l1_weight = 1.0f;
        BH_TRY(bh_image_loss_value_and_grad(ctx, ro.out_img, gt_packed, H, W, &lc, 0.0f, loss, v_output));
    }
    BH_TRY(bh_render_backward_saved(ctx, &ro, v_output, r_t, sh_coeffs, r_o, v_t, v_sh, v_op, v_rf));
    if (min_scale) {
        ProfScope ps(ctx, "FoldMinScaleBackward");
        BH_TRY(launch_fold_min_scale_backward(ctx, transforms, raw_opacities, min_scale, n, v_t, v_op));
    }
    // Dense over all n rows, not over the visible list: rows of splats that got no gradient are +-0 and skipped after a 24-byte read,
    // and the rest are visited in index order.  Same bits as the row list (global_from_compact_gid[0:num_visible]), which visits the
    // visible rows in depth order, i.e. at random: 72 us against 24 us per 1080p view of 1 M splats (scripts/lod_probe.py).
    ProfScope ps(ctx, "PupAccumulate");
    return launch_pup_accumulate(ctx, v_t, n, nullptr, n, hessian);
}

int bh_pup_scores(bh_ctx* ctx, const float* hessian, uint32_t n, float* scores) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (n > 0 && (!hessian || !scores)) return set_error(ctx, BH_ERR_INVALID_ARG, "pup_scores: null argument");
    if (n == 0) return 0;
    BH_HIP(ctx, hipSetDevice(ctx->device));
    ProfScope ps(ctx, "PupScores");
    hipLaunchKernelGGL(pup_scores_kernel, dim3((n + LOD_WG - 1) / LOD_WG), dim3(LOD_WG), 0, ctx->stream, hessian, n, scores);
    BH_LAUNCH_CHECK(ctx, "pup_scores_kernel");
    return 0;
}

int bh_decimate_to_count(bh_ctx* ctx, const float* scores, uint32_t n, uint32_t target_count, uint32_t num_coeffs, const float* transforms,
                         const float* sh_coeffs, const float* raw_opacities, const float* min_scale, float* out_transforms, float* out_sh,
                         float* out_raw_opacities, float* out_min_scale, uint32_t* keep_idx) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    const uint32_t count = target_count < n ? target_count : n;
    if (num_coeffs == 0 || num_coeffs > 25) return set_error(ctx, BH_ERR_INVALID_ARG, "decimate_to_count: num_coeffs must be (d+1)^2, d <= 4");
    if (n > 0 && (!scores || !transforms || !sh_coeffs || !raw_opacities)) return set_error(ctx, BH_ERR_INVALID_ARG, "decimate_to_count: null input");
    if (count > 0 && (!out_transforms || !out_sh || !out_raw_opacities || (min_scale && !out_min_scale)))
        return set_error(ctx, BH_ERR_INVALID_ARG, "decimate_to_count: null output");
    if (count == 0) return 0;
    BH_HIP(ctx, hipSetDevice(ctx->device));
    ProfScope ps(ctx, "DecimateToCount");
    const uint32_t c3 = 3 * num_coeffs;
    if (target_count >= n) {
        // lod.rs:15-17: the splats unchanged, in their order
        if (out_transforms != transforms) BH_HIP(ctx, hipMemcpyAsync(out_transforms, transforms, (size_t)n * 40, hipMemcpyDeviceToDevice, ctx->stream));
        if (out_sh != sh_coeffs) BH_HIP(ctx, hipMemcpyAsync(out_sh, sh_coeffs, (size_t)n * c3 * 4, hipMemcpyDeviceToDevice, ctx->stream));
        if (out_raw_opacities != raw_opacities)
            BH_HIP(ctx, hipMemcpyAsync(out_raw_opacities, raw_opacities, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        if (min_scale && out_min_scale != min_scale)
            BH_HIP(ctx, hipMemcpyAsync(out_min_scale, min_scale, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        if (keep_idx) {
            hipLaunchKernelGGL(iota_kernel, dim3(lod_blocks(n)), dim3(LOD_WG), 0, ctx->stream, keep_idx, n);
            BH_LAUNCH_CHECK(ctx, "iota_kernel");
        }
        return 0;
    }
    auto* sort = (uint32_t*)ensure(ctx, SLOT_LOD_SORT, (size_t)n * 3 * 4);
    if (!sort) return BH_ERR_OOM;
    uint32_t* keys = sort;
    uint32_t* keys_sorted = sort + n;
    uint32_t* ids = sort + 2 * (size_t)n;
    hipLaunchKernelGGL(score_keys_kernel, dim3(lod_blocks(n)), dim3(LOD_WG), 0, ctx->stream, scores, n, keys);
    BH_LAUNCH_CHECK(ctx, "score_keys_kernel");
    BH_TRY(radix_argsort(ctx, keys, nullptr, n, 32, keys_sorted, ids));   // stable: ties keep ascending index
    hipLaunchKernelGGL(lod_gather_kernel, dim3(lod_blocks((uint64_t)count * (c3 > 10 ? c3 : 10))), dim3(LOD_WG), 0, ctx->stream, ids, count, c3,
                       transforms, sh_coeffs, raw_opacities, min_scale, out_transforms, out_sh, out_raw_opacities, out_min_scale, keep_idx);
    BH_LAUNCH_CHECK(ctx, "lod_gather_kernel");
    return 0;
}

}  // extern "C"
