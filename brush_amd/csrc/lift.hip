// lift.hip — mask lifting: per-splat blend-weight votes from 2-D label maps, the two contribution statistics of the same pass, and
// the element-wise steps from votes to a choice of splats (include/brush_hip_lift.h).
//
// bh_lift_accumulate is one more pass over the lists a BH_FLAG_BWD_INFO forward saved, as a feature map is: the same splats in the
// same order with the same alpha, cut-off, clamp and saturation rule as the colour blend.  The arithmetic is device_blend.h's one
// copy (blend_alpha, blend_step) behind device_map_blend.h's staging (stage_map_batch) and tile mapping (tile_of_block); the conic
// evaluation in front of it is written as map_forward_kernel writes it, with the forward's pre-test and the forward's early exit
// (every pixel done, checked at a batch's start and every 8th splat): this pass needs no pixel total, so it does not pay for the
// tail the backward replay walks.  Where the forward folds a weight into per-PIXEL accumulators, this kernel sums it per SPLAT:
//
//   * once per tile the distinct labels among the tile's 256 pixels are numbered (a 256-bit presence set in LDS, a label's local
//     index = the set bits below it) and every lane keeps its four pixels' local indices;
//   * the list is walked in PASSES of four local labels (most tiles of a real mask hold one to three: one pass).  Per splat a
//     lane adds its pixels' votes q = rint(w 2^24) into the four u32 sums of the pass; the four leave through ONE register
//     butterfly (device_blend.h: swap32_add_u32 twice, swap16_add_u32, row_allreduce_u32), after which every lane of 16-lane row r
//     holds sum comp(r) = 0 2 1 3; lane 0 of each row issues one 64-bit integer atomic add into votes[gid, label], skipped when the
//     sum is 0.  A splat that contributed nowhere in the tile costs one ballot;
//   * the first pass also takes the two statistics where they are asked for (a template parameter): the count is four ballots and
//     popcounts, the maximum a DPP maximum on the weights' bits; lane 0 issues one u32 atomic max and one u32 atomic add.
//
// Integer sums and an unsigned maximum: nothing depends on the order in which tiles, passes or calls arrive.
#include <cmath>

#include "context.h"
#include "device_map_blend.h"
#include "../../include/brush_hip_lift.h"

namespace bh {

namespace {

// What this pass stages per splat: the six projected floats in the maps' layout, x y c00/2 c01 | c11/2 alpha0 sigma_cut -
struct LiftMap {
    static constexpr int STRIDE = 8;
    struct Attr {};
    struct Rec { float4 s0, s1; };
    static BH_DEV Rec load(const float* p) { return Rec{*reinterpret_cast<const float4*>(p), *reinterpret_cast<const float4*>(p + 4)}; }
    static BH_DEV float cut(const Rec& r) { return r.s1.z; }
    static BH_DEV void stage(float4* d, const float* v, float sigma_cut, const Attr&, uint32_t) {
        d[0] = make_float4(v[0], v[1], 0.5f * v[2], v[3]);
        d[1] = make_float4(0.5f * v[4], v[5], sigma_cut, 0.0f);
    }
};

constexpr uint32_t NO_LABEL = 0xFFFFFFFFu;
constexpr int LIFT_PASS = 4;   // local labels per pass over the lists: what one butterfly carries

struct LiftTables {
    const uint8_t* __restrict__ labels;     // [H,W] or NULL
    uint32_t num_labels;
    unsigned long long* __restrict__ votes; // [N,L]
    uint32_t* __restrict__ max_bits;        // [N] the bits of max_weight, or NULL
    uint32_t* __restrict__ pixel_count;     // [N] or NULL
};

template <bool SMOOTH, bool STATS>
__global__ __launch_bounds__(64, 8) void lift_accumulate_kernel(MapUniforms u, const uint32_t* __restrict__ isect_gids,
                                                                const uint32_t* __restrict__ tile_offsets,
                                                                const uint32_t* __restrict__ tile_offsets_far, const float* __restrict__ projected,
                                                                const uint32_t* __restrict__ global_from_compact_gid, LiftTables tb) {
    __shared__ __attribute__((aligned(16))) float s_splat[MAP_BATCH * LiftMap::STRIDE];
    __shared__ uint32_t s_gid[MAP_BATCH];
    __shared__ uint32_t s_present[BH_LIFT_MAX_LABELS / 32];
    __shared__ uint32_t s_label_of[BH_LIFT_MAX_LABELS];
    const uint32_t local_tile = tile_of_block(blockIdx.x, u.num_tiles, u.band_mode);
    if (local_tile >= u.num_tiles) return;
    const uint32_t tile = u.tile_begin + local_tile;
    const uint32_t lo0 = tile_offsets[tile * 2], hi0 = tile_offsets[tile * 2 + 1];
    uint32_t lo1 = 0u, hi1 = 0u;
    if (tile_offsets_far) { lo1 = tile_offsets_far[tile * 2]; hi1 = tile_offsets_far[tile * 2 + 1]; }
    if (hi0 <= lo0 && hi1 <= lo1) return;
    const int lane = threadIdx.x;
    const uint32_t px0 = (tile % u.tile_bw) * TILE_WIDTH + (lane & 7), py0 = (tile / u.tile_bw) * TILE_WIDTH + (lane >> 3);
    const float pcx[2] = {(float)px0 + 0.5f, (float)(px0 + 8) + 0.5f};
    const float pcy[2] = {(float)py0 + 0.5f, (float)(py0 + 8) + 0.5f};

    // the tile's distinct labels, numbered in ascending order
    if (lane < (int)(BH_LIFT_MAX_LABELS / 32)) s_present[lane] = 0u;
    __syncthreads();
    uint32_t lab[4];
    bool inside[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t px = px0 + 8 * (q & 1), py = py0 + 8 * (q >> 1);
        inside[q] = px < u.img_w && py < u.img_h;
        uint32_t l = NO_LABEL;
        if (inside[q]) l = tb.labels ? (uint32_t)tb.labels[(size_t)py * u.img_w + px] : 0u;
        lab[q] = l < tb.num_labels ? l : NO_LABEL;   // >= num_labels (255 by convention): votes nowhere
        if (lab[q] != NO_LABEL) atomicOr(&s_present[lab[q] >> 5], 1u << (lab[q] & 31u));
    }
    __syncthreads();
    uint32_t distinct = 0u, loc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < BH_LIFT_MAX_LABELS / 32; ++k) {
        const uint32_t word = s_present[k];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t w = lab[q] >> 5;   // (NO_LABEL: beyond every word, loc is overwritten below)
            loc[q] += k < w ? __popc(word) : (k == w ? __popc(word & ((1u << (lab[q] & 31u)) - 1u)) : 0u);
        }
        distinct += __popc(word);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (lab[q] != NO_LABEL) s_label_of[loc[q]] = lab[q];   // (lanes of one label store the same value)
        else loc[q] = NO_LABEL;
    }
    __syncthreads();
    const uint32_t passes = STATS ? max(1u, (distinct + LIFT_PASS - 1u) / LIFT_PASS) : (distinct + LIFT_PASS - 1u) / LIFT_PASS;

    uint32_t sign_mask = 0x80000000u;   // kept in a VGPR, as in the map kernels
    asm volatile("" : "+v"(sign_mask));
    for (uint32_t pass = 0; pass < passes; ++pass) {
        const uint32_t base = pass * LIFT_PASS;
        const bool stats = STATS && pass == 0u;
        uint32_t slot[4];   // which sum of this pass a pixel votes into (>= LIFT_PASS: none; NO_LABEL - base stays >= LIFT_PASS)
        float tr[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            slot[q] = loc[q] - base;
            tr[q] = inside[q] ? 1.0f : -1.0f;
        }
        auto any_live = [&]() {
            bool l = false;
#pragma unroll
            for (int q = 0; q < 4; ++q) l = l || tr[q] > 0.0f;
            return l;
        };
        bool done = false;
#pragma nounroll
        for (int part = 0; part < 2 && !done; ++part) {
            const uint32_t range_lo = part ? lo1 : lo0, range_hi = part ? hi1 : hi0;
            for (uint32_t batch_start = range_lo; batch_start < range_hi && !done; batch_start += MAP_BATCH) {
                if (__ballot(any_live()) == 0ull) { done = true; break; }
                const uint32_t cnt = min((uint32_t)MAP_BATCH, range_hi - batch_start);
                __syncthreads();
                const uint32_t my_cg = stage_map_batch<SMOOTH, LiftMap>(isect_gids, projected, LiftMap::Attr{}, batch_start, cnt, lane, s_splat);
                if ((uint32_t)lane < cnt) s_gid[lane] = global_from_compact_gid[my_cg];
                __syncthreads();
                for (uint32_t t = 0; t < cnt; ++t) {
                    const LiftMap::Rec r = LiftMap::load(&s_splat[t * LiftMap::STRIDE]);
                    const uint32_t cut_bits = f2u(LiftMap::cut(r));
                    float a_xx[2], b_x[2], c_y[2], dy[2];
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const float dx = pcx[k] - r.s0.x;
                        a_xx[k] = (r.s0.z * dx) * dx;
                        b_x[k] = r.s0.w * dx;
                        dy[k] = pcy[k] - r.s0.y;
                        c_y[k] = r.s1.x * dy[k];
                    }
                    uint32_t sum[LIFT_PASS] = {0u, 0u, 0u, 0u}, wmax = 0u, terms = 0u;
                    bool any = false;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int k = q & 1, m = q >> 1;
                        const float half_qv = __builtin_fmaf(c_y[m], dy[m], a_xx[k]);
                        const float sigma = __builtin_fmaf(b_x[k], dy[m], half_qv);
                        const bool pre = ((f2u(tr[q]) & sign_mask) | f2u(sigma)) <= cut_bits;
                        if (__ballot(pre) != 0ull) {
                            const float alpha = blend_alpha(r.s1.y, sigma);
                            float alpha_eff, next_t;
                            bool sat;
                            const bool ok = blend_step<SMOOTH>(alpha, pre, tr[q], alpha_eff, next_t, sat);
                            const bool contrib = ok && !sat;
                            const float w = alpha_eff * tr[q];   // the forward's one f32 product
                            const uint32_t vote = contrib ? (uint32_t)rintf(w * BH_LIFT_VOTE_ONE) : 0u;
#pragma unroll
                            for (int j = 0; j < LIFT_PASS; ++j) sum[j] += slot[q] == (uint32_t)j ? vote : 0u;
                            any = any || (contrib && (stats || slot[q] < (uint32_t)LIFT_PASS));
                            if (stats) {
                                wmax = max(wmax, contrib ? f2u(w) : 0u);
                                terms += (uint32_t)__popcll(__ballot(contrib));
                            }
                            tr[q] = ok ? (sat ? -tr[q] : next_t) : tr[q];
                        }
                    }
                    if (__ballot(any) != 0ull) {
                        const int ri = lane & 15, rrow = lane >> 4;
                        const uint32_t comp = (uint32_t)(((rrow & 1) << 1) | (rrow >> 1));   // which of the four sums this row holds
                        const uint32_t h0 = swap32_add_u32(sum[0], sum[1]), h1 = swap32_add_u32(sum[2], sum[3]);
                        const uint32_t total = row_allreduce_u32(swap16_add_u32(h0, h1));
                        const uint32_t gid = s_gid[t];
                        if (ri == 0 && total != 0u)   // (total != 0 implies base + comp < distinct)
                            __hip_atomic_fetch_add(&tb.votes[(size_t)gid * tb.num_labels + s_label_of[base + comp]], (unsigned long long)total,
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (stats) {
                            const uint32_t top = wave_max_u32(wmax);
                            if (lane == 0) {
                                if (tb.max_bits) __hip_atomic_fetch_max(&tb.max_bits[gid], top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                if (tb.pixel_count) __hip_atomic_fetch_add(&tb.pixel_count[gid], terms, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            }
                        }
                    }
                    if ((t & 7u) == 7u && __ballot(any_live()) == 0ull) { done = true; break; }
                }
            }
        }
    }
}

constexpr uint32_t LIFT_WG = 256;

struct AssignArgs {
    uint32_t n, num_labels;
    unsigned long long min_total;
};

__global__ __launch_bounds__(LIFT_WG) void lift_assign_kernel(AssignArgs a, const unsigned long long* __restrict__ votes, uint8_t* __restrict__ labels_out,
                                                              float* __restrict__ share_out) {
    const uint32_t i = blockIdx.x * LIFT_WG + threadIdx.x;
    if (i >= a.n) return;
    const unsigned long long* row = votes + (size_t)i * a.num_labels;
    unsigned long long total = 0ull, best = 0ull;
    uint32_t arg = 0u;
    for (uint32_t l = 0; l < a.num_labels; ++l) {
        const unsigned long long v = row[l];
        total += v;
        if (v > best) { best = v; arg = l; }   // ties: the lowest label
    }
    const bool assigned = total != 0ull && total >= a.min_total;
    labels_out[i] = assigned ? (uint8_t)arg : (uint8_t)BH_LIFT_UNASSIGNED;
    if (share_out) share_out[i] = assigned ? (float)((double)best / (double)total) : 0.0f;
}

struct SelectArgs {
    BhLiftSelect sel;
    uint32_t n, num_labels;
    unsigned long long min_total;
};

__global__ __launch_bounds__(LIFT_WG) void lift_select_kernel(SelectArgs a, const unsigned long long* __restrict__ votes, const float* __restrict__ max_weight,
                                                              const uint32_t* __restrict__ pixel_count, float* __restrict__ keep) {
    const uint32_t i = blockIdx.x * LIFT_WG + threadIdx.x;
    if (i >= a.n) return;
    bool k = true;
    if (votes) {
        const unsigned long long* row = votes + (size_t)i * a.num_labels;
        unsigned long long total = 0ull;
        for (uint32_t l = 0; l < a.num_labels; ++l) total += row[l];
        k = total != 0ull && total >= a.min_total;
        if (a.sel.label != BH_LIFT_ANY_LABEL) k = k && (double)row[a.sel.label] >= (double)a.sel.min_share * (double)total;
    }
    if (a.sel.min_max_weight > 0.0f) k = k && max_weight[i] >= a.sel.min_max_weight;
    if (a.sel.min_pixels > 0u) k = k && pixel_count[i] >= a.sel.min_pixels;
    if (a.sel.invert) k = !k;
    keep[i] = k ? 1.0f : 0.0f;
}

struct Span {
    const void* p;
    size_t bytes;
};
bool overlaps(const Span& a, const Span& b) {
    if (!a.p || !b.p || a.bytes == 0 || b.bytes == 0) return false;
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

// (uint64_t)rint((double)min_weight * 2^24); not > 0 (or not a number): 0
unsigned long long min_total_of(float min_weight) {
    if (!(min_weight > 0.0f)) return 0ull;
    const double t = std::rint((double)min_weight * 16777216.0);
    return t >= 18446744073709551615.0 ? ~0ull : (unsigned long long)t;
}

}  // namespace

}  // namespace bh

using namespace bh;

extern "C" {

int bh_lift_accumulate(bh_ctx* ctx, const BhRenderOut* saved, const uint8_t* labels, uint32_t num_labels, uint64_t* votes, float* max_weight,
                       uint32_t* pixel_count) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!saved || !votes) return set_error(ctx, BH_ERR_INVALID_ARG, "lift_accumulate: null argument");
    if (num_labels == 0 || num_labels > BH_LIFT_MAX_LABELS) return set_error(ctx, BH_ERR_INVALID_ARG, "lift_accumulate: num_labels must be 1 .. 256");
    const ForwardState* found = nullptr;
    BH_TRY(find_saved_bwd_forward(ctx, saved, BH_ERR_INVALID_ARG, "lift_accumulate", &found));
    const ForwardState& fs = *found;
    const MapUniforms u = map_uniforms(ctx, fs.uniforms);
    const Span spans[4] = {{labels, (size_t)u.img_w * u.img_h}, {votes, (size_t)fs.n * num_labels * 8}, {max_weight, (size_t)fs.n * 4},
                           {pixel_count, (size_t)fs.n * 4}};
    for (int o = 1; o < 4; ++o)
        for (int k = 0; k < o; ++k)
            if (overlaps(spans[o], spans[k])) return set_error(ctx, BH_ERR_INVALID_ARG, "lift_accumulate: an output table overlaps the labels or another table");
    if (fs.out.num_intersections == 0 || fs.out.num_listed_splats == 0 || u.num_tiles == 0) return 0;   // nothing listed: the tables stay
    ProfScope ps(ctx, "LiftAccumulate");
    const BhRenderOut& r = fs.out;
    const LiftTables tb{labels, num_labels, reinterpret_cast<unsigned long long*>(votes), reinterpret_cast<uint32_t*>(max_weight), pixel_count};
    const dim3 grid(band_slots(u.num_tiles) * 8u), block(64);
    const bool smooth = fs.flags & BH_FLAG_SMOOTH_CUTOFF, stats = max_weight || pixel_count;
#define BH_LIFT(S, ST) hipLaunchKernelGGL((lift_accumulate_kernel<S, ST>), grid, block, 0, ctx->stream, u, r.compact_gid_from_isect, r.tile_offsets, \
                                          r.tile_offsets_far, r.projected, r.global_from_compact_gid, tb)
    if (smooth) { if (stats) BH_LIFT(true, true); else BH_LIFT(true, false); }
    else { if (stats) BH_LIFT(false, true); else BH_LIFT(false, false); }
#undef BH_LIFT
    BH_LAUNCH_CHECK(ctx, "lift_accumulate_kernel");
    return 0;
}

int bh_lift_assign(bh_ctx* ctx, const uint64_t* votes, uint32_t n, uint32_t num_labels, float min_weight, uint8_t* labels_out, float* share_out) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (num_labels == 0 || num_labels > BH_LIFT_MAX_LABELS) return set_error(ctx, BH_ERR_INVALID_ARG, "lift_assign: num_labels must be 1 .. 256");
    if (n == 0) return 0;
    if (!votes || !labels_out) return set_error(ctx, BH_ERR_INVALID_ARG, "lift_assign: null argument");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    ProfScope ps(ctx, "LiftAssign");
    const AssignArgs a{n, num_labels, min_total_of(min_weight)};
    hipLaunchKernelGGL(lift_assign_kernel, dim3((n + LIFT_WG - 1) / LIFT_WG), dim3(LIFT_WG), 0, ctx->stream, a,
                       reinterpret_cast<const unsigned long long*>(votes), labels_out, share_out);
    BH_LAUNCH_CHECK(ctx, "lift_assign_kernel");
    return 0;
}

int bh_lift_select(bh_ctx* ctx, const uint64_t* votes, const float* max_weight, const uint32_t* pixel_count, uint32_t n, uint32_t num_labels,
                   const BhLiftSelect* sel, float* keep) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    const char* who = "lift_select";
    if (!sel) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": null selection");
    if (sel->min_share != sel->min_share || sel->min_weight != sel->min_weight || sel->min_max_weight != sel->min_max_weight)
        return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": a threshold is not a number");
    if (votes && (num_labels == 0 || num_labels > BH_LIFT_MAX_LABELS)) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": num_labels must be 1 .. 256");
    if (!votes && (sel->label != BH_LIFT_ANY_LABEL || sel->min_weight > 0.0f))
        return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": a label or a min_weight needs the votes table");
    if (sel->label != BH_LIFT_ANY_LABEL && sel->label >= num_labels) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": label >= num_labels");
    if (sel->min_max_weight > 0.0f && !max_weight) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": min_max_weight needs the max_weight table");
    if (sel->min_pixels > 0u && !pixel_count) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": min_pixels needs the pixel_count table");
    if (n == 0) return 0;
    if (!keep) return set_error(ctx, BH_ERR_INVALID_ARG, std::string(who) + ": null keep");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    ProfScope ps(ctx, "LiftSelect");
    const SelectArgs a{*sel, n, num_labels, min_total_of(sel->min_weight)};
    hipLaunchKernelGGL(lift_select_kernel, dim3((n + LIFT_WG - 1) / LIFT_WG), dim3(LIFT_WG), 0, ctx->stream, a,
                       reinterpret_cast<const unsigned long long*>(votes), max_weight, pixel_count, keep);
    BH_LAUNCH_CHECK(ctx, "lift_select_kernel");
    return 0;
}

}  // extern "C"
