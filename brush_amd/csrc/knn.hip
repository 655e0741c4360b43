// knn.hip — compute_knn_scales: every point's initial log-scale from the distances to its two nearest other points, by an
// exact search on the device.
//
// Reference: brush-train/src/splat_init.rs:179-216 (compute_knn_scales), called by to_init_splats (:218-242) when a point cloud
// (COLMAP points3D, an init.ply without scale_*) starts a run (brush-process/src/train_stream.rs:100-123).  The reference
// builds a ball tree on the host and queries it with rayon: log(clamp((d1 + d2) / 4, 1e-3, 0.1 median_size)), d1 <= d2 the
// f32 glam distances sqrt((dx*dx + dy*dy) + dz*dz) to the two nearest rows j != i, median_size = max(2 * middle extent of
// bounds_from_pos(0.75), 0.01).  Fewer than three points: every log-scale is 0.
//
// Non-finite rows (any coordinate NaN / +-inf) are undefined in the reference (whatever the ball tree does with them).  Here a
// non-finite row is nobody's neighbour and a missing neighbour is at +inf: a non-finite row, and a finite row with fewer than
// two finite neighbours, gets the upper clamp ln(0.1 median_size); nn_dist holds +inf for what is missing.
//
// MI355X shape (an exact search that is not quadratic):
//   order   every finite point gets a 30-bit Morton key of its per-axis RANKS quantised to 10 bits (three 32-bit radix sorts
//           give the ranks: a cloud of far outliers does not squeeze the dense part into a few cells), non-finite rows
//           0xFFFFFFFF (they sort last and drop out); one more radix sort orders the rows; the M finite positions are gathered
//           into SoA x[] y[] z[] in that order.
//   tree    implicit: leaf l = sorted points [64 l, 64 l + 64) with one AABB, level k + 1 = fixed groups of KNN_FAN boxes of
//           level k.  Only the level arrays of boxes are stored (32 B per box).
//   query   one wave per leaf: its 64 queries are spatial neighbours.  Each lane seeds its best two from its own leaf, then the
//           wave walks the tree with ONE stack (LDS): a node is visited when some lane's f32 box distance can still beat that
//           lane's current second-best (__ballot), children are pushed nearest-first (to the leaf's box centre).  A visited leaf
//           is staged in LDS once (coalesced) and every lane tests all its points, read as LDS broadcasts.
//   prune   the comparisons run on the f32 squared sum s = (dx*dx + dy*dy) + dz*dz: sqrt is correctly rounded and monotone, so
//           the two smallest s give the two smallest f32 distances bit for bit.  The box bound is computed with the same
//           operations on the per-axis gaps, which rounding keeps <= the s of every point inside the box; the prune still
//           keeps KNN_SLACK = 8 ulp of relative slack (visit when box_s * (1 - 8 eps) <= best_s2), so a tie or near-tie is never
//           dropped (lattices, duplicates).
//   work    every wave counts the (query, point) distance evaluations it performs (active lanes x points of each leaf it
//           tests, its own leaf included) and adds them to one u64 with one atomic: the machine-independent evidence that the
//           prune works (a brute force is N per point).
//
// Workspace: arena slot SLOT_KNN, 28 B per point + 32 B per 64 points (+ a few boxes): axis / Morton keys [N] | sorted keys [N] |
// order [N] | rank cells [N] | x y z [M] | boxes; the radix sorts use their own slots (16 B per point).  bh_splat_bounds, which
// this calls for median_size, uses 12 B per point of its own.  The call blocks (the bounds readback).
#include <algorithm>
#include <cmath>

#include "context.h"

namespace bh {

namespace {

constexpr int KNN_WG = 256;
constexpr int KNN_LEAF = 64;          // points per leaf = lanes per query wave
constexpr uint32_t KNN_FAN = 16;      // child boxes per node of the upper levels
constexpr int KNN_MAX_LEVELS = 8;     // 2^32 points: 2^26 leaves -> 2^22 -> ... -> 4 -> 1
constexpr int KNN_STACK = 128;        // >= 1 + (KNN_MAX_LEVELS - 1) * (KNN_FAN - 1) = 106 entries
constexpr float KNN_SLACK = 1.0f - 8.0f * 1.1920928955078125e-7f;   // 1 - 8 eps

struct KnnTree {
    uint32_t m;                        // finite points (= sorted positions 0..m-1)
    uint32_t levels;                   // level 0 = leaves; level levels-1 has one box
    uint32_t count[KNN_MAX_LEVELS];    // boxes per level
    uint32_t offset[KNN_MAX_LEVELS];   // first box of each level in the box array
};

// f32::total_cmp order as an unsigned key; non-finite values go last (as in refine.hip's bounds keys)
BH_DEV uint32_t knn_axis_key(float v) {
    if (!is_finite_f32(v)) return 0xFFFFFFFFu;
    const uint32_t b = f2u(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

BH_DEV uint32_t spread10(uint32_t x) {   // 10 bits -> every third bit of 30
    x &= 0x3FFu;
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

__global__ __launch_bounds__(KNN_WG) void knn_axis_keys_kernel(uint32_t n, const float* __restrict__ transforms, int axis, uint32_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * KNN_WG + threadIdx.x;
    if (i < n) keys[i] = knn_axis_key(transforms[(size_t)i * 10 + axis]);
}

// rank r of the axis sort -> 10-bit cell coordinate of row perm[r], packed into cells[row] at bits 10 axis .. 10 axis + 9
__global__ __launch_bounds__(KNN_WG) void knn_rank_cells_kernel(uint32_t n, const uint32_t* __restrict__ perm, int axis, uint32_t* __restrict__ cells) {
    const uint32_t r = blockIdx.x * KNN_WG + threadIdx.x;
    if (r >= n) return;
    const uint32_t row = perm[r];
    const uint32_t q = (uint32_t)(((uint64_t)r << 10) / n);
    cells[row] = axis == 0 ? q : (cells[row] | (q << (10 * axis)));
}

// Morton key of a finite row's cell, 0xFFFFFFFF for a non-finite row
__global__ __launch_bounds__(KNN_WG) void knn_morton_kernel(uint32_t n, const float* __restrict__ transforms, const uint32_t* __restrict__ cells,
                                                           uint32_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * KNN_WG + threadIdx.x;
    if (i >= n) return;
    const float* t = transforms + (size_t)i * 10;
    const bool fin = is_finite_f32(t[0]) && is_finite_f32(t[1]) && is_finite_f32(t[2]);
    const uint32_t c = cells[i];
    keys[i] = fin ? (spread10(c) << 2) | (spread10(c >> 10) << 1) | spread10(c >> 20) : 0xFFFFFFFFu;
}

// the number of finite rows = the position of the first 0xFFFFFFFF in the sorted keys (a Morton key is < 2^30): the one thread at
// the boundary writes it (ctl[0] stays 0 when there is no finite row).  No counting atomics: 10^5 waves adding to one word
// serialise (~1.8 ms at 10 M rows).
__global__ __launch_bounds__(KNN_WG) void knn_count_finite_kernel(uint32_t n, const uint32_t* __restrict__ sorted, uint32_t* __restrict__ ctl) {
    const uint32_t s = blockIdx.x * KNN_WG + threadIdx.x;
    if (s >= n || sorted[s] == 0xFFFFFFFFu) return;
    if (s + 1 == n || sorted[s + 1] == 0xFFFFFFFFu) ctl[0] = s + 1;
}

__global__ __launch_bounds__(KNN_WG) void knn_gather_kernel(uint32_t m, const float* __restrict__ transforms, const uint32_t* __restrict__ order,
                                                           float* __restrict__ xs, float* __restrict__ ys, float* __restrict__ zs) {
    const uint32_t s = blockIdx.x * KNN_WG + threadIdx.x;
    if (s >= m) return;
    const float* t = transforms + (size_t)order[s] * 10;
    xs[s] = t[0];
    ys[s] = t[1];
    zs[s] = t[2];
}

// one wave per leaf: the AABB of its (up to) 64 points.  boxes: [2] float4 per box (min xyz, max xyz)
__global__ __launch_bounds__(KNN_WG) void knn_leaf_boxes_kernel(uint32_t m, uint32_t leaves, const float* __restrict__ xs, const float* __restrict__ ys,
                                                               const float* __restrict__ zs, float4* __restrict__ boxes) {
    const uint32_t leaf = blockIdx.x * (KNN_WG / KNN_LEAF) + threadIdx.x / KNN_LEAF;
    if (leaf >= leaves) return;   // wave-uniform
    const uint32_t s = leaf * KNN_LEAF + (threadIdx.x & (KNN_LEAF - 1));
    const float inf = __builtin_inff();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    if (s < m) {
        lo[0] = hi[0] = xs[s];
        lo[1] = hi[1] = ys[s];
        lo[2] = hi[2] = zs[s];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = __builtin_fminf(lo[k], __shfl_xor(lo[k], off));
            hi[k] = __builtin_fmaxf(hi[k], __shfl_xor(hi[k], off));
        }
    }
    if ((threadIdx.x & (KNN_LEAF - 1)) == 0) {
        boxes[2 * (size_t)leaf] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        boxes[2 * (size_t)leaf + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

// one thread per box of the next level: the union of its KNN_FAN children
__global__ __launch_bounds__(KNN_WG) void knn_node_boxes_kernel(uint32_t parents, uint32_t children, const float4* __restrict__ child_boxes,
                                                               float4* __restrict__ boxes) {
    const uint32_t p = blockIdx.x * KNN_WG + threadIdx.x;
    if (p >= parents) return;
    const float inf = __builtin_inff();
    float4 lo = make_float4(inf, inf, inf, 0.0f), hi = make_float4(-inf, -inf, -inf, 0.0f);
    const uint32_t end = std::min(children, (p + 1) * KNN_FAN);
    for (uint32_t c = p * KNN_FAN; c < end; ++c) {
        const float4 a = child_boxes[2 * (size_t)c], b = child_boxes[2 * (size_t)c + 1];
        lo.x = __builtin_fminf(lo.x, a.x); lo.y = __builtin_fminf(lo.y, a.y); lo.z = __builtin_fminf(lo.z, a.z);
        hi.x = __builtin_fmaxf(hi.x, b.x); hi.y = __builtin_fmaxf(hi.y, b.y); hi.z = __builtin_fmaxf(hi.z, b.z);
    }
    boxes[2 * (size_t)p] = lo;
    boxes[2 * (size_t)p + 1] = hi;
}

// f32 squared distance from q to the box, with the operations of the point distance on the per-axis gaps: never above the s
// of a point inside the box (rounding is monotone)
BH_DEV float box_s(float qx, float qy, float qz, float4 lo, float4 hi) {
    const float gx = __builtin_fmaxf(__builtin_fmaxf(lo.x - qx, qx - hi.x), 0.0f);
    const float gy = __builtin_fmaxf(__builtin_fmaxf(lo.y - qy, qy - hi.y), 0.0f);
    const float gz = __builtin_fmaxf(__builtin_fmaxf(lo.z - qz, qz - hi.z), 0.0f);
    return (gx * gx + gy * gy) + gz * gz;
}

// every lane tests its query against the (up to) 64 points of one leaf, staged in LDS.  SELF: the wave's own leaf (lane k is the
// query itself and is skipped).  Returns the number of points in the leaf.
template <bool SELF>
BH_DEV uint32_t knn_visit_leaf(uint32_t leaf, uint32_t m, const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                               float4* pts, float qx, float qy, float qz, float& b1, float& b2) {
    const uint32_t lane = threadIdx.x;
    const uint32_t base = leaf * KNN_LEAF;
    const uint32_t cnt = std::min((uint32_t)KNN_LEAF, m - base);
    const float inf = __builtin_inff();
    __syncthreads();   // (the previous leaf's reads are done)
    const uint32_t s = base + lane;
    float4 p = make_float4(inf, inf, inf, 0.0f);   // +inf: never inserted
    if (lane < cnt) p = make_float4(xs[s], ys[s], zs[s], 0.0f);
    pts[lane] = p;
    __syncthreads();
#pragma unroll 16
    for (uint32_t k = 0; k < (uint32_t)KNN_LEAF; ++k) {
        const float4 p = pts[k];   // same address in every lane: a broadcast
        const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
        float d = (dx * dx + dy * dy) + dz * dz;
        if (SELF && k == lane) d = inf;
        // the two smallest of {b1, b2, d}, b1 <= b2
        b2 = __builtin_fmaxf(b1, __builtin_fminf(d, b2));
        b1 = __builtin_fminf(b1, d);
    }
    return cnt;
}

__global__ __launch_bounds__(KNN_LEAF) void knn_query_kernel(KnnTree t, uint32_t n, const float* __restrict__ xs, const float* __restrict__ ys,
                                                            const float* __restrict__ zs, const float4* __restrict__ boxes,
                                                            const uint32_t* __restrict__ order, float upper, int zero_scales,
                                                            float* __restrict__ transforms, float* __restrict__ nn_dist,
                                                            unsigned long long* __restrict__ pairs) {
    __shared__ float4 pts[KNN_LEAF];
    __shared__ uint32_t stack[KNN_STACK];
    const uint32_t lane = threadIdx.x;
    const uint32_t w = blockIdx.x;
    const uint32_t s = w * KNN_LEAF + lane;
    const uint32_t m = t.m;
    const float inf = __builtin_inff();
    float b1 = inf, b2 = inf;
    const bool active = s < m;
    if (w < t.count[0]) {   // wave-uniform: a leaf of finite points (waves behind the last one hold non-finite rows only)
        float qx = 0.0f, qy = 0.0f, qz = 0.0f;
        if (active) { qx = xs[s]; qy = ys[s]; qz = zs[s]; }
        const uint32_t lanes = (uint32_t)__popcll(__ballot(active));
        uint64_t work = (uint64_t)lanes * knn_visit_leaf<true>(w, m, xs, ys, zs, pts, qx, qy, qz, b1, b2);
        if (t.levels > 1) {
            // the own leaf's box centre orders the children of a node nearest-first
            const float4 olo = boxes[2 * (size_t)w], ohi = boxes[2 * (size_t)w + 1];
            const float cx = (olo.x + ohi.x) * 0.5f, cy = (olo.y + ohi.y) * 0.5f, cz = (olo.z + ohi.z) * 0.5f;
            if (lane == 0) stack[0] = (t.levels - 1) << 28;
            uint32_t sp = 1;
            __syncthreads();
            while (sp > 0) {
                --sp;
                const uint32_t node = __builtin_amdgcn_readfirstlane(stack[sp]);
                const uint32_t lvl = node >> 28, idx = node & 0x0FFFFFFFu;
                if (lvl == 0 && idx == w) continue;
                const size_t bi = 2 * ((size_t)t.offset[lvl] + idx);
                const float4 lo = boxes[bi], hi = boxes[bi + 1];
                const bool want = active && box_s(qx, qy, qz, lo, hi) * KNN_SLACK <= b2;
                if (__ballot(want) == 0) continue;
                if (lvl == 0) {
                    work += (uint64_t)lanes * knn_visit_leaf<false>(idx, m, xs, ys, zs, pts, qx, qy, qz, b1, b2);
                    continue;
                }
                const uint32_t first = idx * KNN_FAN;
                const uint32_t nc = std::min(KNN_FAN, t.count[lvl - 1] - first);
                float key = inf;
                if (lane < nc) {
                    const size_t ci = 2 * ((size_t)t.offset[lvl - 1] + first + lane);
                    key = box_s(cx, cy, cz, boxes[ci], boxes[ci + 1]);
                }
                uint32_t rank = 0;   // position of this child in ascending (key, lane) order
#pragma unroll
                for (uint32_t k = 0; k < KNN_FAN; ++k) {
                    const float kk = __shfl(key, (int)k);
                    rank += (k < nc && (kk < key || (kk == key && k < lane))) ? 1u : 0u;
                }
                __syncthreads();   // (every lane has read the popped entry)
                if (lane < nc) stack[sp + (nc - 1u - rank)] = ((lvl - 1) << 28) | (first + lane);   // nearest on top
                sp += nc;
                __syncthreads();
            }
        }
        if (lane == 0 && pairs) atomicAdd(pairs, (unsigned long long)work);
    }
    if (s >= n) return;
    const uint32_t row = order[s];
    // (an inactive lane of the last leaf ran the tests with q = 0: its row is non-finite and has no neighbour)
    const float d1 = active ? __builtin_sqrtf(b1) : inf, d2 = active ? __builtin_sqrtf(b2) : inf;   // correctly rounded (the hipcc default)
    float dist = (d1 + d2) / 4.0f;
    if (dist < 1e-3f) dist = 1e-3f;   // f32::clamp(1e-3, upper)
    if (dist > upper) dist = upper;
    const float ls = zero_scales ? 0.0f : bh_logf(dist);
    float* tr = transforms + (size_t)row * 10;
    tr[7] = ls;
    tr[8] = ls;
    tr[9] = ls;
    if (nn_dist) {
        nn_dist[2 * (size_t)row] = d1;
        nn_dist[2 * (size_t)row + 1] = d2;
    }
}

inline uint32_t knn_blocks(uint64_t n) { return (uint32_t)((n + KNN_WG - 1) / KNN_WG); }

}  // namespace

}  // namespace bh

using namespace bh;

extern "C" {

int bh_knn_log_scales(bh_ctx* ctx, float* transforms, uint32_t n, float* nn_dist, uint64_t* pairs_tested) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (pairs_tested) *pairs_tested = 0;
    if (n == 0) return 0;
    if (!transforms) return set_error(ctx, BH_ERR_INVALID_ARG, "knn_log_scales: null transforms");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    // [4] u32 control (finite count, pad, pairs u64) | keys [N] | sorted keys [N] | order [N] | cells [N] | x y z [N] | boxes
    uint64_t leaves_max = (n + KNN_LEAF - 1) / KNN_LEAF, boxes_max = 0;
    for (uint64_t c = leaves_max; ; c = (c + KNN_FAN - 1) / KNN_FAN) {
        boxes_max += c;
        if (c <= 1) break;
    }
    const size_t words = 4 + (size_t)n * 7 + 4;   // (+4: the boxes start 16-byte aligned)
    uint32_t* buf = (uint32_t*)ensure(ctx, SLOT_KNN, words * 4 + boxes_max * 32);
    if (!buf) return BH_ERR_OOM;
    uint32_t* ctl = buf;
    unsigned long long* pairs = (unsigned long long*)(buf + 2);
    uint32_t* keys = buf + 4;
    uint32_t* sorted = keys + n;
    uint32_t* order = sorted + n;
    uint32_t* cells = order + n;
    float* xs = (float*)(cells + n);
    float* ys = xs + n;
    float* zs = ys + n;
    float4* boxes = (float4*)(((uintptr_t)(zs + n) + 15) & ~(uintptr_t)15);
    BH_HIP(ctx, hipMemsetAsync(ctl, 0, 16, ctx->stream));
    for (int axis = 0; axis < 3; ++axis) {   // per-axis ranks -> 10-bit cells
        hipLaunchKernelGGL(knn_axis_keys_kernel, dim3(knn_blocks(n)), dim3(KNN_WG), 0, ctx->stream, n, transforms, axis, keys);
        BH_LAUNCH_CHECK(ctx, "knn_axis_keys_kernel");
        BH_TRY(radix_argsort(ctx, keys, nullptr, n, 32, sorted, order));
        hipLaunchKernelGGL(knn_rank_cells_kernel, dim3(knn_blocks(n)), dim3(KNN_WG), 0, ctx->stream, n, order, axis, cells);
        BH_LAUNCH_CHECK(ctx, "knn_rank_cells_kernel");
    }
    hipLaunchKernelGGL(knn_morton_kernel, dim3(knn_blocks(n)), dim3(KNN_WG), 0, ctx->stream, n, transforms, cells, keys);
    BH_LAUNCH_CHECK(ctx, "knn_morton_kernel");
    BH_TRY(radix_argsort(ctx, keys, nullptr, n, 32, sorted, order));
    hipLaunchKernelGGL(knn_count_finite_kernel, dim3(knn_blocks(n)), dim3(KNN_WG), 0, ctx->stream, n, sorted, ctl);
    BH_LAUNCH_CHECK(ctx, "knn_count_finite_kernel");
    // the finite count travels to the host with the bounds readback (pinned word 8: behind the six bounds picks)
    uint32_t* host_m = ctx->host_counters + 8;
    BH_HIP(ctx, hipMemcpyAsync(host_m, ctl, 4, hipMemcpyDeviceToHost, ctx->stream));
    float center[3], extent[3];
    BH_TRY(bh_splat_bounds(ctx, transforms, n, 0.75f, center, extent));   // bounds_from_pos(0.75); blocks
    const uint32_t m = *reinterpret_cast<volatile uint32_t*>(host_m);
    // BoundingBox::median_size (bounding_box.rs:23-29: extents sorted by total_cmp, the middle one doubled), .max(0.01)
    std::sort(extent, extent + 3, [](float a, float b) { return std::isnan(b) ? !std::isnan(a) : a < b; });
    const float median_size = std::fmax(extent[1] * 2.0f, 0.01f);
    const float upper = median_size * 0.1f;
    KnnTree t{};
    t.m = m;
    uint32_t nb = 0;
    if (m > 0) {
        t.count[0] = (m + KNN_LEAF - 1) / KNN_LEAF;
        t.levels = 1;
        while (t.count[t.levels - 1] > 1) {
            if (t.levels == KNN_MAX_LEVELS) return set_error(ctx, BH_ERR_UNSUPPORTED, "knn_log_scales: tree too deep");
            t.count[t.levels] = (t.count[t.levels - 1] + KNN_FAN - 1) / KNN_FAN;
            ++t.levels;
        }
        for (uint32_t l = 0; l < t.levels; ++l) { t.offset[l] = nb; nb += t.count[l]; }
        hipLaunchKernelGGL(knn_gather_kernel, dim3(knn_blocks(m)), dim3(KNN_WG), 0, ctx->stream, m, transforms, order, xs, ys, zs);
        BH_LAUNCH_CHECK(ctx, "knn_gather_kernel");
        hipLaunchKernelGGL(knn_leaf_boxes_kernel, dim3((t.count[0] + KNN_WG / KNN_LEAF - 1) / (KNN_WG / KNN_LEAF)), dim3(KNN_WG), 0, ctx->stream, m,
                           t.count[0], xs, ys, zs, boxes);
        BH_LAUNCH_CHECK(ctx, "knn_leaf_boxes_kernel");
        for (uint32_t l = 1; l < t.levels; ++l) {
            hipLaunchKernelGGL(knn_node_boxes_kernel, dim3(knn_blocks(t.count[l])), dim3(KNN_WG), 0, ctx->stream, t.count[l], t.count[l - 1],
                               boxes + 2 * (size_t)t.offset[l - 1], boxes + 2 * (size_t)t.offset[l]);
            BH_LAUNCH_CHECK(ctx, "knn_node_boxes_kernel");
        }
    }
    // one wave per 64 sorted rows: the finite ones search, the rest (sorted behind them) take the missing-neighbour outputs
    hipLaunchKernelGGL(knn_query_kernel, dim3((n + KNN_LEAF - 1) / KNN_LEAF), dim3(KNN_LEAF), 0, ctx->stream, t, n, xs, ys, zs,
                       (const float4*)boxes, order, upper, n < 3 ? 1 : 0, transforms, nn_dist, pairs);
    BH_LAUNCH_CHECK(ctx, "knn_query_kernel");
    if (pairs_tested) BH_HIP(ctx, hipMemcpyAsync(ctx->host_counters + 10, pairs, 8, hipMemcpyDeviceToHost, ctx->stream));
    BH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    deliver_pending_loss(ctx);
    if (pairs_tested) {
        const volatile uint32_t* h = ctx->host_counters + 10;
        *pairs_tested = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
    }
    return 0;
}

}  // extern "C"
