// sort_groups.h — device side of the sorts' group tables (context.h SortGroups): what a scatter block adds up to find its
// offsets, and the histogram kernels' share of clearing the stale set.  Included by sort.hip and depth_sort.hip only.
#pragma once
#include "context.h"

namespace bh {

// Thread `d` (one per digit) of scatter block `b`: the digit's keys in the blocks in front of b (-> before) and in all blocks
// (-> total).  hist: [nblocks][256] block histograms, gsum: [ngroups][256] group totals, or (scanned, block-uniform) their exclusive
// prefixes with the digit totals in totals[256].  Indices are clamped, not predicated: the loads are independent of each other.
BH_DEV void sort_group_offset(const uint32_t* __restrict__ hist, const uint32_t* __restrict__ gsum, const uint32_t* totals, uint32_t ngroups, bool scanned,
                              uint32_t b, uint32_t d, uint32_t& before, uint32_t& total) {
    constexpr uint32_t GB = 16;
    const uint32_t g = b / SORT_GROUP_BLOCKS, bi = b % SORT_GROUP_BLOCKS;
    const uint32_t* hrow = hist + (size_t)(g * SORT_GROUP_BLOCKS) * 256u + d;
    const uint32_t* grow = gsum + d;
    uint32_t hv[SORT_GROUP_BLOCKS - 1], gv[GB];
#pragma unroll
    for (uint32_t j = 0; j < SORT_GROUP_BLOCKS - 1u; ++j) hv[j] = hrow[(size_t)(j < bi ? j : bi) * 256u];   // (row bi: the block's own)
    if (scanned) {
        uint32_t bef = grow[(size_t)g * 256u];
        const uint32_t tot = totals[d];
#pragma unroll
        for (uint32_t j = 0; j < SORT_GROUP_BLOCKS - 1u; ++j) bef += j < bi ? hv[j] : 0u;
        before = bef;
        total = tot;
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < GB; ++j) gv[j] = grow[(size_t)(j < ngroups ? j : ngroups - 1u) * 256u];
    uint32_t bef = 0, tot = 0;
#pragma unroll
    for (uint32_t j = 0; j < SORT_GROUP_BLOCKS - 1u; ++j) bef += j < bi ? hv[j] : 0u;
#pragma unroll
    for (uint32_t j = 0; j < GB; ++j) {
        const uint32_t v = j < ngroups ? gv[j] : 0u;
        tot += v;
        bef += j < g ? v : 0u;
    }
    for (uint32_t g0 = GB; g0 < ngroups; g0 += GB) {   // (at most once more: SORT_DIRECT_GROUPS)
#pragma unroll
        for (uint32_t j = 0; j < GB; ++j) gv[j] = grow[(size_t)(g0 + j < ngroups ? g0 + j : ngroups - 1u) * 256u];
#pragma unroll
        for (uint32_t j = 0; j < GB; ++j) {
            const uint32_t v = g0 + j < ngroups ? gv[j] : 0u;
            tot += v;
            bef += g0 + j < g ? v : 0u;
        }
    }
    before = bef;
    total = tot;
}
// ... and the histogram kernel's share of clearing the stale set (SortGroups), by every block of its grid
BH_DEV void sort_groups_clear(uint32_t* __restrict__ stale, uint32_t stale_words) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < stale_words; i += gridDim.x * blockDim.x) stale[i] = 0u;
}

}  // namespace bh
