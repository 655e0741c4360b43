// depth_deal.h — K1 deals the listed splats straight into the depth sort's buckets (context.h DEALING K1).
//
// The fused depth sort (depth_sort.hip) is a split into 255 buckets followed by one block per bucket.  When the split digit is
// "number of the view's splitters <= key" (SPLITTERS there), the bucket of a splat is known the moment K1 has its key: the
// histogram and split launches — two passes over all n keys to move the listed fifth of them — do nothing K1 cannot do on its
// way out.  A listed lane looks its digit up in the block's LDS copy of the table and takes a slot in the bucket's region
// with ONE returning 64-bit atomic on the bucket's counter word: the low half counts splats (the old value is the slot), the
// high half adds up the tile counts the scan is made of.  Slots are taken in arrival order; the bucket kernel restores the
// stable sort's order (ties by splat id) itself.
//
// What replaces the key-range rule of the histogram kernel (a table whose frame's range has moved is ignored): nothing
// needs to.  ANY ascending table is a correct set of splitters, a stale one only fills the buckets unevenly — and a bucket
// that runs out of slots sets the overflow word, which the host sees with the counts and answers with the three-launch
// path over depth_keys (api.hip).  A table that holds no quantiles (validity word 0) sets the same word.
#pragma once
#include "context.h"

namespace bh {

constexpr uint32_t DEAL_SPL_WORDS = 256;   // what a block stages: [0..253] splitters | [254] the sentinel | [255] the validity word

// slots per bucket: twice what a frame that lists ALL n splats needs when its buckets are even (16 bytes of region per splat)
inline uint32_t deal_capacity(uint32_t n) { return n / 128u > 2048u ? (n + 127u) / 128u : 2048u; }

BH_DEV void deal_stage(const DealArgs& d, uint32_t* s_spl /*[DEAL_SPL_WORDS]; the caller's next barrier publishes it*/) {
    for (uint32_t i = threadIdx.x; i < DEAL_SPL_WORDS; i += blockDim.x) s_spl[i] = d.spl[i];
}

// number of splitters <= key, the rule of depth_digit (depth_sort.hip); a table without its sentinel still names a bucket
BH_DEV uint32_t deal_digit(uint32_t key, const uint32_t* s_spl) {
    uint32_t dg = 0;
#pragma unroll
    for (uint32_t step = 128u; step != 0u; step >>= 1) dg += s_spl[dg + step - 1u] <= key ? step : 0u;
    return dg < DEAL_BUCKETS ? dg : DEAL_BUCKETS - 1u;
}

// Two halves, so that a caller can put work between the atomic and the first use of what it returns: deal_take -> (bucket, slot)
// — bucket DEAL_BUCKETS: none, the table holds no quantiles —, deal_put stores there, or sets the overflow word when there is no such slot.
struct DealSlot { uint32_t bucket, slot; };
BH_DEV DealSlot deal_take(const DealArgs& d, const uint32_t* s_spl, uint32_t key, uint32_t tiles) {
    if (s_spl[255] == 0u) return DealSlot{DEAL_BUCKETS, 0u};   // (block-uniform) the host was wrong about the table
    const uint32_t dg = deal_digit(key, s_spl);
    const unsigned long long old = atomicAdd(&d.ctr[(size_t)dg * DEAL_LINE_U64], ((unsigned long long)tiles << 32) | 1ull);
    return DealSlot{dg, (uint32_t)old};
}
BH_DEV void deal_put(const DealArgs& d, DealSlot at, uint32_t key, uint32_t id) {
    // (255 * cap slots: below 2^32 for every n the fused sort takes; every writer of the overflow word stores the same value: a plain store)
    if (at.bucket < DEAL_BUCKETS && at.slot < d.cap) d.region[(size_t)at.bucket * d.cap + at.slot] = make_uint2(key, id);
    else d.ctr[DEAL_OVERFLOW_U64] = 1ull;
}

}  // namespace bh
