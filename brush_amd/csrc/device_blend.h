// device_blend.h — the arithmetic every blend kernel shares (K16 / K17 in rasterize.hip, the depth and normal maps' one blend
// skeleton in device_map_blend.h): one copy of exp_blend and of a pixel's alpha / transmittance step, so that what one kernel
// blends another one replays decision for decision.
#pragma once
#include "device_math.h"

namespace bh {

// exp(x) for the blend loops, x = -sigma <= 0 wherever the result is used (lanes that fail the
// sigma pre-test compute a value nobody reads).  Base-2 form chosen for gfx950 issue rates: nine
// full-rate VALU ops (fma, sub, fma, 5 fma, lshl_add) where the Cephes sequence of bh_expf
// takes 14 with three half-rate ones (rndne, cvt, ldexp): k = rint(x*log2e) through the 1.5*2^23
// magic add (fused into the product), 2^f from a degree-5 minimax polynomial on [-0.5, 0.5] (1.6e-7 max rel. error), and the
// exponent spliced in by adding k << 23 to the bit pattern.  The CPU checker used by the tests
// restates the same sequence, so images stay bit-identical to it.
BH_DEV float exp_blend(float x) {
    const float s = __builtin_fmaf(x, 1.44269504088896341f, 12582912.0f);
    const float nkf = 12582912.0f - s;                               // -rint(x log2e), exact (as a subtraction: both fmas keep
    const float f = __builtin_fmaf(x, 1.44269504088896341f, nkf);    //  their constant as a literal, no SGPR operand)
    float p = 1.3274633092805743e-3f;
    p = __builtin_fmaf(p, f, 9.671961888670921e-3f);
    p = __builtin_fmaf(p, f, 5.5506784468889236e-2f);
    p = __builtin_fmaf(p, f, 2.4022234976291656e-1f);
    p = __builtin_fmaf(p, f, 6.931470632553101e-1f);
    p = __builtin_fmaf(p, f, 1.0f);
    return u2f(f2u(p) + (f2u(s) << 23));
}

// alpha of a splat at a pixel: alpha0 * exp(-sigma) under the 0.999 clamp (rasterize.rs:139)
BH_DEV float blend_alpha(float alpha0, float sigma) { return __builtin_fminf(0.999f, alpha0 * exp_blend(-sigma)); }

// One (pixel, splat) step of the front-to-back fold, given the pixel's transmittance T and whether it passed the sigma
// pre-test: the 1/255 cut-off (hard, or the smooth weight), the effective alpha, the transmittance behind the splat and the
// saturation rule (next_t <= 1e-4: the pixel is done WITHOUT this splat, rasterize.rs:155-160).  Returns `ok` (the splat
// passes the cut-off); it contributes iff ok && !sat.
template <bool SMOOTH>
BH_DEV bool blend_step(float alpha, bool pre, float T, float& alpha_eff, float& next_t, bool& sat) {
    const float w_cut = SMOOTH ? alpha_cutoff_weight(alpha) : (alpha >= ALPHA_CUTOFF_MID ? 1.0f : 0.0f);
    const bool ok = pre && w_cut > 0.0f;  // pre already implies sigma >= 0
    alpha_eff = SMOOTH ? alpha * w_cut : alpha;
    next_t = T * (1.0f - alpha_eff);
    sat = next_t <= 1.0e-4f;
    return ok;
}

// Conservative sigma bound of a splat: alpha0 * exp(-sigma) can only reach the cut-off where sigma <= this (the wave-uniform
// quadrant skip of the blend loops tests it before the exp).
constexpr float SIGMA_CUT_MARGIN = 0.01f;  // >> the error of bh_logf/exp_blend (~1e-7)
template <bool SMOOTH>
BH_DEV float blend_sigma_cut(float alpha0) {
    const float thr = SMOOTH ? (ALPHA_CUTOFF_MID - 0.5f * ALPHA_CUTOFF_BAND) : ALPHA_CUTOFF_MID;
    return __builtin_fmaxf(bh_logf(alpha0 / thr) + SIGMA_CUT_MARGIN, 0.0f);
}

// Register butterfly: wave-wide sum of ten per-lane values in 28 VALU ops — v_permlane32_swap /
// v_permlane16_swap fold two registers into one per step ("transpose-reduce"), then a DPP rotate-add finishes inside each
// 16-lane row.  Afterwards every lane of row r of k[i] holds component comp(i, r): k0 -> g0 g2 g1 g3, k1 -> g4 g6 g5 g7,
// k2 -> g8 - g9 -.
BH_DEV float swap32_add(float a, float b) {
    const auto r = __builtin_amdgcn_permlane32_swap(f2u(a), f2u(b), false, false);
    return u2f(r[0]) + u2f(r[1]);
}
BH_DEV float swap16_add(float a, float b) {
    const auto r = __builtin_amdgcn_permlane16_swap(f2u(a), f2u(b), false, false);
    return u2f(r[0]) + u2f(r[1]);
}
template <int CTRL>
BH_DEV float dpp_rot_add(float x) {
    return x + u2f(__builtin_amdgcn_update_dpp(0u, f2u(x), CTRL, 0xF, 0xF, false));
}
BH_DEV float row_allreduce(float x) {
    x = dpp_rot_add<0x128>(x);  // row_ror:8
    x = dpp_rot_add<0x124>(x);  // row_ror:4
    x = dpp_rot_add<0x122>(x);  // row_ror:2
    x = dpp_rot_add<0x121>(x);  // row_ror:1
    return x;
}
// The butterfly's integer kin (lift.hip: four u32 sums per register; the same lanes end up with the same components), and the
// wave-wide unsigned maximum: the row's by four DPP rotates, the four rows' through scalar registers.
BH_DEV uint32_t swap32_add_u32(uint32_t a, uint32_t b) {
    const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    return r[0] + r[1];
}
BH_DEV uint32_t swap16_add_u32(uint32_t a, uint32_t b) {
    const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    return r[0] + r[1];
}
template <int CTRL>
BH_DEV uint32_t dpp_rot_u32(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0u, x, CTRL, 0xF, 0xF, false);
}
BH_DEV uint32_t row_allreduce_u32(uint32_t x) {
    x += dpp_rot_u32<0x128>(x);  // row_ror:8
    x += dpp_rot_u32<0x124>(x);  // row_ror:4
    x += dpp_rot_u32<0x122>(x);  // row_ror:2
    x += dpp_rot_u32<0x121>(x);  // row_ror:1
    return x;
}
BH_DEV uint32_t wave_max_u32(uint32_t x) {
    x = max(x, dpp_rot_u32<0x128>(x));
    x = max(x, dpp_rot_u32<0x124>(x));
    x = max(x, dpp_rot_u32<0x122>(x));
    x = max(x, dpp_rot_u32<0x121>(x));
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)x, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)x, 16);
    const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)x, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)x, 48);
    return max(max(r0, r1), max(r2, r3));
}
// The same three row sums, FOLDED into one register while they are reduced (seven DPP adds instead of twelve): a DPP add with a
// partial bank_mask writes only some 4-lane banks of its destination, so b's row_ror:8 sums go into banks 2-3 of a's, the
// merged row_ror:4 step is kept where it is right (row_ror:4 feeds bank n from bank n-1: banks 1 and 3), c's row_ror:4 sums take
// the two banks that step left stale (0 and 2), and the last two steps run inside the quads of the ONE register.  Afterwards
// row r holds, in every lane of the bank, bank 1: a's row sum, bank 3: b's, banks 0 and 2: c's — each the same 16 values in a
// pairwise tree of the same depth as row_allreduce's.
// The compiler does not fuse a masked update_dpp with the add, hence the assembly, and it pads no hazard inside it: a VALU write
// of a VGPR needs 2 wait states before a DPP op reads it (what the compiler's own recognizer enforces: GCNHazardRecognizer,
// DppVgprWaitStates).  The opening s_nop covers the adds in front; below, every DPP read has two instructions or one + s_nop 0,
// or s_nop 1, between it and the write of its source.  Needs all 64 lanes active (DPP reads return 0 from lanes that are not).
BH_DEV float row_allreduce3_folded(float a, float b, float c) {
    asm volatile(
        "s_nop 1\n\t"
        "v_add_f32_dpp %[a], %[a], %[a] row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %[c], %[c], %[c] row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %[a], %[b], %[b] row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %[a], %[a], %[a] row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %[a], %[c], %[c] row_ror:4 row_mask:0xf bank_mask:0x5\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %[a], %[a], %[a] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %[a], %[a], %[a] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
        : [a] "+v"(a), [c] "+v"(c)
        : [b] "v"(b));
    return a;
}

}  // namespace bh
