// optim.hip — AdamScaled step, refine statistics, visibility-gated mean noise.
//
// Reference: brush-train/src/adam_scaled.rs:75-147, stats.rs:40-50,
// train.rs:389-416.  The reference expresses these as a few dozen burn tensor ops
// (fused opportunistically by burn-fusion); here each is ONE pass over HBM:
// 28 B/element for Adam (p,g,m,v read; p,m,v written), the floor for the update.
#include <cstdlib>

#include "context.h"
#include "device_rng.h"

namespace bh {

constexpr int OPT_WG = 256;

struct AdamArgs {
    float beta1, beta2, f1, f2, bc1, bc2, eps, lr;
    uint32_t first;  // t == 1: initialise the moments instead of decaying them
};

BH_DEV bool same_bits(float a, float b) { return f2u(a) == f2u(b); }
BH_DEV bool same_bits4(const float4& a, const float4& b) {
    return ((f2u(a.x) ^ f2u(b.x)) | (f2u(a.y) ^ f2u(b.y)) | (f2u(a.z) ^ f2u(b.z)) | (f2u(a.w) ^ f2u(b.w))) == 0u;
}

// ---- The element arithmetic of AdamScaled (adam_scaled.rs:75-147), written once: the fused update kernel must leave the bits
// the stand-alone kernels leave, and both the oracle's.
// One step of the first moment (g: the gradient) / of the second (gsq: its square, or a row's mean of squares).  `old` comes by
// address because the first step must not read it: it may be the tensor's element, which may hold anything then.  The betas
// are read inside the arm that uses them (as every call site did when it spelled this out): the compiler keeps the branch.
BH_DEV float moment1_step(const AdamArgs& a, const float* old, float g) { return a.first ? g * a.f1 : *old * a.beta1 + g * a.f1; }
BH_DEV float moment2_step(const AdamArgs& a, const float* old, float gsq) { return a.first ? gsq * a.f2 : *old * a.beta2 + gsq * a.f2; }
// the parameter after the step: m1 / v are the moments of THIS step, `step` the element's learning rate
BH_DEV float adam_elem(float p, float m1, float v, const AdamArgs& a, float step) {
    const float m1c = m1 / a.bc1;
    const float m2c = v / a.bc2;
    const float upd = m1c / (__builtin_sqrtf(m2c) + a.eps);
    return p - upd * step;
}
// a row's second moment (adam_scaled.rs:99-104,152-165) from its gradients g[0..row_len): the mean of their squares, summed
// sequentially in index order (the oracle's order, so the result is bit-identical), then the recurrence
BH_DEV float row_moment2(const float* g, uint32_t row_len, const float* v_old, const AdamArgs& a) {
    float s = 0.0f;
    for (uint32_t c = 0; c < row_len; ++c) s += g[c] * g[c];
    return moment2_step(a, v_old, s / (float)row_len);
}
BH_DEV uint32_t row10(uint32_t e) { return (e * 52429u) >> 19; }   // e / 10, exact for e < 2560 (a block's transforms)

// full second moment: one thread per element
__global__ __launch_bounds__(OPT_WG) void adam_full_kernel(float* __restrict__ param, const float* __restrict__ grad,
                                                          float* __restrict__ m1, float* __restrict__ m2, uint64_t count,
                                                          uint32_t row_len, const float* __restrict__ col_scale, AdamArgs a, float gscale) {
    const uint64_t i = (uint64_t)blockIdx.x * OPT_WG + threadIdx.x;
    if (i >= count) return;
    const float g = grad[i] * gscale;   // (gscale 1: the gradient's own bits)
    const float mm1 = moment1_step(a, &m1[i], g);
    const float mm2 = moment2_step(a, &m2[i], g * g);
    m1[i] = mm1;
    m2[i] = mm2;
    const float step = col_scale ? col_scale[i % row_len] * a.lr : a.lr;
    param[i] = adam_elem(param[i], mm1, mm2, a, step);
}

// second moment reduced to one scalar per row (adam_scaled.rs:99-104,152-165).
// A block owns 256 consecutive rows: the gradient tile is staged through LDS with
// coalesced loads (row pitch row_len+1: conflict-free for the per-row pass), thread r
// forms row r's second moment (row_moment2), and the update pass runs element-wise,
// coalesced, reading the row's v back from LDS.  (One thread per row made every access a
// 4*row_len-byte stride: 4.3 ms at 1 M splats / SH degree 3; this layout moves the same
// bytes at HBM speed.)
constexpr int ADAM_ROWS = 256;

__global__ __launch_bounds__(OPT_WG) void adam_rowreduced_kernel(float* __restrict__ param, const float* __restrict__ grad,
                                                                float* __restrict__ m1, float* __restrict__ m2, uint64_t rows,
                                                                uint32_t row_len, const float* __restrict__ col_scale, AdamArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    float* s_g = s_dyn;                                   // [ADAM_ROWS][row_len + 1]
    float* s_v = s_dyn + ADAM_ROWS * (row_len + 1);       // [ADAM_ROWS]
    const uint64_t row0 = (uint64_t)blockIdx.x * ADAM_ROWS;
    const uint32_t nrows = (uint32_t)(rows - row0 < (uint64_t)ADAM_ROWS ? rows - row0 : (uint64_t)ADAM_ROWS);
    const uint32_t count = nrows * row_len;
    const uint64_t base = row0 * row_len;
    const float rcp_len = 1.0f / (float)row_len;
    const uint32_t pitch = row_len + 1;
    for (uint32_t e = threadIdx.x; e < count; e += OPT_WG) {
        const uint32_t r = (uint32_t)(((float)e + 0.5f) * rcp_len);  // e / row_len, exact for e < 2^16
        const uint32_t c = e - r * row_len;
        s_g[r * pitch + c] = grad[base + e];
    }
    __syncthreads();
    if (threadIdx.x < nrows) {
        const uint64_t r = row0 + threadIdx.x;
        const float v = row_moment2(s_g + threadIdx.x * pitch, row_len, &m2[r], a);
        m2[r] = v;
        s_v[threadIdx.x] = v;
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < count; e += OPT_WG) {
        const uint32_t r = (uint32_t)(((float)e + 0.5f) * rcp_len);
        const uint32_t c = e - r * row_len;
        const uint64_t i = base + e;
        const float gi = s_g[r * pitch + c];
        const float mm1 = moment1_step(a, &m1[i], gi);
        m1[i] = mm1;
        const float step = col_scale ? col_scale[c] * a.lr : a.lr;
        param[i] = adam_elem(param[i], mm1, s_v[r], a, step);
    }
}

// compiler-rt __powisf2: the lowering of Rust's f32::powi (adam_scaled.rs:131-138)
static float powi_f32(float a, int b) {
    const bool recip = b < 0;
    float r = 1.0f;
    while (true) {
        if (b & 1) r *= a;
        b /= 2;
        if (b == 0) break;
        a *= a;
    }
    return recip ? 1.0f / r : r;
}

// the constants of step t (1-based)
static AdamArgs make_adam_args(float beta1, float beta2, float eps, float lr, uint32_t t) {
    AdamArgs a;
    a.beta1 = beta1; a.beta2 = beta2;
    a.f1 = 1.0f - beta1; a.f2 = 1.0f - beta2;
    a.bc1 = 1.0f - powi_f32(beta1, (int)t);
    a.bc2 = 1.0f - powi_f32(beta2, (int)t);
    a.eps = eps; a.lr = lr;
    a.first = t == 1 ? 1u : 0u;
    return a;
}

// the most dynamic LDS a block may ask for on the ctx's device once the kernel has opted in (hipFuncAttributeMaxDynamicSharedMemorySize):
// the device attribute, read once per ctx; a runtime that does not report the opt-in limit leaves the plain per-block limit
static size_t max_dynamic_lds(bh_ctx* ctx) {
    if (ctx->lds_optin_max == 0) {
        int optin = 0, plain = 0;
        if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, ctx->device) != hipSuccess) { (void)hipGetLastError(); optin = 0; }
        if (hipDeviceGetAttribute(&plain, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device) != hipSuccess) { (void)hipGetLastError(); plain = 0; }
        const int best = optin > plain ? optin : plain;
        ctx->lds_optin_max = best > 0 ? (size_t)best : (size_t)64 * 1024;
    }
    return ctx->lds_optin_max;
}

int launch_adam(bh_ctx* ctx, float* param, const float* grad, float* m1, float* m2, uint64_t rows, uint32_t row_len,
                const float* col_scale, float lr, uint32_t t, bool reduce_m2, float beta1, float beta2, float eps, float gscale) {
    if (rows == 0 || row_len == 0) return 0;
    if (t == 0) return set_error(ctx, BH_ERR_INVALID_ARG, "adam: t is 1-based");
    if (reduce_m2 && gscale != 1.0f) return set_error(ctx, BH_ERR_UNSUPPORTED, "adam (reduced second moment): no gradient scale");
    const AdamArgs a = make_adam_args(beta1, beta2, eps, lr, t);
    if (reduce_m2) {
        // 256 rows of row_len + 1 floats and the rows' second moments in LDS: what fits is the device's word (the opt-in limit of
        // dynamic LDS per block, 160 KB on gfx950: row_len <= 158), refused here, in front of any launch
        if (row_len > 255) return set_error(ctx, BH_ERR_UNSUPPORTED, "adam (reduced second moment): row_len must be <= 255");
        const uint64_t nb = (rows + ADAM_ROWS - 1) / ADAM_ROWS;
        const size_t lds = ((size_t)ADAM_ROWS * (row_len + 1) + ADAM_ROWS) * sizeof(float);
        const size_t lds_max = max_dynamic_lds(ctx);
        if (lds > lds_max)
            return set_error(ctx, BH_ERR_UNSUPPORTED, "adam (reduced second moment): row_len " + std::to_string(row_len) + " needs " + std::to_string(lds) +
                                                          " bytes of LDS per block, the device allows " + std::to_string(lds_max));
        if (lds > 64 * 1024 && !ctx->adam_lds_raised) {  // above the default dynamic-LDS limit (row_len > 62): opt in once per ctx (the attribute is per device)
            BH_HIP(ctx, hipFuncSetAttribute((const void*)adam_rowreduced_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
            ctx->adam_lds_raised = true;
        }
        hipLaunchKernelGGL(adam_rowreduced_kernel, dim3((unsigned)nb), dim3(OPT_WG), lds, ctx->stream, param, grad, m1, m2, rows, row_len, col_scale, a);
        BH_LAUNCH_CHECK(ctx, "adam_rowreduced_kernel");
    } else {
        const uint64_t count = rows * row_len;
        const uint64_t nb = (count + OPT_WG - 1) / OPT_WG;
        hipLaunchKernelGGL(adam_full_kernel, dim3((unsigned)nb), dim3(OPT_WG), 0, ctx->stream, param, grad, m1, m2, count, row_len, col_scale, a, gscale);
        BH_LAUNCH_CHECK(ctx, "adam_full_kernel");
    }
    return 0;
}

// ---------------------------------------------------------------------------
// The train step's whole "after the backward" tail in ONE launch: RefineRecord::gather_stats
// (stats.rs:40-50) + the three AdamScaled updates (train.rs:300-381) with the data-parallel
// 1/K gradient scale folded in.  A block owns ROWS (64, 128 or 256) consecutive splats, so every
// tensor it touches is one contiguous run: transforms 10*ROWS floats, SH ROWS*3C floats (staged through
// LDS for the per-row second moment, as adam_rowreduced_kernel), opacity / statistics ROWS floats.  The
// element arithmetic is that of the stand-alone kernels above (bit-identical results); what
// goes away is five launches, the lr-table upload and the separate gradient-scale pass.
// ---------------------------------------------------------------------------
struct UpdateArgs {
    AdamArgs a;            // betas / bias corrections of step t (shared: the three params step together; a.lr is not read)
    float lr_sh, lr_opac;  // the transforms' rates are the per-column table tab_t (train.rs:328-350)
    float gscale;          // 1/world for data parallel over cameras, else 1
    uint32_t n, sh_len;    // splats, 3*C
    uint32_t vis_clamp;    // tile-partitioned frame: visible arrives summed over strips -> min(v, 1)
    uint32_t dormant_skip; // 0 = BH_UPDATE_NO_DORMANT (A/B, tests): dormant splats are fetched and updated like everyone else
    uint32_t masked;       // the gradient tensors were not zero-filled: row i holds a gradient iff the sign bit of refine_weight[i] is set (K18's mark), else it is 0
    uint32_t sparse_max;   // option update_sparse: a block with at most this many non-dormant rows takes the one-round-trip path (0 = no block does)
    float tab_t[10];       // lr_mean x3, lr_rotation x4, lr_scale x3
    float tab_sh[75];      // 1 for the DC coefficient, 1/lr_coeffs_sh_scale for the rest
    // visibility-gated noise on the means (train.rs:389-416) drawn on the device and added right behind the Adam update
    uint32_t noise_on, noise_step;
    float noise_scale, noise_clamp;
    uint64_t noise_seed;
};

// VEC: every tensor base is 16-byte aligned -> 128-bit loads / stores (a block's region starts at a multiple of
// 256 rows, so it is aligned whenever the tensor is; a float4 may straddle two rows, rows/columns are resolved per
// component).  The element arithmetic is identical either way.
// ROWS: splats per block (multiple of 4, <= OPT_WG) — fewer for long SH rows keeps more blocks resident per CU.
// SPARSE: the kernel has the second path for blocks with few non-dormant rows (launched when option update_sparse is not 0).
constexpr uint32_t UPDATE_SPARSE_DEFAULT = 64;   // non-dormant rows of a 256-row block at SH degree 0 up to which the sparse path runs
// s_mask[row] (only with u.masked): nobody wrote the row's gradient (it counts as 0) / K18 wrote it / the splat is dormant
constexpr float ROW_UNWRITTEN = 0.0f, ROW_WRITTEN = 1.0f, ROW_DORMANT = 2.0f;

template <bool VEC, int ROWS, bool SPARSE>
__global__ __launch_bounds__(OPT_WG) void train_update_kernel(
    float* __restrict__ transforms, float* __restrict__ m1_t, float* __restrict__ m2_t, const float* __restrict__ g_t,
    float* __restrict__ sh, float* __restrict__ m1_sh, float* __restrict__ m2_sh, const float* __restrict__ g_sh,
    float* __restrict__ opac, float* __restrict__ m1_o, float* __restrict__ m2_o, const float* __restrict__ g_o,
    float* __restrict__ refine_weight_norm, float* __restrict__ vis_weight, float* __restrict__ max_screen_size,
    const float* __restrict__ refine_weight, const float* __restrict__ visible, const float* __restrict__ screen_radius,
    UpdateArgs u) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    const AdamArgs& a = u.a;
    const uint64_t row0 = (uint64_t)blockIdx.x * (uint32_t)ROWS;
    const uint32_t nrows = (uint32_t)((uint64_t)u.n - row0 < (uint64_t)(uint32_t)ROWS ? (uint64_t)u.n - row0 : (uint64_t)(uint32_t)ROWS);
    const uint32_t row_len = u.sh_len, pitch = row_len + 1;
    float* s_g = s_dyn;                       // [rows][row_len + 1]
    float* s_v = s_dyn + (uint32_t)ROWS * pitch;      // [rows]
    float* s_mask = s_v + (uint32_t)ROWS;             // [rows] ROW_* (only with u.masked)
    float* s_nz = s_mask + (uint32_t)ROWS;            // [rows] != 0: some moment of the splat is non-zero after this step (only with u.masked)
    uint32_t* s_list = reinterpret_cast<uint32_t*>(s_nz + (uint32_t)ROWS);   // [rows] the block's non-dormant rows, ascending (sparse path)
    uint32_t* s_cnt = s_list + (uint32_t)ROWS;        // [4] non-dormant rows of each wave
    float* s_noise = reinterpret_cast<float*>(s_cnt + 4);   // [rows][3], only with noise_on
    // masked (block-uniform): the gradient tensors were not zero-filled — row r of them counts iff K18 marked the splat: the sign
    // bit of its (non-negative) refine weight, a vector that WAS cleared.
    // No barrier stands in front of what the block fetches: the SH staging below reads the marks it needs straight from global
    // memory (its gradients are wanted last, two round trips hide) and skips the rows nobody wrote — they would come from
    // cold HBM: +7 us at SH degree 3 when loaded and thrown away; the transforms' gradients are loaded unconditionally, their
    // marks come through LDS from the per-splat section (which reads the refine weight anyway), behind its barrier.  (Marks
    // staged through LDS up front, every gradient load predicated on them: +6 us at SH degree 0.)
    const bool masked = u.masked != 0u;
    // DORMANT splats (single-GPU step).  Nine tenths of a scene like the bench's never receive a gradient: every Adam moment of such
    // a splat is zero, its gradient row is not written this step either, the view did not reach it (no noise) — its update is
    // exactly nothing, and fetching its 26 moments, 14 parameters and 14 gradient slots (240 B at SH degree 0, 1.6 KB at degree 3)
    // only to find that out was most of this kernel's traffic.  The fact "all moments of this splat are zero" is kept where the
    // caller's tensors already have a spare bit: the SIGN of the row-reduced SH second moment m2_sh[i] — a sum of squares,
    // never negative — is set (the value is -0.0f) by the step that finds every new moment of the splat zero, and is cleared by the
    // first step that writes a real second moment (any gradient).  -0.0 equals +0.0 in every comparison and in the arithmetic that
    // reads it ((-0) b2 + g f2, sqrt, + eps), so the tensors stay what the reference's are; the mark travels with the caller's
    // data through refine's row gathers and through checkpoints, and a tensor that was zero-filled or loaded from elsewhere simply
    // carries no marks (every splat is processed until it is found dormant again).  A dormant splat costs its eleven per-splat
    // words (44 B: statistics, marks, opacity moments) and nothing else.  Not on the first step (the moment tensors may hold anything).
    const bool dorm_ok = masked && !a.first && u.dormant_skip != 0u;
    // SPARSE blocks (option update_sparse, kernel-uniform switch `sparse_on`).  With the skip, what a block still fetches behind its
    // per-splat section depends only on WHICH rows are not dormant, yet the sections below fetch it in three further dependent
    // round trips (SH gradients behind their marks, transforms, SH rows), and at SH degree 0 a block of the bench scene keeps a
    // few dozen rows.  A block with at most u.sparse_max such rows compacts them into an LDS list and issues every remaining load
    // — gradients, both moments and the parameters of the transforms, gradients, first moment and parameters of the SH rows — in ONE
    // round trip, element-wise over the listed rows (see `sparse` below).  While the switch is on nobody stages SH gradients up
    // front (a sparse block never wants the dormant rows'): a block over the threshold stages them behind the per-splat section's
    // barrier, marks from LDS — the same number of dependent trips as up-front staging behind global marks.  With the option at 0
    // the launcher picks the instantiations without the path (SPARSE = false): the one-path kernel, statement for statement.
    const bool sparse_on = SPARSE && dorm_ok && u.sparse_max != 0u;
    const uint32_t* mark_rows = reinterpret_cast<const uint32_t*>(refine_weight) + row0;
    const float rcp_len = 1.0f / (float)row_len;
    const uint32_t sh_count = nrows * row_len;
    const uint64_t sh_base = row0 * row_len;
    // ---- the sections below are separated by barriers (marks and noise travel through LDS, the SH rows need their second moment
    // first) and each fetches its own inputs: a block is a chain of dependent global round trips.  To keep it short the
    // per-splat section's eleven loads are unconditional and issued together, and the transforms loop has a fixed trip count
    // (unrolled: its loads leave together).
    constexpr int T_IT = (ROWS * 10 / 4 + OPT_WG - 1) / OPT_WG;          // float4s of the block's transforms per thread
    const uint32_t t_count = nrows * 10u, t_vec_end = VEC ? (t_count & ~3u) : 0u;
    const uint64_t t_base = row0 * 10u;
    const uint32_t s_vec_end = VEC ? (sh_count & ~3u) : 0u;
    // this thread's splat (clamped for the threads behind the block's last row)
    const uint64_t si = row0 + (threadIdx.x < nrows ? threadIdx.x : 0u);
    float in_rw = refine_weight[si], in_rn = refine_weight_norm[si], in_vis = visible[si], in_vw = vis_weight[si];
    float in_ms = max_screen_size[si], in_sr = screen_radius[si], in_go = g_o[si], in_m1o = m1_o[si], in_m2o = m2_o[si], in_op = opac[si];
    float in_m2sh = m2_sh[si];
    auto row_of = [&](uint32_t e) { return (uint32_t)(((float)e + 0.5f) * rcp_len); };   // e / row_len, exact for e < 2^16
    // ---- SH gradients -> LDS (coalesced), its loads queue behind the ones above
    auto stage_sh = [&](auto row_marked) {
        for (uint32_t e = threadIdx.x * 4u; e < s_vec_end; e += OPT_WG * 4u) {
            // (a float4 spans at most two rows: the first and the last component's)
            const uint32_t ra = row_of(e), rb = row_of(e + 3u);
            const bool wa = !masked || row_marked(ra), wb = !masked || row_marked(rb);
            float4 g4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (wa || wb) g4 = *reinterpret_cast<const float4*>(&g_sh[sh_base + e]);
            const float gv[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t ee = e + k;
                const uint32_t r = row_of(ee);
                s_g[r * pitch + (ee - r * row_len)] = (r == ra ? wa : wb) ? gv[k] * u.gscale : 0.0f;
            }
        }
        for (uint32_t e = s_vec_end + threadIdx.x; e < sh_count; e += OPT_WG) {
            const uint32_t r = row_of(e);
            s_g[r * pitch + (e - r * row_len)] = (!masked || row_marked(r)) ? g_sh[sh_base + e] * u.gscale : 0.0f;
        }
    };
    if (!sparse_on) stage_sh([&](uint32_t r) { return (mark_rows[r] >> 31) != 0u; });
    // ---- statistics + opacity: one splat per thread
    bool live = false;   // this thread's row exists and is not dormant
    if (threadIdx.x < nrows) {
        const uint64_t i = row0 + threadIdx.x;
        const float rw_raw = in_rw;
        const bool written = !masked || (f2u(rw_raw) >> 31) != 0u;
        // (the mark is checked against the two moments this thread has loaded anyway: a caller that restored or edited the opacity
        //  moments without rewriting m2_sh cannot make the step skip a splat whose moments are not zero)
        const bool dormant = dorm_ok && !written && f2u(in_m2sh) == 0x80000000u && in_vis == 0.0f && in_m1o == 0.0f && in_m2o == 0.0f;
        if (masked) s_mask[threadIdx.x] = written ? ROW_WRITTEN : (dormant ? ROW_DORMANT : ROW_UNWRITTEN);
        live = !dormant;
        // (masked: K18 stored the weight with the sign bit as the mark; an unmarked entry is the zero the forward left)
        {
            const float rn_old = in_rn, vw_old = in_vw, ms_old = in_ms;
            const float rn = __builtin_fmaxf(masked ? __builtin_fabsf(rw_raw) : rw_raw, rn_old);
            const float v = u.vis_clamp ? __builtin_fminf(in_vis, 1.0f) : in_vis;
            const float vw = vw_old + v;
            const float ms = __builtin_fmaxf(in_sr, ms_old);
            if (!same_bits(rn, rn_old)) refine_weight_norm[i] = rn;
            if (!same_bits(vw, vw_old)) vis_weight[i] = vw;
            if (!same_bits(ms, ms_old)) max_screen_size[i] = ms;
        }
        const float g = written ? in_go * u.gscale : 0.0f;
        const float m1_old = in_m1o, m2_old = in_m2o;
        const float mm1 = moment1_step(a, &m1_old, g);
        const float mm2 = moment2_step(a, &m2_old, g * g);
        const float p_old = in_op;
        const float p = adam_elem(p_old, mm1, mm2, a, u.lr_opac);
        // (stores of values that did not change are left out, here and below: see the note at the transforms)
        if (a.first || !same_bits(mm1, m1_old)) m1_o[i] = mm1;
        if (a.first || !same_bits(mm2, m2_old)) m2_o[i] = mm2;
        if (!same_bits(p, p_old)) opac[i] = p;
        if (masked) s_nz[threadIdx.x] = (mm1 != 0.0f || mm2 != 0.0f) ? 1.0f : 0.0f;
        if (u.noise_on) {   // the gate reads the UPDATED opacity (train.rs:389)
            const float w = mean_noise_gate(p, in_vis);
            float nz[3] = {0.0f, 0.0f, 0.0f};
            if (w != 0.0f) {
                const float wm = w * u.noise_scale;
                normal3(u.noise_seed, u.noise_step, (uint32_t)i, nz[0], nz[1], nz[2]);
#pragma unroll
                for (int k = 0; k < 3; ++k) nz[k] = clampf(nz[k] * wm, -u.noise_clamp, u.noise_clamp);
            }
            s_noise[threadIdx.x * 3u] = nz[0];
            s_noise[threadIdx.x * 3u + 1u] = nz[1];
            s_noise[threadIdx.x * 3u + 2u] = nz[2];
        }
    }
    // (sparse_on) this row's place among the block's non-dormant rows: within its wave here, the waves' counts through LDS
    uint32_t my_pos = 0;
    if (sparse_on) {
        const uint64_t bal = __ballot(live);
        my_pos = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if ((threadIdx.x & 63u) == 0u) s_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(bal);
    }
    if (u.noise_on || masked) __syncthreads();   // block-uniform
    // ---- one element of the transforms (full second moment, per-column lr) / of the SH rows (gradient and the row's second
    // moment from LDS: s_g / s_v, e = row * row_len + column in THEIR indexing) — shared by both paths below
    auto one_t = [&](float g_raw, bool written, float m1v, float m2v, float pv, uint32_t e, float& o_m1, float& o_m2, float& o_p) {
        const uint32_t r = row10(e);
        const uint32_t c = e - r * 10u;
        const float g = written ? g_raw * u.gscale : 0.0f;
        const float mm1 = moment1_step(a, &m1v, g);
        const float mm2 = moment2_step(a, &m2v, g * g);
        o_m1 = mm1;
        o_m2 = mm2;
        float p = adam_elem(pv, mm1, mm2, a, u.tab_t[c]);
        if (u.noise_on && c < 3u) p = p + s_noise[r * 3u + c];
        o_p = p;
    };
    auto one_sh = [&](float m1v, float pv, uint32_t e, float& o_m1, float& o_p) {
        const uint32_t r = row_of(e);
        const uint32_t c = e - r * row_len;
        const float mm1 = moment1_step(a, &m1v, s_g[r * pitch + c]);
        o_m1 = mm1;
        o_p = adam_elem(pv, mm1, s_v[r], a, u.tab_sh[c] * u.lr_sh);
    };
    uint32_t n_live = 0;
    bool sparse = false;   // block-uniform
    if (sparse_on) {
        uint32_t before = 0;
#pragma unroll
        for (uint32_t wv = 0; wv < (uint32_t)OPT_WG / 64u; ++wv) {
            const uint32_t cw = s_cnt[wv];
            n_live += cw;
            before += wv < (threadIdx.x >> 6) ? cw : 0u;
        }
        n_live = __builtin_amdgcn_readfirstlane(n_live);
        my_pos += before;
        sparse = n_live <= u.sparse_max;
    }
    if (sparse) {
        // ---- SPARSE: the listed rows in chunks of at most ch_rows (one chunk for nearly every block the threshold lets in).  Per
        // chunk: every load in one round trip, element-wise — lane x of trip k holds column x % 10 (x % row_len) of listed row
        // x / 10 (x / row_len), so a row's words stay on neighbouring lanes; a lane past the chunk's end loads its block's element 0
        // and drops it.  Gradients follow the mark: an unmarked row's lanes read the first-moment word they load anyway, not the
        // gradient tensor, and take 0.  The arithmetic is one_t / one_sh, the stores are left out per element where the dense path
        // decides per float4 (a store it adds there rewrites the bits that are in memory), so both paths leave the same tensors —
        // short of one corner: a dormant row's moment that holds -0.0 stays -0.0 here, where the dense path rewrites it as +0.0 if
        // the row shares a float4 with a non-dormant one (as it stays in the dense path when both of the float4's rows are dormant).
        constexpr uint32_t SP_T = 2, SP_S = 2;   // trips per chunk over the transforms / the SH rows
        const uint32_t ch_s = (SP_S * (uint32_t)OPT_WG) / row_len, ch_rows = ch_s < (SP_T * (uint32_t)OPT_WG) / 10u ? ch_s : (SP_T * (uint32_t)OPT_WG) / 10u;
        if (live) s_list[my_pos] = threadIdx.x;
        __syncthreads();
        for (uint32_t j0 = 0; j0 < n_live; j0 += ch_rows) {   // (block-uniform bounds)
            const uint32_t cn = n_live - j0 < ch_rows ? n_live - j0 : ch_rows;
            float tg[SP_T], tm1[SP_T], tm2[SP_T], tp[SP_T], sg[SP_S], sm1[SP_S], sp[SP_S];
            uint32_t te[SP_T], sr[SP_S];       // the element's index in the block's transforms / the SH element's row; ~0u: a lane past the end
            bool tw[SP_T], sw[SP_S];           // its row's gradient was written
#pragma unroll
            for (uint32_t k = 0; k < SP_T; ++k) {
                const uint32_t x = threadIdx.x + k * (uint32_t)OPT_WG;
                const uint32_t j = row10(x);
                const bool ok = x < cn * 10u;
                uint32_t r = 0u;
                if (ok) r = s_list[j0 + j];
                const uint32_t e = ok ? r * 10u + (x - j * 10u) : 0u;
                tw[k] = ok && s_mask[r] == ROW_WRITTEN;
                te[k] = ok ? e : ~0u;
                const uint64_t i = t_base + e;
                tg[k] = *(tw[k] ? &g_t[i] : &m1_t[i]);
                tm1[k] = m1_t[i];
                tm2[k] = m2_t[i];
                tp[k] = transforms[i];
            }
#pragma unroll
            for (uint32_t k = 0; k < SP_S; ++k) {
                const uint32_t x = threadIdx.x + k * (uint32_t)OPT_WG;
                const uint32_t j = row_of(x);            // x / row_len, exact for x < 2^16
                const bool ok = x < cn * row_len;
                uint32_t r = 0u;
                if (ok) r = s_list[j0 + j];
                const uint32_t e = ok ? r * row_len + (x - j * row_len) : 0u;
                sw[k] = ok && s_mask[r] == ROW_WRITTEN;
                sr[k] = ok ? r : ~0u;
                const uint64_t i = sh_base + e;
                sg[k] = *(sw[k] ? &g_sh[i] : &m1_sh[i]);
                sm1[k] = m1_sh[i];
                sp[k] = sh[i];
            }
            asm volatile("" ::: "memory");   // (compiler-only: every load above is issued in front of the first use below)
            // SH gradients, scaled, into s_g rows by position in the chunk: s_g[x / row_len][x % row_len] is element x of one_sh
#pragma unroll
            for (uint32_t k = 0; k < SP_S; ++k) {
                const uint32_t x = threadIdx.x + k * (uint32_t)OPT_WG;
                const uint32_t j = row_of(x);
                if (sr[k] != ~0u) s_g[j * pitch + (x - j * row_len)] = sw[k] ? sg[k] * u.gscale : 0.0f;
            }
#pragma unroll
            for (uint32_t k = 0; k < SP_T; ++k) {
                if (te[k] == ~0u) continue;
                const uint64_t i = t_base + te[k];
                float o1, o2, op;
                one_t(tg[k], tw[k], tm1[k], tm2[k], tp[k], te[k], o1, o2, op);
                if (o1 != 0.0f || o2 != 0.0f) s_nz[row10(te[k])] = 1.0f;
                if (!same_bits(o1, tm1[k])) m1_t[i] = o1;
                if (!same_bits(o2, tm2[k])) m2_t[i] = o2;
                if (!same_bits(op, tp[k])) transforms[i] = op;
            }
            __syncthreads();
            // the rows' second moment: the row's own thread (it holds the old value)
            if (live && my_pos >= j0 && my_pos - j0 < cn) {
                const float v = row_moment2(s_g + (my_pos - j0) * pitch, row_len, &in_m2sh, a);
                if (!same_bits(v, in_m2sh)) m2_sh[row0 + threadIdx.x] = v;
                s_v[my_pos - j0] = v;
                if (v != 0.0f) s_nz[threadIdx.x] = 1.0f;
            }
            __syncthreads();
#pragma unroll
            for (uint32_t k = 0; k < SP_S; ++k) {
                if (sr[k] == ~0u) continue;
                const uint32_t x = threadIdx.x + k * (uint32_t)OPT_WG;
                const uint64_t i = sh_base + sr[k] * row_len + (x - row_of(x) * row_len);
                float o1, op;
                one_sh(sm1[k], sp[k], x, o1, op);
                if (o1 != 0.0f) s_nz[sr[k]] = 1.0f;
                if (!same_bits(o1, sm1[k])) m1_sh[i] = o1;
                if (!same_bits(op, sp[k])) sh[i] = op;
            }
            if (j0 + ch_rows < n_live) __syncthreads();   // the next chunk overwrites s_g / s_v
        }
    } else {
        if (sparse_on) stage_sh([&](uint32_t r) { return s_mask[r] == ROW_WRITTEN; });
        // ---- transforms: full second moment, per-column lr
        {
#pragma unroll
            for (int k = 0; k < T_IT; ++k) {
                const uint32_t e = (threadIdx.x + (uint32_t)k * OPT_WG) * 4u;
                if (e >= t_vec_end) break;
                const uint64_t i = t_base + e;
                const uint32_t ra = row10(e), rb = row10(e + 3u);   // the float4's first and last row
                const float ka = masked ? s_mask[ra] : ROW_WRITTEN, kb = masked ? s_mask[rb] : ROW_WRITTEN;
                if (ka == ROW_DORMANT && kb == ROW_DORMANT) continue;   // both rows dormant: nothing to fetch, nothing moves
                const float4 g4 = *reinterpret_cast<const float4*>(&g_t[i]);
                float4 m14 = *reinterpret_cast<const float4*>(&m1_t[i]);
                float4 m24 = *reinterpret_cast<const float4*>(&m2_t[i]);
                float4 p4 = *reinterpret_cast<const float4*>(&transforms[i]);
                const bool wa = ka == ROW_WRITTEN, wb = kb == ROW_WRITTEN;
                const float4 m1_old = m14, m2_old = m24, p_old = p4;
                one_t(g4.x, wa, m14.x, m24.x, p4.x, e, m14.x, m24.x, p4.x);
                one_t(g4.y, row10(e + 1u) == ra ? wa : wb, m14.y, m24.y, p4.y, e + 1, m14.y, m24.y, p4.y);
                one_t(g4.z, row10(e + 2u) == ra ? wa : wb, m14.z, m24.z, p4.z, e + 2, m14.z, m24.z, p4.z);
                one_t(g4.w, wb, m14.w, m24.w, p4.w, e + 3, m14.w, m24.w, p4.w);
                if (masked) {   // which rows still carry a non-zero moment (the dormant mark is set from this at the end)
                    const uint32_t r1 = row10(e + 1u), r2 = row10(e + 2u);
                    if (m14.x != 0.0f || m24.x != 0.0f) s_nz[ra] = 1.0f;
                    if (m14.y != 0.0f || m24.y != 0.0f) s_nz[r1] = 1.0f;
                    if (m14.z != 0.0f || m24.z != 0.0f) s_nz[r2] = 1.0f;
                    if (m14.w != 0.0f || m24.w != 0.0f) s_nz[rb] = 1.0f;
                }
                // A store whose four values are bit for bit what was loaded is left out.  That is the case for every splat that has
                // never received a gradient (moments 0, gradient 0: the moments stay 0 and the parameter does not move) — nine tenths
                // of the bench scene, where most splats lie behind saturated tiles in every view; a scene whose splats all reach a
                // pixel now and then writes everything, as before.  The update is HBM-bound and 3 of its 7 streams are stores.
                if (a.first || !same_bits4(m14, m1_old)) *reinterpret_cast<float4*>(&m1_t[i]) = m14;
                if (a.first || !same_bits4(m24, m2_old)) *reinterpret_cast<float4*>(&m2_t[i]) = m24;
                if (!same_bits4(p4, p_old)) *reinterpret_cast<float4*>(&transforms[i]) = p4;
            }
            for (uint32_t e = t_vec_end + threadIdx.x; e < t_count; e += OPT_WG) {
                const uint64_t i = t_base + e;
                float o1, o2, op;
                const uint32_t r = row10(e);
                one_t(g_t[i], !masked || s_mask[r] == ROW_WRITTEN, m1_t[i], m2_t[i], transforms[i], e, o1, o2, op);
                m1_t[i] = o1;
                m2_t[i] = o2;
                transforms[i] = op;
                if (masked && (o1 != 0.0f || o2 != 0.0f)) s_nz[r] = 1.0f;
            }
        }
        // ---- SH: per-row second moment
        __syncthreads();
        if (threadIdx.x < nrows) {
            const float v = row_moment2(s_g + threadIdx.x * pitch, row_len, &in_m2sh, a);
            const bool is_dormant = masked && s_mask[threadIdx.x] == ROW_DORMANT;
            // (a dormant row keeps its -0.0: the recurrence would turn it into +0.0 and un-mark it every step)
            if (!is_dormant && (a.first || !same_bits(v, in_m2sh))) m2_sh[row0 + threadIdx.x] = v;
            s_v[threadIdx.x] = v;
            if (masked && v != 0.0f) s_nz[threadIdx.x] = 1.0f;
        }
        __syncthreads();
        {
            auto four = [&](float4 m14, float4 p4, uint32_t e) {
                const uint64_t i = sh_base + e;
                const float4 m1_old = m14, p_old = p4;
                one_sh(m14.x, p4.x, e, m14.x, p4.x);
                one_sh(m14.y, p4.y, e + 1, m14.y, p4.y);
                one_sh(m14.z, p4.z, e + 2, m14.z, p4.z);
                one_sh(m14.w, p4.w, e + 3, m14.w, p4.w);
                if (masked) {
                    if (m14.x != 0.0f) s_nz[row_of(e)] = 1.0f;
                    if (m14.y != 0.0f) s_nz[row_of(e + 1u)] = 1.0f;
                    if (m14.z != 0.0f) s_nz[row_of(e + 2u)] = 1.0f;
                    if (m14.w != 0.0f) s_nz[row_of(e + 3u)] = 1.0f;
                }
                if (a.first || !same_bits4(m14, m1_old)) *reinterpret_cast<float4*>(&m1_sh[i]) = m14;
                if (!same_bits4(p4, p_old)) *reinterpret_cast<float4*>(&sh[i]) = p4;
            };
            for (uint32_t e = threadIdx.x * 4u; e < s_vec_end; e += OPT_WG * 4u) {
                // (a float4 spans at most two rows for row_len >= 3: the first and the last component's)
                if (masked && s_mask[row_of(e)] == ROW_DORMANT && s_mask[row_of(e + 3u)] == ROW_DORMANT) continue;   // dormant rows: nothing to fetch
                four(*reinterpret_cast<const float4*>(&m1_sh[sh_base + e]), *reinterpret_cast<const float4*>(&sh[sh_base + e]), e);
            }
            for (uint32_t e = s_vec_end + threadIdx.x; e < sh_count; e += OPT_WG) {
                const uint64_t i = sh_base + e;
                float o1, op;
                one_sh(m1_sh[i], sh[i], e, o1, op);
                m1_sh[i] = o1;
                sh[i] = op;
                if (masked && o1 != 0.0f) s_nz[row_of(e)] = 1.0f;
            }
        }
    }
    // ---- a splat whose moments are ALL zero after this step is dormant from now on: the mark is the sign of its m2_sh (== -0.0f)
    if (masked) {   // block-uniform
        __syncthreads();
        if (threadIdx.x < nrows && s_mask[threadIdx.x] != ROW_DORMANT && s_nz[threadIdx.x] == 0.0f) m2_sh[row0 + threadIdx.x] = -0.0f;
    }
}

int launch_train_update(bh_ctx* ctx, const BhTrainState* st, const UpdateCall& c) {
    const uint32_t n = st->n, C = (st->sh_degree + 1) * (st->sh_degree + 1), t = c.t;
    if (n == 0) return 0;
    if (t == 0) return set_error(ctx, BH_ERR_INVALID_ARG, "adam: t is 1-based");
    const float *g_t = c.g_transforms, *g_sh = c.g_sh, *g_o = c.g_opac;
    const NoiseArgs* noise = c.noise;
    UpdateArgs u;
    u.a = make_adam_args(c.beta1, c.beta2, c.eps, 1.0f, t);   // (the kernel reads no a.lr)
    u.lr_sh = c.lr_sh; u.lr_opac = c.lr_opac; u.gscale = c.gscale;
    u.n = n; u.sh_len = 3 * C; u.vis_clamp = c.vis_clamp ? 1u : 0u;
    u.masked = c.masked_rows ? 1u : 0u;
    // Marks are trusted only on a state this context updated at the previous step (same tensors, consecutive step count): a state
    // seen for the first time, re-bound to other tensors (refine, a checkpoint restore) or with a step counter that jumped is
    // processed in full once — that step re-derives every mark from the moments it finds.
    const bool same_state = ctx->marks_m2_sh == st->m2_sh && ctx->marks_m1_t == st->m1_transforms && ctx->marks_n == n && ctx->marks_step + 1u == t;
    ctx->marks_m2_sh = st->m2_sh; ctx->marks_m1_t = st->m1_transforms; ctx->marks_n = n; ctx->marks_step = t;
    u.dormant_skip = (ctx->knob_no_dormant || !same_state) ? 0u : 1u;
    // option update_sparse (read here, at every launch).  Its default is measured at SH degree 0 only — 256-row blocks of three SH
    // words a row; longer rows keep the one-path kernel unless the option asks for the sparse path
    u.sparse_max = ctx->knob_update_sparse >= 0 ? (uint32_t)ctx->knob_update_sparse : (u.sh_len == 3u ? UPDATE_SPARSE_DEFAULT : 0u);
    u.noise_on = noise ? 1u : 0u;
    u.noise_step = noise ? noise->step : 0u;
    u.noise_scale = noise ? noise->scale : 0.0f;
    u.noise_clamp = noise ? noise->clamp_abs : 0.0f;
    u.noise_seed = noise ? noise->seed : 0ull;
    for (int i = 0; i < 10; ++i) u.tab_t[i] = c.tab_t[i];
    for (uint32_t k = 0; k < 75; ++k) u.tab_sh[k] = (k / 3 == 0) ? 1.0f : c.sh_rest_scale;
    // splats per block: ~13 KB of LDS-staged SH gradients keeps >= 8 blocks resident per CU (measured at 1 M splats:
    // SH degree 3: 0.368 ms @256, 0.300 @128, 0.290 @64, 0.327 @32; degree 0 is best at 256)
    uint32_t rows = u.sh_len <= 12 ? 256u : (u.sh_len <= 27 ? 128u : 64u);
    if (ctx->knob_update_rows) rows = ctx->knob_update_rows;  // developer knob BH_UPDATE_ROWS (read once at bh_create)
    const size_t lds = ((size_t)rows * (u.sh_len + 1) + 4 * rows + 4 + (noise ? 3 * rows : 0)) * sizeof(float);   // s_g, s_v, s_mask, s_nz, s_list, s_cnt, s_noise
    const unsigned nb = (unsigned)(((uint64_t)n + rows - 1) / rows);
    const void* vec_ptrs[] = {st->transforms, st->m1_transforms, st->m2_transforms, g_t, st->sh_coeffs, st->m1_sh, g_sh};
    bool vec = true;
    for (const void* q : vec_ptrs) vec = vec && ((uintptr_t)q & 15u) == 0;
#define BH_LAUNCH_UPDATE(V, R, P)                                                                                                       \
    hipLaunchKernelGGL((train_update_kernel<V, R, P>), dim3(nb), dim3(OPT_WG), lds, ctx->stream, st->transforms, st->m1_transforms,    \
                       st->m2_transforms, g_t, st->sh_coeffs, st->m1_sh, st->m2_sh, g_sh, st->raw_opacities, st->m1_opac, st->m2_opac, \
                       g_o, st->refine_weight_norm, st->vis_weight, st->max_screen_size, c.refine_weight, c.visible, c.screen_radius, u)
#define BH_LAUNCH_UPDATE_ROWS(R)                                                                        \
    case R:                                                                                             \
        if (vec) { if (sparse) BH_LAUNCH_UPDATE(true, R, true); else BH_LAUNCH_UPDATE(true, R, false); }    \
        else { if (sparse) BH_LAUNCH_UPDATE(false, R, true); else BH_LAUNCH_UPDATE(false, R, false); }      \
        break
    const bool sparse = u.sparse_max != 0u;   // 0: the instantiations without the second path
    if (rows != 64u && rows != 128u && rows != 256u) return set_error(ctx, BH_ERR_INVALID_ARG, "update_rows must be 64, 128 or 256");
    // 256-row blocks of SH degree 4 stage 85 KB: above the default dynamic-LDS limit, the instantiation opts in once per ctx
    // (the attribute is per device), and what the device cannot give is refused in front of the launch
    if (lds > 64 * 1024) {
        const size_t lds_max = max_dynamic_lds(ctx);
        if (lds > lds_max) return set_error(ctx, BH_ERR_INVALID_ARG, "update_rows " + std::to_string(rows) + " at this SH degree needs more LDS per block than the device allows");
        const uint32_t bit = 1u << ((vec ? 1u : 0u) | (sparse ? 2u : 0u) | (rows == 64u ? 0u : rows == 128u ? 4u : 8u));
        if (!(ctx->update_lds_raised & bit)) {
#define BH_RAISE_UPDATE(V, R, P) BH_HIP(ctx, hipFuncSetAttribute((const void*)train_update_kernel<V, R, P>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max))
#define BH_RAISE_UPDATE_ROWS(R)                                                                     \
    case R:                                                                                         \
        if (vec) { if (sparse) BH_RAISE_UPDATE(true, R, true); else BH_RAISE_UPDATE(true, R, false); }  \
        else { if (sparse) BH_RAISE_UPDATE(false, R, true); else BH_RAISE_UPDATE(false, R, false); }    \
        break
            switch (rows) {
                BH_RAISE_UPDATE_ROWS(64);
                BH_RAISE_UPDATE_ROWS(128);
                BH_RAISE_UPDATE_ROWS(256);
            }
#undef BH_RAISE_UPDATE_ROWS
#undef BH_RAISE_UPDATE
            ctx->update_lds_raised |= bit;
        }
    }
    switch (rows) {
        BH_LAUNCH_UPDATE_ROWS(64);
        BH_LAUNCH_UPDATE_ROWS(128);
        BH_LAUNCH_UPDATE_ROWS(256);
        default: return set_error(ctx, BH_ERR_INVALID_ARG, "update_rows must be 64, 128 or 256");
    }
#undef BH_LAUNCH_UPDATE_ROWS
#undef BH_LAUNCH_UPDATE
    BH_LAUNCH_CHECK(ctx, "train_update_kernel");
    return 0;
}

// stats.rs:40-50
__global__ __launch_bounds__(OPT_WG) void gather_stats_kernel(float* __restrict__ refine_weight_norm, float* __restrict__ vis_weight,
                                                             float* __restrict__ max_screen_size, const float* __restrict__ refine_weight,
                                                             const float* __restrict__ visible, const float* __restrict__ screen_radius,
                                                             uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * OPT_WG + threadIdx.x;
    if (i >= n) return;
    refine_weight_norm[i] = __builtin_fmaxf(refine_weight[i], refine_weight_norm[i]);
    vis_weight[i] = vis_weight[i] + visible[i];
    max_screen_size[i] = __builtin_fmaxf(screen_radius[i], max_screen_size[i]);
}

int launch_gather_stats(bh_ctx* ctx, float* refine_weight_norm, float* vis_weight, float* max_screen_size,
                        const float* refine_weight, const float* visible, const float* screen_radius, uint64_t n) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(gather_stats_kernel, dim3((unsigned)((n + OPT_WG - 1) / OPT_WG)), dim3(OPT_WG), 0, ctx->stream, refine_weight_norm, vis_weight, max_screen_size, refine_weight, visible, screen_radius, n);
    BH_LAUNCH_CHECK(ctx, "gather_stats_kernel");
    return 0;
}

// train.rs:389-416: means += clamp(sample * (1 - sigmoid(raw_opac))^150 * visible * scale, +-clamp_abs)
// samples == NULL: the N(0,1) samples are drawn on the spot (device_rng.h, keyed by seed / step / splat).
__global__ __launch_bounds__(OPT_WG) void mean_noise_kernel(float* __restrict__ transforms, const float* __restrict__ raw_opac,
                                                           const float* __restrict__ visible, const float* __restrict__ samples,
                                                           uint64_t n, float noise_scale, float clamp_abs, uint64_t seed, uint32_t step) {
    const uint64_t i = (uint64_t)blockIdx.x * OPT_WG + threadIdx.x;
    if (i >= n) return;
    const float w = mean_noise_gate(raw_opac[i], visible[i]);
    const float wm = w * noise_scale;
    float smp[3];
    if (samples) {
        smp[0] = samples[i * 3]; smp[1] = samples[i * 3 + 1]; smp[2] = samples[i * 3 + 2];
    } else {
        if (w == 0.0f) return;   // sample * 0 = 0 for every finite sample: the means do not move
        normal3(seed, step, (uint32_t)i, smp[0], smp[1], smp[2]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float nz = clampf(smp[k] * wm, -clamp_abs, clamp_abs);
        transforms[i * 10 + k] = transforms[i * 10 + k] + nz;
    }
}

int launch_mean_noise(bh_ctx* ctx, float* transforms, const float* raw_opac, const float* visible, const float* samples,
                      uint64_t n, float noise_scale, float clamp_abs, uint64_t seed, uint32_t step) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(mean_noise_kernel, dim3((unsigned)((n + OPT_WG - 1) / OPT_WG)), dim3(OPT_WG), 0, ctx->stream, transforms, raw_opac, visible, samples, n, noise_scale, clamp_abs, seed, step);
    BH_LAUNCH_CHECK(ctx, "mean_noise_kernel");
    return 0;
}

// the raw N(0,1) samples a step would draw: out [n,3] (tests; callers that want the reference's `samples` tensor)
__global__ __launch_bounds__(OPT_WG) void normal_samples_kernel(float* __restrict__ out, uint64_t n, uint64_t seed, uint32_t step) {
    const uint64_t i = (uint64_t)blockIdx.x * OPT_WG + threadIdx.x;
    if (i >= n) return;
    float a, b, c;
    normal3(seed, step, (uint32_t)i, a, b, c);
    out[i * 3] = a; out[i * 3 + 1] = b; out[i * 3 + 2] = c;
}

int launch_normal_samples(bh_ctx* ctx, float* out, uint64_t n, uint64_t seed, uint32_t step) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(normal_samples_kernel, dim3((unsigned)((n + OPT_WG - 1) / OPT_WG)), dim3(OPT_WG), 0, ctx->stream, out, n, seed, step);
    BH_LAUNCH_CHECK(ctx, "normal_samples_kernel");
    return 0;
}

}  // namespace bh
