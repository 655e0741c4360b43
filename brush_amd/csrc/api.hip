// api.hip — the extern "C" surface of libbrush_hip.so (include/brush_hip.h):
// context / arena / error plumbing and the host-side orchestration of the
// forward pipeline (render.rs:37-314) and the backward (bwd/render_bwd.rs:21-171).
// (SplatTrainer::step, brush-train/src/train.rs:176-429, is train.hip.)
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <new>

#include "../../include/brush_hip_intrinsics.h"
#include "context.h"
#include "depth_deal.h"
#include "device_rng.h"
#include "param_table.h"

namespace bh {

// grid-stride clear of two float4 spans in one launch
__global__ __launch_bounds__(256) void zero_two_kernel(float4* __restrict__ a, size_t na, float4* __restrict__ b, size_t nb) {
    const size_t stride = (size_t)gridDim.x * 256;
    const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < na + nb; i += stride) {
        if (i < na) a[i] = z;
        else b[i - na] = z;
    }
}

int set_error(bh_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->last_error = msg;
    return code;
}

int check_hip(bh_ctx* ctx, hipError_t e, const char* what) {
    if (e == hipSuccess) return 0;
    std::string m = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return set_error(ctx, e == hipErrorOutOfMemory ? BH_ERR_OOM : BH_ERR_HIP, m);
}

// Host wait for a tag word a kernel stores into pinned host memory (instead of an event behind the kernel: the barrier packet an
// event costs is ~6 us of bubble in front of the NEXT kernel).  Spins; every 16 k polls it asks the stream whether it is still
// alive, so a device fault ends in an error instead of a hang.
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    __asm__ __volatile__("yield");
#endif
}
int wait_host_tag(bh_ctx* ctx, const volatile uint32_t* word, uint32_t want, const char* what) {
    // Spins for at most ~2 ms (a healthy step delivers its tag within tens of microseconds), then stops burning the core: an event
    // behind everything queued so far and a blocking wait on it — the tag's kernel is in front of that event, so afterwards the tag
    // is there, or its kernel was never launched (an error, not a hang).
    for (uint64_t it = 1; it < (1ull << 21); ++it) {
        if (*word == want) return 0;
        if ((it & 0x3FFFull) == 0ull) {
            const hipError_t q = hipStreamQuery(ctx->stream);
            if (q == hipSuccess) break;   // everything queued has run: the tag must be there (checked below)
            if (q != hipErrorNotReady) return check_hip(ctx, q, what);
        }
        cpu_relax();
    }
    if (*word == want) return 0;
    BH_HIP(ctx, hipEventRecord(ctx->readback_ev, ctx->stream));
    BH_HIP(ctx, hipEventSynchronize(ctx->readback_ev));
    if (*word == want) return 0;
    return set_error(ctx, BH_ERR_STATE, std::string(what) + ": the kernel that signals the host never stored its tag");
}

void* ensure(bh_ctx* ctx, Slot s, size_t bytes) {
    Buffer& b = ctx->slots[s];
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return b.ptr;
    // growing: wait for queued work that may still read the old block
    if (b.ptr) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(b.ptr);
        b.ptr = nullptr;
        b.cap = 0;
    }
    // a block handed back by bh_render_release (the smallest one that fits, at most 2x too large)
    {
        int best = -1;
        for (size_t i = 0; i < ctx->pool.size(); ++i)
            if (ctx->pool[i].cap >= bytes && ctx->pool[i].cap <= 2 * bytes + 4096 && (best < 0 || ctx->pool[i].cap < ctx->pool[(size_t)best].cap)) best = (int)i;
        if (best >= 0) {
            b = ctx->pool[(size_t)best];
            ctx->pool.erase(ctx->pool.begin() + best);
            return b.ptr;
        }
    }
    size_t cap = bytes + bytes / 4;  // head-room so slowly growing scenes do not realloc every step
    cap = (cap + 255) & ~(size_t)255;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, cap);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        cap = (bytes + 255) & ~(size_t)255;
        e = hipMalloc(&p, cap);
    }
    if (e != hipSuccess) {
        char msg[160];
        snprintf(msg, sizeof msg, "hipMalloc(%zu bytes) for scratch slot %d failed: %s", cap, (int)s, hipGetErrorString(e));
        (void)hipGetLastError();
        set_error(ctx, BH_ERR_OOM, msg);
        return nullptr;
    }
    b.ptr = p;
    b.cap = cap;
    return p;
}

ViewUniforms make_uniforms(const BhCamera& c) {
    ViewUniforms u;
    for (int i = 0; i < 12; ++i) u.vm[i] = c.vm[i];
    u.fx = c.fx; u.fy = c.fy; u.cx = c.cx; u.cy = c.cy;
    u.lim_pos_x = c.lim_pos_x; u.lim_pos_y = c.lim_pos_y; u.lim_neg_x = c.lim_neg_x; u.lim_neg_y = c.lim_neg_y;
    u.cam_x = c.cam_pos[0]; u.cam_y = c.cam_pos[1]; u.cam_z = c.cam_pos[2];
    u.img_w = c.img_w; u.img_h = c.img_h;
    u.tile_bw = (c.img_w + TILE_WIDTH - 1) / TILE_WIDTH;  // render.rs:30-35
    u.tile_bh = (c.img_h + TILE_WIDTH - 1) / TILE_WIDTH;
    const bool whole = c.tile_row_begin == 0 && c.tile_row_end == 0;
    u.tile_y0 = whole ? 0u : c.tile_row_begin;
    u.tile_y1 = whole ? u.tile_bh : c.tile_row_end;
    u.model = c.model;
    for (int i = 0; i < 8; ++i) u.dist[i] = c.dist[i];
    u.half_fov = c.half_max_render_fov;
    return u;
}

// ---- profiling -----------------------------------------------------------------
static int prof_index(Profiler& p, const char* name) {
    for (int i = 0; i < p.count; ++i)
        if (p.names[i] == name || std::strcmp(p.names[i], name) == 0) return i;
    if (p.count >= MAX_PROF) return -1;
    p.names[p.count] = name;
    p.ms[p.count] = 0.0f;
    p.calls[p.count] = 0;
    return p.count++;
}
static hipEvent_t prof_event(Profiler& p) {
    if (!p.pool.empty()) {
        hipEvent_t e = p.pool.back();
        p.pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
static void prof_resolve(bh_ctx* ctx) {
    Profiler& p = ctx->prof;
    for (auto& pe : p.pending) {
        (void)hipEventSynchronize(pe.b);
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, pe.a, pe.b) == hipSuccess && pe.idx >= 0) {
            p.ms[pe.idx] += ms;
            p.calls[pe.idx] += 1;
        }
        p.pool.push_back(pe.a);
        p.pool.push_back(pe.b);
    }
    p.pending.clear();
}

ProfScope::ProfScope(bh_ctx* c, const char* name, bool dominant) : ctx(c) {
    if (c->prof.level == 0 || (c->prof.level == 2 && !dominant)) return;
    idx = prof_index(c->prof, name);
    a = prof_event(c->prof);
    b = prof_event(c->prof);
    if (c->prof.level == 2) {   // handed to the kernel launch inside the scope (Profiler::ext_a)
        c->prof.ext_a = a;
        c->prof.ext_b = b;
        return;
    }
    (void)hipEventRecord(a, c->stream);
}
ProfScope::~ProfScope() {
    if (!a) return;
    if (ctx->prof.level == 2) {
        const bool used = ctx->prof.ext_a == nullptr;   // the launch took the events
        ctx->prof.ext_a = ctx->prof.ext_b = nullptr;
        if (!used) {   // nothing was launched inside the scope
            ctx->prof.pool.push_back(a);
            ctx->prof.pool.push_back(b);
            return;
        }
    } else {
        (void)hipEventRecord(b, ctx->stream);
    }
    ctx->prof.pending.push_back({idx, a, b});
}


}  // namespace bh

using namespace bh;

extern "C" {

const char* bh_version(void) { return "brush_hip 0.1 (gfx950)"; }

uint32_t bh_abi_version(void) { return BH_ABI_VERSION; }

uint32_t bh_struct_size(uint32_t which) {
    switch (which) {
        case BH_STRUCT_CAMERA: return (uint32_t)sizeof(BhCamera);
        case BH_STRUCT_RENDER_OUT: return (uint32_t)sizeof(BhRenderOut);
        case BH_STRUCT_LOSS_CONFIG: return (uint32_t)sizeof(BhLossConfig);
        case BH_STRUCT_TRAIN_CONFIG: return (uint32_t)sizeof(BhTrainConfig);
        case BH_STRUCT_TRAIN_STATE: return (uint32_t)sizeof(BhTrainState);
        case BH_STRUCT_TRAIN_BATCH: return (uint32_t)sizeof(BhTrainBatch);
        case BH_STRUCT_TRAIN_STATS: return (uint32_t)sizeof(BhTrainStats);
        case BH_STRUCT_REFINE_CONFIG: return (uint32_t)sizeof(BhRefineConfig);
        case BH_STRUCT_REFINE_STATS: return (uint32_t)sizeof(BhRefineStats);
        case BH_STRUCT_PLY_INFO: return (uint32_t)sizeof(BhPlyInfo);
        default: return 0u;
    }
}

bh_ctx* bh_create(int device, void* stream, int own_stream) {
    bh_ctx* ctx = new (std::nothrow) bh_ctx();
    if (!ctx) return nullptr;
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess) {
        (void)hipGetLastError();
        delete ctx;
        return nullptr;
    }
    if (!own_stream) {
        ctx->stream = (hipStream_t)stream;
        ctx->owns_stream = false;
    } else {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
            (void)hipGetLastError();
            delete ctx;
            return nullptr;
        }
        ctx->owns_stream = true;
    }
    if (hipHostMalloc((void**)&ctx->host_counters, bh::HOST_COUNTERS_BYTES, hipHostMallocCoherent)   /* (polled by the host while kernels store into it: never the non-coherent flavour HIP_HOST_COHERENT=0 would make of the default) */ != hipSuccess) {
        (void)hipGetLastError();
        if (ctx->owns_stream) (void)hipStreamDestroy(ctx->stream);
        delete ctx;
        return nullptr;
    }
    std::memset(ctx->host_counters, 0, bh::HOST_COUNTERS_BYTES);
    // No environment variable configures the shipping library: every tuning / A-B knob is a documented bh_set_option key.
#ifdef BH_TEST_HOOKS   // libbrush_hip_testhooks.so only (csrc/Makefile): the shipping library neither reads these nor exports the hook below
    ctx->knob_break_allreduce = getenv("BH_BREAK_ALLREDUCE") != nullptr;
    if (ctx->knob_break_allreduce)   // (bench.py's exchange self-check must catch it): never silent
        fprintf(stderr, "brush_hip: BH_BREAK_ALLREDUCE is set - every all-reduce of this context's communicator is deliberately CORRUPTED (test hook)\n");
    if (const char* e = getenv("BH_TEST_FAIL_LOSS_AT")) {   // (tests/test_gpu_sliced.py): the k-th train step on this ctx fails between its forward and its loss
        ctx->knob_fail_loss_at = (uint32_t)atoi(e);
        if (ctx->knob_fail_loss_at) fprintf(stderr, "brush_hip: BH_TEST_FAIL_LOSS_AT=%u - that train step of this context will FAIL on purpose (test hook)\n", ctx->knob_fail_loss_at);
    }
#endif
    if (hipEventCreateWithFlags(&ctx->readback_ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->gate_ev, hipEventDisableTiming) != hipSuccess) {
        if (ctx->readback_ev) (void)hipEventDestroy(ctx->readback_ev);
        (void)hipGetLastError();
        (void)hipHostFree(ctx->host_counters);
        if (ctx->owns_stream) (void)hipStreamDestroy(ctx->stream);
        delete ctx;
        return nullptr;
    }
    return ctx;
}

void bh_destroy(bh_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    prof_resolve(ctx);
    for (hipEvent_t e : ctx->prof.pool) (void)hipEventDestroy(e);
    for (auto& b : ctx->slots)
        if (b.ptr) (void)hipFree(b.ptr);
    for (auto& kv : ctx->views)
        if (kv.second.zcut) (void)hipFree(kv.second.zcut);
    for (auto& rt : ctx->retained)
        for (auto& b : rt.blocks)
            if (b.ptr) (void)hipFree(b.ptr);
    for (auto& b : ctx->pool)
        if (b.ptr) (void)hipFree(b.ptr);
    if (ctx->host_counters) (void)hipHostFree(ctx->host_counters);
    if (ctx->dsort_spl) (void)hipFree(ctx->dsort_spl);
    if (ctx->deal_ctr) (void)hipFree(ctx->deal_ctr);
    if (ctx->sort_groups) (void)hipFree(ctx->sort_groups);
    if (ctx->readback_ev) (void)hipEventDestroy(ctx->readback_ev);
    if (ctx->gate_ev) (void)hipEventDestroy(ctx->gate_ev);
    if (ctx->image_tab_host) (void)hipHostFree(ctx->image_tab_host);
    if (ctx->image_tab_ev) (void)hipEventDestroy(ctx->image_tab_ev);
    bh::param_tables_free_all(ctx);
    if (ctx->comm) (void)bh_comm_destroy(ctx);
    if (ctx->owns_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* bh_last_error(bh_ctx* ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }

int bh_sync(bh_ctx* ctx) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (ctx->far_job.pending) {   // (a deferred decision may queue kernels: on the ctx's device)
        BH_HIP(ctx, hipSetDevice(ctx->device));
        BH_TRY(finish_far_slice(ctx, nullptr));
    }
    BH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    deliver_pending_loss(ctx);  // the last train step's loss, staged through pinned memory
    return 0;
}

int bh_profile_enable(bh_ctx* ctx, int on) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    ctx->prof.level = on < 0 ? 0 : (on > 2 ? 1 : on);
    return 0;
}

int bh_profile_fetch(bh_ctx* ctx, const char** names, float* ms, uint32_t* calls, int cap) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    prof_resolve(ctx);
    Profiler& p = ctx->prof;
    const int n = p.count < cap ? p.count : cap;
    for (int i = 0; i < n; ++i) {
        names[i] = p.names[i];
        ms[i] = p.ms[i];
        calls[i] = p.calls[i];
    }
    p.count = 0;
    return n;
}

// ---- options ---------------------------------------------------------------------
// One documented setter for everything earlier revisions read from BH_* environment variables at bh_create (include/brush_hip.h
// lists the keys).  Options select between paths that give the SAME results (A/B measurements, tests of the alternative paths);
// they are host fields read when the next call is queued.
namespace {
bool parse_u32(const char* v, uint32_t lo, uint32_t hi, uint32_t* out) {
    if (!v || !*v) return false;
    char* end = nullptr;
    const unsigned long long x = strtoull(v, &end, 10);
    if (*end != '\0' || x < lo || x > hi) return false;
    *out = (uint32_t)x;
    return true;
}
bool parse_flag(const char* v, bool* out) {
    uint32_t x = 0;
    if (!parse_u32(v, 0, 1, &x)) return false;
    *out = x != 0;
    return true;
}
// One row per key: bh_option_name / bh_option_help list it, bh_set_option finds it and calls apply, which parses the value and
// stores it (false, and nothing stored: a bad value).  The row index is public (bh_option_name(i)): new keys go at the end.
struct Option { const char* name; const char* help; bool (*apply)(bh_ctx* c, const char* v); };
const Option kOptions[] = {
    {"cut_min_pairs", "u32: a view whose last frame had fewer pairs keeps complete lists (= bh_set_list_cut_threshold)",
     [](bh_ctx* c, const char* v) { return parse_u32(v, 0, 0xFFFFFFFFu, &c->cut_min_pairs); }},
    {"cut_margin_pct", "0..10000: base margin behind a tile's last useful splat, % of its depth rank (default 150)",
     [](bh_ctx* c, const char* v) { return parse_u32(v, 0, 10000, &c->knob_cut_margin_pct); }},
    {"cut_margin_fixed", "0|1: the margin is cut_margin_pct for every frame instead of adaptive",
     [](bh_ctx* c, const char* v) { return parse_flag(v, &c->knob_fixed_margin); }},
    {"cut_ctrl", "up:down:floor:gap_exp — the margin controller's constants (default 1.5:0.998:0.5:0.3333)", [](bh_ctx* c, const char* v) {
        float a = 0, b = 0, d = 0, e = 0;
        if (sscanf(v, "%f:%f:%f:%f", &a, &b, &d, &e) != 4 || !(a >= 1.0f && b > 0.0f && b <= 1.0f && d > 0.0f && e >= 0.0f && e <= 1.0f)) return false;
        c->ctrl_up = a; c->ctrl_down = b; c->ctrl_floor = d; c->ctrl_gap_exp = e;
        return true;
    }},
    {"cut_sort_all", "0|1: with per-tile cuts, still depth-sort every visible splat",
     [](bh_ctx* c, const char* v) { return parse_flag(v, &c->knob_cut_sort_all); }},
    {"auto_exact_share", "0..1: a view whose last cut frame listed more than this share of its pairs renders complete lists (default 0.9; 0 = never)", [](bh_ctx* c, const char* v) {
        char* end = nullptr;
        const float x = strtof(v, &end);
        if (end == v || *end != '\0' || !(x >= 0.0f && x <= 1.0f)) return false;
        c->auto_exact_share = x;
        return true;
    }},
    {"no_view_hash", "0|1: frames without a view id share ONE table instead of being keyed by their camera",
     [](bh_ctx* c, const char* v) { return parse_flag(v, &c->knob_no_view_hash); }},
    {"k16_order", "0 index order | 1 by the view's last per-tile work | 2 dealt: the forward blend's tile order",
     [](bh_ctx* c, const char* v) { return parse_u32(v, 0, 2, &c->knob_k16_order); }},
    {"band_mode", "0|1: XCD bands of the blend kernels — contiguous eighths of the tile range, or dealt in chunks of 8 adjacent tiles (default 1)",
     [](bh_ctx* c, const char* v) { return parse_u32(v, 0, 1, &c->knob_band_mode); }},
    {"k16_waves", "0..8: forward blend: resident one-wave tiles per SIMD (0 = 8 = all resident at once; fewer: the lighter tiles are dispatched as the heavier ones finish)",
     [](bh_ctx* c, const char* v) { return parse_u32(v, 0, 8, &c->knob_k16_waves); }},
    {"k16_split", "0..1000: forward blend: a tile whose forecast work is at least max(256, k16_split / 100 x its band's mean) is blended by four quadrant waves (default 250; 0: no tile is split)",
     [](bh_ctx* c, const char* v) { return parse_u32(v, 0, 1000, &c->knob_k16_split); }},
    {"k16_split_of_max", "0..100: ... and at least this many percent of its band's heaviest tile (default 45)",
     [](bh_ctx* c, const char* v) { return parse_u32(v, 0, 100, &c->knob_k16_split_of_max); }},
    {"k16_split_min", "1..1023: a tile below this many blended splats (forecast) is never split (default 256)",
     [](bh_ctx* c, const char* v) { return parse_u32(v, 1, 1023, &c->knob_k16_split_min); }},
    {"k5_exact_spw", "16|32|64: splats per wave of the list builder for complete lists",
     [](bh_ctx* c, const char* v) { uint32_t u = 0; if (!parse_u32(v, 16, 64, &u) || !(u == 16 || u == 32 || u == 64)) return false; c->knob_k5_exact_spw = u; return true; }},
    {"bwd_jobs", "0|1: the blend backward works on checkpointed 128-entry segments of the tiles' lists (default 1) or on whole tiles",
     [](bh_ctx* c, const char* v) { return parse_flag(v, &c->knob_bwd_jobs); }},
    {"bwd_wide_rows", "0|1: the blend backward addresses the gradient accumulator in 64 bits, as it does by itself from 2^32 bytes of accumulator on (default 0)",
     [](bh_ctx* c, const char* v) { return parse_flag(v, &c->knob_bwd_wide_rows); }},
    {"no_lpt", "0|1: the blend backward takes its tiles in index order",
     [](bh_ctx* c, const char* v) { return parse_flag(v, &c->knob_no_lpt); }},
    {"lpt_classes", "log|linear: work classes of the backward's longest-first tile order — two per octave of blended splats, or 1/64 of the mean list length wide",
     [](bh_ctx* c, const char* v) { const std::string w(v); if (w == "log") { c->knob_lpt_linear = false; return true; } if (w == "linear") { c->knob_lpt_linear = true; return true; } return false; }},
    {"generic_depth_sort", "0|1: depth order by the generic radix sort + scan instead of the fused split sort",
     [](bh_ctx* c, const char* v) { return parse_flag(v, &c->knob_generic_depth_sort); }},
    {"dsort_splitters", "0|1: the fused depth sort splits at the 254 depth quantiles of the view's previous frame (default 1) or always linearly over the frame's key range",
     [](bh_ctx* c, const char* v) { return parse_flag(v, &c->knob_dsort_splitters); }},
    {"dsort_deal", "0|1: K1 deals the listed splats straight into the depth sort's buckets when the view's splitter table holds quantiles (default 1) or the histogram and split launches always run",
     [](bh_ctx* c, const char* v) { return parse_flag(v, &c->knob_dsort_deal); }},
    {"tile_sort", "auto|bucket|lsd: the forward's tile sort (auto: bucket sort unless the view's pairs are concentrated in few tiles)",
     [](bh_ctx* c, const char* v) { const std::string w(v); if (w == "auto") { c->knob_tile_sort = 0; return true; } if (w == "bucket") { c->knob_tile_sort = 1; return true; } if (w == "lsd") { c->knob_tile_sort = 2; return true; } return false; }},
    {"spec_k5", "0|1: queue the list builder before the host has read the frame's counts (default 1; 0: behind the count readback)",
     [](bh_ctx* c, const char* v) { return parse_flag(v, &c->knob_spec_k5); }},
    {"event_waits", "0|1: the host's mid-step waits use events behind the kernels instead of polled tag words",
     [](bh_ctx* c, const char* v) { return parse_flag(v, &c->knob_event_waits); }},
    {"readback_copy", "0|1: counts and gate word reach the host through copy launches",
     [](bh_ctx* c, const char* v) { return parse_flag(v, &c->knob_readback_copy); }},
    {"force_exchange", "0|1: a one-rank communicator still walks the whole gradient-exchange path (overhead measurement)",
     [](bh_ctx* c, const char* v) { return parse_flag(v, &c->knob_force_exchange); }},
    {"zero_grads", "0|1: the single-GPU train step zero-fills its gradient span like the exchange path",
     [](bh_ctx* c, const char* v) { return parse_flag(v, &c->knob_zero_grads); }},
    {"loss_bands", "0|1: the fused loss's blocks take their tiles by XCD column bands (1) or row-major (0)",
     [](bh_ctx* c, const char* v) { return parse_u32(v, 0, 1, &c->knob_loss_bands); }},
    {"update_rows", "0|64|128|256: splats per block of the update kernel (0 = default)",
     [](bh_ctx* c, const char* v) { uint32_t u = 0; if (!parse_u32(v, 0, 256, &u) || !(u == 0 || u == 64 || u == 128 || u == 256)) return false; c->knob_update_rows = u; return true; }},
    {"no_dormant", "0|1: the update kernel fetches and updates dormant splats like everyone else",
     [](bh_ctx* c, const char* v) { return parse_flag(v, &c->knob_no_dormant); }},
    {"sort_kpt", "0|4|8|16: keys per thread of the generic radix sort (0 = default)",
     [](bh_ctx* c, const char* v) { uint32_t u = 0; if (!parse_u32(v, 0, 16, &u) || !(u == 0 || u == 4 || u == 8 || u == 16)) return false; c->knob_sort_kpt = u; return true; }},
    {"grad_allreduce", "ring|direct: the dense gradient block's collective — ncclAllReduce, or reduce-scatter + all-gather over grouped send/recv",
     [](bh_ctx* c, const char* v) { const std::string w(v); if (w == "ring") { c->knob_direct_allreduce = false; return true; } if (w == "direct") { c->knob_direct_allreduce = true; return true; } return false; }},
    {"update_sparse", "0..256: an update block with at most this many non-dormant rows fetches them in one round trip (0: never; 256: every block that may skip dormant rows; default 64 at SH degree 0, else 0)",
     [](bh_ctx* c, const char* v) { uint32_t u = 0; if (!parse_u32(v, 0, 256, &u)) return false; c->knob_update_sparse = (int)u; return true; }},
    {"feature_chunk", "0|4|8|16: channels per pass over the lists of the feature-map blends (0 = chosen per channel count)",
     [](bh_ctx* c, const char* v) { uint32_t u = 0; if (!parse_u32(v, 0, 16, &u) || !(u == 0 || u == 4 || u == 8 || u == 16)) return false; c->feature_chunk = u; return true; }},
};
constexpr int kOptionCount = (int)(sizeof(kOptions) / sizeof(kOptions[0]));
}  // namespace

extern "C" int bh_option_count(void) { return kOptionCount; }
extern "C" const char* bh_option_name(int i) { return i >= 0 && i < kOptionCount ? kOptions[i].name : nullptr; }
extern "C" const char* bh_option_help(int i) { return i >= 0 && i < kOptionCount ? kOptions[i].help : nullptr; }

extern "C" int bh_set_option(bh_ctx* ctx, const char* key, const char* value) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!key || !value) return set_error(ctx, BH_ERR_INVALID_ARG, "set_option: null key or value");
    const std::string k(key);
    for (const Option& o : kOptions) {
        if (k != o.name) continue;
        if (!o.apply(ctx, value)) return set_error(ctx, BH_ERR_INVALID_ARG, "set_option: bad value '" + std::string(value) + "' for '" + k + "'");
        return 0;
    }
    return set_error(ctx, BH_ERR_INVALID_ARG, "set_option: unknown key '" + k + "' (bh_option_name lists the keys)");
}

// ---- lens laws in f64 (brush-render/src/camera.rs:85-198) ------------------------------------
namespace {
struct Kb4Law {  // d(theta) = theta + k1 theta^3 + k2 theta^5 + k3 theta^7 + k4 theta^9   (camera.rs:120-142)
    double k[4];
    explicit Kb4Law(const float* d) { for (int i = 0; i < 4; ++i) k[i] = d ? (double)d[i] : 0.0; }
    double value(double th) const {
        const double t2 = th * th, t3 = t2 * th, t5 = t3 * t2, t7 = t5 * t2, t9 = t7 * t2;
        return th + k[0] * t3 + k[1] * t5 + k[2] * t7 + k[3] * t9;
    }
    double slope(double th) const {
        const double t2 = th * th, t4 = t2 * t2, t6 = t4 * t2, t8 = t6 * t2;
        return 1.0 + 3.0 * k[0] * t2 + 5.0 * k[1] * t4 + 7.0 * k[2] * t6 + 9.0 * k[3] * t8;
    }
    // Newton on d(theta) = target, theta in [0, pi] (camera.rs:145-167)
    double invert(double target) const {
        if (target <= 0.0) return 0.0;
        const double pi = 3.14159265358979323846;
        double th = target < pi - 1e-6 ? target : pi - 1e-6;
        for (int it = 0; it < 50; ++it) {
            const double fp = slope(th);
            if (std::fabs(fp) < 1e-12) break;
            double next = th - (value(th) - target) / fp;
            next = next < 0.0 ? 0.0 : (next > pi ? pi : next);
            const bool done = std::fabs(next - th) < 1e-12;
            th = next;
            if (done) break;
        }
        return th;
    }
};
struct Rt8Law {  // radial factor (1 + k1 r^2 + k2 r^4 + k3 r^6) / (1 + k4 r^2 + k5 r^4 + k6 r^6)   (camera.rs:170-178)
    double k[6];
    explicit Rt8Law(const float* d) { for (int i = 0; i < 6; ++i) k[i] = d ? (double)d[i] : 0.0; }
    double radial(double r) const {
        const double r2 = r * r, r4 = r2 * r2, r6 = r4 * r2;
        return (1.0 + k[0] * r2 + k[1] * r4 + k[2] * r6) / (1.0 + k[3] * r2 + k[4] * r4 + k[5] * r6);
    }
    // fixed-point r <- r_d / radial(r)   (camera.rs:182-198)
    double undistort(double r_d) const {
        double r = r_d;
        for (int it = 0; it < 30; ++it) {
            const double f = radial(r);
            if (std::fabs(f) < 1e-12) break;
            const double rn = r_d / f;
            const bool done = std::fabs(rn - r) < 1e-12;
            r = rn;
            if (done) break;
        }
        return r;
    }
};

// What bh_camera_setup_model and bh_camera_set_intrinsics (brush_hip_intrinsics.h) share: lim_* and half_max_render_fov of a camera
// whose model, dist, fx, fy, cx, cy, img_w and img_h are written, with the f64 fields of view its focals stand for.
void camera_limits(BhCamera* out, double fov_x, double fov_y) {
    // calculate_jacobian_clamp_limits (camera.rs:200-254): image edges +-15 %, in normalised coordinates
    const float wf = (float)out->img_w, hf = (float)out->img_h;
    float lim[4] = {(1.15f * wf - out->cx) / out->fx, (1.15f * hf - out->cy) / out->fy,
                    (-0.15f * wf - out->cx) / out->fx, (-0.15f * hf - out->cy) / out->fy};
    if (out->model == BH_CAMERA_RADIAL_TANGENTIAL_8) {
        // the clamp bounds the UNDISTORTED coordinate: invert the radial law at each edge
        const Rt8Law law(out->dist);
        for (float& e : lim) {
            const float mag = (float)law.undistort(std::fabs((double)e));
            e = (e != e) ? e : (std::signbit(e) ? -mag : mag);  // * f32::signum(edge)
        }
    } else if (out->model != BH_CAMERA_PINHOLE) {
        for (float& e : lim) e = 0.0f;  // fisheye Jacobians are not clamped
    }
    out->lim_pos_x = lim[0]; out->lim_pos_y = lim[1]; out->lim_neg_x = lim[2]; out->lim_neg_y = lim[3];
    // render.rs:70-71 (f32)
    const float full = hypotf((float)fov_x, (float)fov_y) * 1.05f;
    const float cap = 2.0f * 3.14159265358979323846f - 1e-6f;
    out->half_max_render_fov = (full < cap ? full : cap) * 0.5f;
}
}  // namespace

double bh_fov_to_focal(double fov, uint32_t pixels, uint32_t model, const float* dist) {
    const double half = fov / 2.0, r_pix = (double)pixels / 2.0;
    switch (model) {
        case BH_CAMERA_PINHOLE: return r_pix / std::tan(half);
        case BH_CAMERA_KANNALA_BRANDT_4:
        case BH_CAMERA_THIN_PRISM_FISHEYE: return r_pix / Kb4Law(dist).value(half);
        case BH_CAMERA_RADIAL_TANGENTIAL_8: { const double r = std::tan(half); return r_pix / (r * Rt8Law(dist).radial(r)); }
        default: return std::nan("");
    }
}

double bh_focal_to_fov(double focal, uint32_t pixels, uint32_t model, const float* dist) {
    const double r_norm = ((double)pixels / 2.0) / focal;
    switch (model) {
        case BH_CAMERA_PINHOLE: return 2.0 * std::atan(r_norm);
        case BH_CAMERA_KANNALA_BRANDT_4:
        case BH_CAMERA_THIN_PRISM_FISHEYE: return 2.0 * Kb4Law(dist).invert(r_norm);
        case BH_CAMERA_RADIAL_TANGENTIAL_8: return 2.0 * std::atan(Rt8Law(dist).undistort(r_norm));
        default: return std::nan("");
    }
}

// brush-render/src/camera.rs:63-101,200-254, render.rs:70-71; glam 0.30 Affine3A/Mat3A restated in f32.
int bh_camera_setup_model(const float* pos, const float* rot_xyzw, double fov_x, double fov_y, float center_u, float center_v,
                          uint32_t img_w, uint32_t img_h, uint32_t model, const float* dist, BhCamera* out) {
    if (!pos || !rot_xyzw || !out || img_w == 0 || img_h == 0 || model > BH_CAMERA_THIN_PRISM_FISHEYE) return BH_ERR_INVALID_ARG;
    const float x = rot_xyzw[0], y = rot_xyzw[1], z = rot_xyzw[2], w = rot_xyzw[3];
    const float x2 = x + x, y2 = y + y, z2 = z + z;
    const float xx = x * x2, xy = x * y2, xz = x * z2;
    const float yy = y * y2, yz = y * z2, zz = z * z2;
    const float wx = w * x2, wy = w * y2, wz = w * z2;
    // camera-to-world rotation columns (Mat3A::from_quat)
    const float ax[3] = {1.0f - (yy + zz), xy + wz, xz - wy};
    const float ay[3] = {xy - wz, 1.0f - (xx + zz), yz + wx};
    const float az[3] = {xz + wy, yz - wx, 1.0f - (xx + yy)};
    auto cross = [](const float* a, const float* b, float* o) {
        o[0] = a[1] * b[2] - b[1] * a[2];
        o[1] = a[2] * b[0] - b[2] * a[0];
        o[2] = a[0] * b[1] - b[0] * a[1];
    };
    float t0[3], t1[3], t2[3];
    cross(ay, az, t0);
    cross(az, ax, t1);
    cross(ax, ay, t2);
    const float det = (az[0] * t2[0]) + (az[1] * t2[1]) + (az[2] * t2[2]);
    const float inv_det = 1.0f / det;
    // Mat3A::inverse = from_cols(t0, t1, t2) * inv_det, transposed
    float r0[3], r1[3], r2[3];
    for (int i = 0; i < 3; ++i) { r0[i] = t0[i] * inv_det; r1[i] = t1[i] * inv_det; r2[i] = t2[i] * inv_det; }
    const float c0[3] = {r0[0], r1[0], r2[0]}, c1[3] = {r0[1], r1[1], r2[1]}, c2[3] = {r0[2], r1[2], r2[2]};
    for (int i = 0; i < 3; ++i) {
        out->vm[i] = c0[i];
        out->vm[3 + i] = c1[i];
        out->vm[6 + i] = c2[i];
        const float ip = (c0[i] * pos[0] + c1[i] * pos[1]) + c2[i] * pos[2];
        out->vm[9 + i] = -ip;
    }
    out->model = model;
    for (int i = 0; i < 8; ++i) out->dist[i] = (model != BH_CAMERA_PINHOLE && dist) ? dist[i] : 0.0f;
    out->fx = (float)bh_fov_to_focal(fov_x, img_w, model, out->dist);
    out->fy = (float)bh_fov_to_focal(fov_y, img_h, model, out->dist);
    out->cx = center_u * (float)img_w;
    out->cy = center_v * (float)img_h;
    out->img_w = img_w;
    out->img_h = img_h;
    camera_limits(out, fov_x, fov_y);
    out->cam_pos[0] = pos[0]; out->cam_pos[1] = pos[1]; out->cam_pos[2] = pos[2];
    out->tile_row_begin = 0;
    out->tile_row_end = 0;
    return 0;
}

int bh_camera_set_intrinsics(BhCamera* cam, double fx, double fy, double cx, double cy) {
    if (!cam || cam->img_w == 0 || cam->img_h == 0 || cam->model > BH_CAMERA_THIN_PRISM_FISHEYE) return BH_ERR_INVALID_ARG;
    if (!std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy) || !(fx > 0.0) || !(fy > 0.0)) return BH_ERR_INVALID_ARG;
    const double fov_x = bh_focal_to_fov(fx, cam->img_w, cam->model, cam->dist), fov_y = bh_focal_to_fov(fy, cam->img_h, cam->model, cam->dist);
    const float f[4] = {(float)fx, (float)fy, (float)cx, (float)cy};   // (a double that is no positive finite f32 is refused too)
    if (!std::isfinite(fov_x) || !std::isfinite(fov_y) || !(f[0] > 0.0f) || !(f[1] > 0.0f) || !std::isfinite(f[0]) || !std::isfinite(f[1]) ||
        !std::isfinite(f[2]) || !std::isfinite(f[3]))
        return BH_ERR_INVALID_ARG;
    cam->fx = f[0];
    cam->fy = f[1];
    cam->cx = f[2];
    cam->cy = f[3];
    camera_limits(cam, fov_x, fov_y);
    return 0;
}

int bh_camera_setup(const float* pos, const float* rot_xyzw, double fov_x, double fov_y, float center_u, float center_v,
                    uint32_t img_w, uint32_t img_h, BhCamera* out) {
    return bh_camera_setup_model(pos, rot_xyzw, fov_x, fov_y, center_u, center_v, img_w, img_h, BH_CAMERA_PINHOLE, nullptr, out);
}

// ---- forward -------------------------------------------------------------------
}  // extern "C"

// bh_render_forward and the train step: the request's checks, a deferred far-slice decision collected, then the pipeline
int bh::render_forward(bh_ctx* ctx, const ForwardRequest& req, BhRenderOut* out) {
    const BhCamera& cam = req.cam;
    if (cam.img_w == 0 || cam.img_h == 0) return set_error(ctx, BH_ERR_INVALID_ARG, "Can't render images with 0 size.");  // render.rs:50-53
    if (req.sh_degree > 4) return set_error(ctx, BH_ERR_INVALID_ARG, "sh_degree must be 0..4");
    if (cam.model > BH_CAMERA_THIN_PRISM_FISHEYE) return set_error(ctx, BH_ERR_INVALID_ARG, "unknown camera model");
    // (a splat's candidate box is walked with a 24-bit index: tile grids up to 4095 x 4095)
    if (cam.img_w > 65520 || cam.img_h > 65520) return set_error(ctx, BH_ERR_UNSUPPORTED, "images larger than 65520 px per side are not supported (tile grid <= 4095 x 4095)");
    if (req.n > 0 && (!req.transforms || !req.sh_coeffs || !req.raw_opacities)) return set_error(ctx, BH_ERR_INVALID_ARG, "render_forward: null splat tensor");
    if ((req.flags & BH_FLAG_SMOOTH_CUTOFF) && !(req.flags & BH_FLAG_BWD_INFO)) return set_error(ctx, BH_ERR_INVALID_ARG, "smooth cutoff requires the backward pass flag");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->far_job.pending) BH_TRY(finish_far_slice(ctx, nullptr));   // (a deferred decision nobody collected)
    return forward_impl(ctx, req, out);
}

extern "C" int bh_render_forward(bh_ctx* ctx, const BhCamera* cam, uint32_t n, uint32_t sh_degree, const float* transforms,
                                 const float* sh_coeffs, const float* raw_opacities, const float* background, uint32_t flags,
                                 BhRenderOut* out) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!cam || !out || !background) return set_error(ctx, BH_ERR_INVALID_ARG, "render_forward: null argument");
    ForwardRequest req;
    req.cam = *cam;
    req.n = n; req.sh_degree = sh_degree; req.flags = flags;
    req.transforms = transforms; req.sh_coeffs = sh_coeffs; req.raw_opacities = raw_opacities;
    req.bg[0] = background[0]; req.bg[1] = background[1]; req.bg[2] = background[2];
    req.view_id = ctx->view_id;
    return render_forward(ctx, req, out);
}

// The forward pipeline (arguments validated by render_forward).  req.allow_cut = false: complete lists whatever the view's table
// says (the second attempt after a failed forecast, finish_far_slice).
int bh::forward_impl(bh_ctx* ctx, const ForwardRequest& req, BhRenderOut* out) {
    const uint32_t n = req.n, sh_degree = req.sh_degree, flags = req.flags;
    const float* transforms = req.transforms;
    const float* sh_coeffs = req.sh_coeffs;
    const float* raw_opacities = req.raw_opacities;
    ctx->have_forward = false;
    ctx->clears.begin_forward();   // (filled in below only by the kernels of THIS forward)
    const bool mip = flags & BH_FLAG_MIP;
    Frame f;
    f.bwd_info = flags & BH_FLAG_BWD_INFO; f.smooth = flags & BH_FLAG_SMOOTH_CUTOFF;
    f.bg[0] = req.bg[0]; f.bg[1] = req.bg[1]; f.bg[2] = req.bg[2];
    f.u = make_uniforms(req.cam);
    if (f.u.tile_y0 >= f.u.tile_y1 || f.u.tile_y1 > f.u.tile_bh) return set_error(ctx, BH_ERR_INVALID_ARG, "tile_row window must satisfy begin < end <= ceil(img_h / 16)");
    f.num_tiles = f.u.tile_bw * f.u.tile_bh;
    const size_t npad = n ? n : 1;

    // two counter pairs: K1 accumulates into one and clears the other for the next forward (no fill launch)
    constexpr size_t counter_set_bytes = COUNTER_SET_BYTES, counter_set_words = COUNTER_SET_BYTES / 4, counter_read_bytes = COUNTER_READ_BYTES;
    auto* counter_pairs = (uint32_t*)ensure(ctx, SLOT_COUNTERS, 2 * counter_set_bytes + 64);   // (+ the device copy of this frame's count sums)
    uint32_t* dev_sums = counter_pairs ? counter_pairs + 2 * counter_set_words : nullptr;
    uint32_t* counters = counter_pairs ? counter_pairs + counter_set_words * (ctx->counter_phase & 1u) : nullptr;
    auto* depth_keys = (uint32_t*)ensure(ctx, SLOT_DEPTH_KEYS, npad * 4);
    auto* isect_counts = (uint32_t*)ensure(ctx, SLOT_ISECT_COUNTS, npad * 4);
    auto* max_radius = req.max_radius ? req.max_radius : (float*)ensure(ctx, SLOT_MAX_RADIUS, npad * 4);
    f.proj_by_gid = (float*)ensure(ctx, SLOT_PROJECTED_BY_GID, npad * 9 * 4);
    if (!counters || !depth_keys || !isect_counts || !max_radius || !f.proj_by_gid) return BH_ERR_OOM;

    f.gfc = (uint32_t*)ensure(ctx, SLOT_GLOBAL_FROM_COMPACT, npad * 4);
    auto* depths_sorted = (uint32_t*)ensure(ctx, SLOT_DEPTHS_SORTED, npad * 4);
    if (!f.gfc || !depths_sorted) return BH_ERR_OOM;
    // [T,2] offsets | 8 x LPT_CLASSES work-class counters | [8][LPT_CLASSES][ceil(T/8)] class lists (longest-first tile order of the backward)
    // backward jobs (rasterize.hip): the blend backward works on checkpointed segments of the tiles' lists
    const bool bwd_jobs = f.bwd_info && ctx->knob_bwd_jobs && !ctx->knob_no_lpt && !((flags & BH_FLAG_SLICED_LISTS) && ctx->slice_fraction > 0.0f);
    const size_t lpt_words = LPT_HEADER_WORDS + (size_t)8 * LPT_CLASSES * band_slots(f.num_tiles);
    auto* tile_offsets = (uint32_t*)ensure(ctx, SLOT_TILE_OFFSETS, ((size_t)f.num_tiles * 2 + lpt_words) * 4);
    f.visible = (f.bwd_info && req.visible) ? req.visible : (float*)ensure(ctx, SLOT_VISIBLE, (f.bwd_info ? npad : 1) * 4);
    if (!tile_offsets || !f.visible) return BH_ERR_OOM;
    const size_t visible_words = f.bwd_info ? ((req.visible && req.visible_floats) ? req.visible_floats : npad) : 0;
    // depth-sliced lists: [0] near-slice splats  [1] near-slice pairs  [2] tiles the near slice left unsaturated  [3] far-slice pairs |
    // done bits | far tile offsets [T,2] | far pairs per block group.  Cleared by K1 with the tile table, whether or not this frame ends up slicing.
    const bool want_sliced = (flags & BH_FLAG_SLICED_LISTS) != 0;
    const size_t slice_bit_words = ((size_t)f.num_tiles + 31) / 32;
    const size_t slice_group_words = (size_t)n / (256 * FAR_GROUP_BLOCKS) + 2;   // far pairs per group of count-kernel blocks
    const size_t slice_words = want_sliced ? SLICE_CTRL_WORDS + slice_bit_words + (size_t)f.num_tiles * 2 + slice_group_words : 0;
    uint32_t* slice_tab = nullptr;
    if (want_sliced) {
        slice_tab = (uint32_t*)ensure(ctx, SLOT_SLICE, slice_words * 4);
        if (!slice_tab) return BH_ERR_OOM;
    }
    // ---- per-tile depth cuts (BH_FLAG_SLICED_LISTS with the automatic share) ------------------------------------------------
    // A training loop comes back to each of its views every V steps with parameters that moved by a learning rate: how deep every
    // TILE of the view had to go last time is a near-exact forecast of how deep it has to go now.  So every blend launch leaves,
    // per tile, the depth key of the last splat the tile needed + a margin (rasterize.hip) in a table that belongs to the VIEW
    // (bh_set_view_id / BhTrainBatch.view_id), and the view's next frame lists a (splat, tile) pair only if the splat is at or in
    // front of the tile's cut: K1 counts those hits beside the exact ones (same walk), the scan runs over the near counts, K5 /
    // tile sort / offsets handle ~a tenth of the pairs — per tile, so a frame with thin or empty regions (whose tiles keep
    // "everything", i.e. their own short lists) is cut as deep as a frame that saturates everywhere.  Correctness does not rest
    // on the forecast: a tile that is still live behind an incomplete list is counted, and a frame with such a tile is rendered
    // AGAIN with complete lists (finish_far_slice: only the splats in front of the cuts were depth-ordered, so there is no far
    // pass to continue with); that second attempt re-seeds the table.
    ViewState* view = nullptr;
    bool cut_active = false;
    const bool auto_cuts = want_sliced && !(ctx->slice_fraction > 0.0f);
    // A frame with COMPLETE lists (no BH_FLAG_SLICED_LISTS: the reference's exact aux tensors, eval renders, exact_lists steps) takes
    // the view's table too — not to cut anything, but for the forward blend's tile order: its tiles start in descending order of the
    // work they had at the same camera's last frame (K16 193 -> ~150 us at 1 M splats / 1080p), and it refreshes the table.
    const bool order_only = !want_sliced && ctx->knob_k16_order != 0u && n >= 8u * 256u;
    if (n > 0 && (auto_cuts || order_only)) {
        view = frame_view(ctx, req, f.u.tile_bw, f.u.tile_bh, /*casual=*/order_only && !f.bwd_info);
        if (!view && auto_cuts) return set_error(ctx, BH_ERR_OOM, "hipMalloc for the per-view tile table failed");
        if (!view) (void)hipGetLastError();   // (ordering is optional: carry on in index order)
        cut_active = auto_cuts && view && cut_this_frame(ctx, view, req.allow_cut);
    }
    uint32_t* const vtab = view_table(view);   // [T] depth cuts | [T] per-tile work of the view's last frame | splitter tables
    uint32_t* near_counts = nullptr;
    uint32_t* tile_order = nullptr;
    uint32_t* tile_split = nullptr;
    if (cut_active) {
        near_counts = (uint32_t*)ensure(ctx, SLOT_NEAR_COUNTS, npad * 4);
        if (!near_counts) return BH_ERR_OOM;
    }

    uint32_t near_total = 0, nv_true = 0;
    bool fused_scan = false;
    uint32_t* cum_early = nullptr;
    bool k5_queued = false;   // K5 was queued before the counts were read (below): valid unless the pairs overflowed its buffers
    uint32_t spec_pair_cap = 0;
    float* spec_projected = nullptr;
    float4* spec_vc = nullptr;
    uint32_t *spec_tile_ids = nullptr, *spec_isect_gids = nullptr;
    if (n > 0) {
        fused_scan = depth_sort_supported(n) && !ctx->knob_generic_depth_sort;
        // (the sort's first kernel adds the counter slots up and stores the sums into the pinned block itself; only the generic
        //  sort path still needs a copy launch between K1 and the sort)
        const bool sums_on_device = fused_scan && !ctx->knob_readback_copy;
        // the depth sort's splitter table of this view and list mode — or, for a frame without a view, the ctx's own once a frame has made it
        bool* spl_written = nullptr;
        uint32_t* spl_listed = nullptr;
        uint32_t* spl = view_splitters(view, cut_active, &spl_written, &spl_listed);
        if (!spl && ctx->dsort_spl) { spl = ctx->dsort_spl; spl_written = &ctx->dsort_spl_written; spl_listed = &ctx->dsort_spl_keys; }
        DealArgs dealt;   // K1 deals the listed splats into the depth sort's buckets (depth_deal.h)
        {
            ProfScope ps(ctx, "ProjectSplats");
            if (!ctx->counters_ready) BH_HIP(ctx, hipMemsetAsync(counter_pairs, 0, 2 * counter_set_bytes, ctx->stream));
            ctx->counters_ready = false;
            ForwardPrep prep;
            prep.next_counters = reinterpret_cast<unsigned long long*>(counter_pairs + counter_set_words * ((ctx->counter_phase & 1u) ^ 1u));
            prep.visible = visible_words ? reinterpret_cast<uint32_t*>(f.visible) : nullptr;
            prep.visible_words = (uint32_t)visible_words;
            prep.tile_table = tile_offsets;
            prep.tile_words = f.num_tiles * 2 + LPT_HEADER_WORDS;
            prep.slice_table = slice_tab;
            prep.slice_words = (uint32_t)slice_words;
            prep.list_all_visible = ctx->knob_cut_sort_all;
            if (view && ctx->knob_k16_order && n >= 8u * 256u) {   // the forward blend's tile order from the view's last per-tile work (K1's blocks 0..7 sort it: the grid must have them)
                const uint32_t win_t = f.u.tile_bw * (f.u.tile_y1 - f.u.tile_y0);
                tile_order = (uint32_t*)ensure(ctx, SLOT_TILE_ORDER, ((size_t)8 * band_slots(win_t) + SPLIT_TAIL_WORDS) * 4);
                if (!tile_order) return BH_ERR_OOM;
                prep.order_work = vtab + (size_t)f.num_tiles;
                prep.order_out = tile_order;
                prep.order_tiles = win_t;
                prep.order_tile_begin = f.u.tile_bw * f.u.tile_y0;
                prep.order_mode = ctx->knob_k16_order;
                prep.band_mode = ctx->knob_band_mode;
                if (ctx->knob_k16_split && ctx->knob_k16_order == 1u) {   // split tiles (context.h SPLIT_MAX): K1's order blocks pick them
                    tile_split = tile_order + (size_t)8 * band_slots(win_t);
                    prep.split_out = tile_split;
                    prep.split_factor = (float)ctx->knob_k16_split * 0.01f;
                    prep.split_min = ctx->knob_k16_split_min;
                    prep.split_of_max = (float)ctx->knob_k16_split_of_max * 0.01f;
                }
            }
            if (f.bwd_info && req.grad_begin && req.grad_floats && (req.grad_floats & 3u) == 0 &&
                (reinterpret_cast<uintptr_t>(req.grad_begin) & 15u) == 0 && req.grad_floats / 4 <= 0xFFFFFFFFull) {
                prep.span = reinterpret_cast<float4*>(req.grad_begin);   // the train step's gradient span
                prep.span_f4 = (uint32_t)(req.grad_floats / 4);
                ctx->clears.k1_cleared_span();
            }
            BH_TRY(depth_deal_prepare(ctx, n, spl, sums_on_device && spl_written && *spl_written && depth_deal_table_usable(*spl_listed), &prep));
            dealt = prep.deal;
            BH_TRY(launch_project_forward(ctx, f.u, n, mip, sh_degree, transforms, sh_coeffs, raw_opacities, depth_keys, isect_counts, max_radius,
                                          f.proj_by_gid, counters, prep, cut_active ? vtab : nullptr, near_counts));
            ctx->counter_phase ^= 1u;
            ctx->counters_ready = true;
        }
        // the one mid-pipeline readback (render.rs:146-168).  The depth sort covers all n splats
        // and needs neither count, so it is queued BEFORE the host waits: the GPU sorts while the
        // host reads the counts, sizes the buffers and queues the rest.
        auto* hslots = reinterpret_cast<unsigned long long*>(ctx->host_counters + 16);
        // ... and the host does not wait for an event behind that kernel either: it polls a tag word the kernel stores behind the sums
        const bool poll_tag = sums_on_device && !ctx->knob_event_waits;
        if (!sums_on_device) {
            BH_HIP(ctx, hipMemcpyAsync(hslots, counters, counter_read_bytes, hipMemcpyDeviceToHost, ctx->stream));
            BH_HIP(ctx, hipEventRecord(ctx->readback_ev, ctx->stream));
        }
        {
            ProfScope ps(ctx, "DepthSort");
            // culled splats carry key 0xFFFFFFFF and sort behind every visible one:
            // the stable sort is also the (deterministic) compaction.
            if (fused_scan) {
                // ... and the scan of the tile counts in depth order rides on its last kernel (depth_sort.hip); the arena's
                // cum slot is sized for n here because the visible count is not known yet
                cum_early = (uint32_t*)ensure(ctx, SLOT_CUM_TILES_HIT, npad * 4);
                if (!cum_early) return BH_ERR_OOM;
                // (per-tile cuts: the scan of the NEAR counts = the slot ranges of the near pass's list)
                if (poll_tag && ++ctx->readback_tag == 0u) ctx->readback_tag = 1u;
                BH_TRY(depth_sort_scan(ctx, depth_keys, counters + COUNTER_MINMAX_WORD, cut_active ? near_counts : isect_counts, n, depths_sorted, f.gfc, cum_early,
                                       sums_on_device ? counters : nullptr, ctx->host_counters + 16, ctx->readback_ev, poll_tag ? ctx->readback_tag : 0u,
                                       sums_on_device ? dev_sums : nullptr, spl, spl_written, &dealt));
            } else {
                BH_TRY(radix_argsort(ctx, depth_keys, nullptr, n, 32, depths_sorted, f.gfc));
            }
        }
        // ---- speculative K5: the list builder is queued BEFORE the host has read the counts.  Between the depth sort's last kernel and
        // K5 the GPU used to idle ~5.5 us every frame — the host learns the counts ~70 us into the frame, but sizing and launching K5
        // only then made K5's launch latency a bubble (the one idle gap a kernel trace of a step shows, scripts/gap_trace.py).  K5
        // needs two numbers the host does not have yet: the listed splats (it reads them on the device, where the sort's first kernel
        // left the sums) and room for the pairs — the pair buffers' CAPACITY is the bound: the arena only grows, so after a view's
        // first frames it holds what the frame needs; a wave whose slots would not fit emits nothing, the host finds the overflow in
        // the counts it reads anyway and queues K5 again behind the grown buffers.
        if (poll_tag && ctx->knob_spec_k5 && !(want_sliced && ctx->slice_fraction > 0.0f)) {
            const size_t cap_pairs = std::min(ctx->slots[SLOT_TILE_IDS].cap, ctx->slots[SLOT_ISECT_GIDS].cap) / 4;
            if (cap_pairs >= 4096) {
                spec_projected = (float*)ensure(ctx, SLOT_PROJECTED, npad * 9 * 4);   // (rows for up to n listed splats)
                spec_vc = f.bwd_info ? (float4*)ensure(ctx, SLOT_V_COMBINED, npad * 10 * 4 + 16) : nullptr;
                if (!spec_projected || (f.bwd_info && !spec_vc)) return BH_ERR_OOM;
                spec_tile_ids = (uint32_t*)ctx->slots[SLOT_TILE_IDS].ptr;
                spec_isect_gids = (uint32_t*)ctx->slots[SLOT_ISECT_GIDS].ptr;
                spec_pair_cap = (uint32_t)std::min<size_t>(cap_pairs, 0xFFFFFFFEull);
                ProfScope ps(ctx, "MapGaussiansToIntersect");
                BH_TRY(launch_map_gaussians(ctx, n, f.u, f.proj_by_gid, f.gfc, spec_projected, cum_early, spec_tile_ids, spec_isect_gids, spec_vc,
                                            spec_vc ? (uint32_t)(((size_t)n * 10 + 3) / 4) : 0u, 0xFFFFFFFFu, cut_active ? slice_tab : nullptr,
                                            cut_active ? vtab : nullptr, cut_active ? depths_sorted : nullptr, dev_sums + (cut_active ? 3 : 0), spec_pair_cap));
                k5_queued = true;
            }
        }
        if (poll_tag) BH_TRY(wait_host_tag(ctx, reinterpret_cast<const volatile uint32_t*>(hslots) + HOST_SUM_WORDS - 1u, ctx->readback_tag, "count readback"));
        else BH_HIP(ctx, hipEventSynchronize(ctx->readback_ev));
        if (ctx->gate_learn) {   // the previous sliced frame queued its far slice unasked: did it need it?
            ctx->gate_learn = false;
            ctx->far_direct = reinterpret_cast<const volatile uint32_t*>(ctx->host_counters)[HOST_GATE_WORD] != 0u;
        }
        unsigned long long hc[4] = {0ull, 0ull, 0ull, 0ull};
        if (sums_on_device) {
            const volatile unsigned long long* hs = hslots;
            for (uint32_t c = 0; c < COUNTER_K1_U64; ++c) hc[c] = hs[c];
        } else {
            for (uint32_t k = 0; k < COUNTER_SLOTS; ++k)
                for (uint32_t c = 0; c < COUNTER_K1_U64; ++c) hc[c] += hslots[COUNTER_K1_U64 * k + c];
        }
        if (hc[1] > 0xFFFFFFFFull) return set_error(ctx, BH_ERR_UNSUPPORTED, "more than 2^32-1 tile intersections");
        nv_true = (uint32_t)hc[0];
        f.ni = (uint32_t)hc[1];
        near_total = cut_active ? (uint32_t)hc[2] : f.ni;
        // per-tile cuts: only the splats that own a pair in front of some cut were given a real depth key (K1): the compact
        // arrays, K5's grid, the backward's accumulator and K18 are sized for THEM; num_visible stays the reference's count
        f.nv = cut_active ? (uint32_t)hc[3] : nv_true;   // (BH_CUT_SORT_ALL: K1 then listed every visible splat, hc[3] == hc[0])
        if (dealt.ctr && reinterpret_cast<const volatile uint32_t*>(hslots)[HOST_DEAL_WORD] != 0u) {
            // K1 ran out of slots in a bucket (depth_deal.h): the deal's bucket launch did nothing, and told the kernels queued behind it that
            // nothing is listed.  The order comes from depth_keys and the counts through the three launches, and K5 is queued again behind them,
            // the way a pair-buffer overflow queues it again.
            // (The host has the counts already.  The counter set is handed over once more only because the histogram kernel's readback block is
            //  what refreshes dev_sums, which the deal's launch zeroed and K5 reads: it stores the same sums into the pinned words again, behind
            //  the host's read of them, clears HOST_DEAL_WORD, leaves the tag alone, and its event is one nobody waits for.)
            ProfScope ps(ctx, "DepthSort");
            ctx->deal_fallbacks++;
            BH_TRY(depth_sort_scan(ctx, depth_keys, counters + COUNTER_MINMAX_WORD, cut_active ? near_counts : isect_counts, n, depths_sorted, f.gfc, cum_early,
                                   counters, ctx->host_counters + 16, ctx->readback_ev, 0u, dev_sums, spl, spl_written));
            k5_queued = false;
        }
        if (fused_scan && spl_listed && (spl_written == nullptr || *spl_written)) *spl_listed = f.nv;   // this frame's bucket kernel rewrote the table: quantiles iff f.nv >= SPL_MIN_KEYS
    } else {   // no K1 to clear them on the way
        BH_HIP(ctx, hipMemsetAsync(tile_offsets, 0, ((size_t)f.num_tiles * 2 + LPT_HEADER_WORDS) * 4, ctx->stream));
        if (visible_words) BH_HIP(ctx, hipMemsetAsync(f.visible, 0, visible_words * 4, ctx->stream));
    }

    const size_t nvpad = f.nv ? f.nv : 1, nipad = f.ni ? f.ni : 1;
    f.cum = fused_scan ? cum_early : (uint32_t*)ensure(ctx, SLOT_CUM_TILES_HIT, nvpad * 4);
    f.projected = (float*)ensure(ctx, SLOT_PROJECTED, nvpad * 9 * 4);
    f.tile_ids = (uint32_t*)ensure(ctx, SLOT_TILE_IDS, nipad * 4);
    f.isect_gids = (uint32_t*)ensure(ctx, SLOT_ISECT_GIDS, nipad * 4);
    f.tile_ids_sorted = (uint32_t*)ensure(ctx, SLOT_TILE_IDS_SORTED, nipad * 4);
    f.isect_gids_sorted = (uint32_t*)ensure(ctx, SLOT_ISECT_GIDS_SORTED, nipad * 4);
    const size_t pixels = (size_t)f.u.img_w * f.u.img_h;
    void* out_img = ensure(ctx, SLOT_OUT_IMG, pixels * (f.bwd_info ? 16 : 4));
    if (!f.cum || !f.projected || !f.tile_ids || !f.isect_gids || !f.tile_ids_sorted || !f.isect_gids_sorted || !out_img)
        return BH_ERR_OOM;
    // the speculative K5 stands if its pairs fitted and none of its buffers has moved since
    if (k5_queued && ((cut_active ? near_total : f.ni) > spec_pair_cap || f.projected != spec_projected || f.tile_ids != spec_tile_ids || f.isect_gids != spec_isect_gids))
        k5_queued = false;

    // ---- depth-sliced lists (BH_FLAG_SLICED_LISTS) --------------------------------------------------------------------------
    // The reference lists EVERY (tile, splat) pair and sorts them all (map_gaussians.rs:15-80, render.rs:228-230), although a tile
    // stops blending once its 256 pixels are saturated (rasterize.rs:116-189): at 1 M splats / 1080p the blend reads 9 % of the
    // sorted list, at 6 M / 4K 1.7 %.  The splats are in depth order and cum_tiles_hit is their slot ranges, so "slot end <= budget"
    // is a NEAR slice of the depth order whose pairs are the first I0 slots of the exact list.  List + sort + blend that slice;
    // tiles whose pixels all saturated are final (one bit each); the FAR rest is listed only into tiles that are not
    // (count -> emit against the bit table), sorted behind the near list and blended from the parked pixel state.
    // Everything the far slice launches is a no-op when no tile is left (a device-side gate: no host round trip).  Per pixel the
    // same splats are folded in the same order: out_img, visible[], the blended part of every list and the gradients are those
    // of the exact path.  The near slice's size comes from the per-tile cuts of the view's last frame (lists.hip list_budget), or
    // from bh_set_list_slicing.
    f.budget = want_sliced && f.ni > 0 ? list_budget(ctx, cut_active ? view : nullptr, near_total, f.ni) : f.ni;   // == ni: one slice, the exact lists
    const bool sliced = f.budget < f.ni;
    const bool by_cut = cut_active && sliced;           // this frame's lists end at the per-tile cuts
    const uint32_t* zcut_lists = cut_active ? vtab : nullptr;   // (cut_active but not sliced: the cut removed nothing — K5 still filters, and keeps everything)
    f.slice_info = slice_tab;
    f.done_bits = slice_tab ? slice_tab + SLICE_CTRL_WORDS : nullptr;
    f.tile_offsets_far = slice_tab ? slice_tab + SLICE_CTRL_WORDS + slice_bit_words : nullptr;
    f.far_group_totals = slice_tab ? slice_tab + SLICE_CTRL_WORDS + slice_bit_words + (size_t)f.num_tiles * 2 : nullptr;
    while (f.tile_bits < 32 && (f.num_tiles >> f.tile_bits) != 0) f.tile_bits++;  // render.rs:228
    if (bwd_jobs) {
        // checkpoint slots are addressed by list position (context.h BwdJobs): listed pairs / BWD_SEG + tiles of them
        const uint32_t listed = cut_active ? near_total : f.ni;
        const uint32_t ckpt_cap = (uint32_t)std::min<uint64_t>((uint64_t)listed / BWD_SEG + f.num_tiles + 1u, BWD_CKPT_MAX_SLOTS);
        f.rs.jobs.ckpt = (float4*)ensure(ctx, SLOT_BWD_CKPT, (size_t)ckpt_cap * 256 * sizeof(float4));
        f.rs.jobs.ckpt_cap = ckpt_cap;
        f.rs.jobs.top_cap = band_slots(f.num_tiles) + ckpt_cap;   // (a band's full segments: at most one per checkpoint + one per tile)
        f.rs.jobs.top_list = (uint32_t*)ensure(ctx, SLOT_BWD_TOPLIST, (size_t)8 * f.rs.jobs.top_cap * 4);
        if (!f.rs.jobs.ckpt || !f.rs.jobs.top_list) return BH_ERR_OOM;
    }
    if (view) {   // every forward of a view refreshes its table
        f.rs.zcut = vtab;
        f.rs.depth_keys_sorted = depths_sorted;
        f.rs.nv = f.nv;
        f.rs.cut_active = by_cut;
        f.rs.margin_pct = cut_margin_pct(ctx, view);
        f.rs.work = vtab + (size_t)f.num_tiles;
        f.rs.order = tile_order;
        f.rs.order_mode = ctx->knob_k16_order;
        f.rs.split = tile_split;
#ifdef BH_TEST_HOOKS
        ctx->last_split = tile_split;
#endif
    }
    // work classes ~1/64 of the mean list length wide (a tile typically blends ~10 % of its list before it saturates)
    const uint32_t win_tiles = f.u.tile_bw * (f.u.tile_y1 - f.u.tile_y0);
    const float class_width_raw = (float)f.ni / (float)(win_tiles ? win_tiles : 1u) / 64.0f;
    f.class_width = ctx->knob_lpt_linear ? (class_width_raw < 8.0f ? 8.0f : class_width_raw) : 0.0f;   // (0: logarithmic classes, rasterize.hip)
    f.lpt = (f.bwd_info && !ctx->knob_no_lpt) ? tile_offsets + (size_t)f.num_tiles * 2 : nullptr;
    f.out_f32 = f.bwd_info ? (float*)out_img : nullptr;
    f.out_u8 = f.bwd_info ? nullptr : (uint32_t*)out_img;

    bool offsets_done = false;   // the tile sort wrote the offsets table on its way
    if (f.nv > 0) {
        if (!fused_scan) {
            ProfScope ps(ctx, "PrefixSumGaussHits");
            BH_TRY(prefix_sum(ctx, cut_active ? near_counts : isect_counts, f.gfc, f.nv, f.cum, false));
        }
        if (f.ni == 0) {   // nothing to map: only the record gather is left (K5 does it on its way otherwise)
            ProfScope ps(ctx, "ProjectVisible");
            BH_TRY(launch_project_visible(ctx, f.nv, f.proj_by_gid, f.gfc, f.projected));
        }
        if (f.ni > 0) {
            {
                ProfScope ps(ctx, "MapGaussiansToIntersect");
                // the backward's accumulator [nv,10] is cleared by K5 on its way (whole float4s: + 16 B of room)
                float4* vc = nullptr;
                if (f.bwd_info) {
                    vc = (float4*)ensure(ctx, SLOT_V_COMBINED, (size_t)f.nv * 10 * 4 + 16);
                    if (!vc) return BH_ERR_OOM;
                }
                if (zcut_lists && near_total == 0u) {
                    // no pair in front of any cut: nothing to emit (and K5 does not run to clear v_combined)
                } else if (k5_queued && (!f.bwd_info || vc == spec_vc)) {
                    ctx->clears.k5_cleared_accum(vc != nullptr);   // (it ran in front of the count readback)
                } else {
                    ctx->clears.k5_cleared_accum(vc != nullptr);
                    BH_TRY(launch_map_gaussians(ctx, f.nv, f.u, f.proj_by_gid, f.gfc, f.projected, f.cum, f.tile_ids, f.isect_gids, vc, vc ? (uint32_t)(((size_t)f.nv * 10 + 3) / 4) : 0u,
                                                (sliced && !by_cut) ? f.budget : 0xFFFFFFFFu, (sliced || zcut_lists) ? f.slice_info : nullptr, zcut_lists,
                                                zcut_lists ? depths_sorted : nullptr));
                }
            }
            {
                ProfScope ps(ctx, "TileSort");
                // (scratch sized for the whole list: the near list's length moves from frame to frame)
                // host-known lengths: the sort that also writes the offsets table, four launches instead of seven (sort.hip)
                if ((zcut_lists || !sliced) && tile_sort_supported(f.tile_bits, zcut_lists ? near_total : f.ni) && !(ctx->knob_tile_sort == 2u)) {
                    BH_TRY(tile_sort_offsets(ctx, f.tile_ids, f.isect_gids, zcut_lists ? near_total : f.ni, f.tile_bits, f.num_tiles, f.tile_ids_sorted, f.isect_gids_sorted,
                                             tile_offsets, f.ni));
                    offsets_done = true;
                } else
                if (zcut_lists) BH_TRY(radix_argsort_dev(ctx, f.tile_ids, f.isect_gids, near_total, nullptr, nullptr, nullptr, f.tile_bits, f.tile_ids_sorted, f.isect_gids_sorted, f.ni));
                else if (sliced) BH_TRY(radix_argsort_dev(ctx, f.tile_ids, f.isect_gids, f.budget, f.slice_info + 1, nullptr, nullptr, f.tile_bits, f.tile_ids_sorted, f.isect_gids_sorted, f.ni));
                else BH_TRY(radix_argsort(ctx, f.tile_ids, f.isect_gids, f.ni, f.tile_bits, f.tile_ids_sorted, f.isect_gids_sorted));
            }
        }
    }
    if (!offsets_done) {
        ProfScope ps(ctx, "GetTileOffsets");   // K1 cleared the table (or a fill did, for n == 0)
        if (zcut_lists) BH_TRY(launch_tile_offsets(ctx, f.tile_ids_sorted, near_total, f.num_tiles, tile_offsets, /*pre_zeroed=*/true));
        else if (sliced) BH_TRY(launch_tile_offsets_dev(ctx, f.tile_ids_sorted, f.budget, f.slice_info + 1, nullptr, nullptr, f.num_tiles, tile_offsets));
        else BH_TRY(launch_tile_offsets(ctx, f.tile_ids_sorted, f.ni, f.num_tiles, tile_offsets, /*pre_zeroed=*/true));
    }
    if (!sliced) {
        ProfScope ps(ctx, "Rasterize");   // `visible` was cleared by K1 as well
        BH_TRY(launch_rasterize(ctx, f.u, f.bg, f.bwd_info, f.smooth, f.isect_gids_sorted, tile_offsets, f.projected, f.gfc, f.out_f32, f.out_u8, f.visible, f.lpt,
                                f.class_width, /*phase=*/0, &f.rs));
    } else {
        auto* state = (float*)ensure(ctx, SLOT_SLICE_STATE, pixels * 16);
        f.far_counts = (uint32_t*)ensure(ctx, SLOT_SLICE_COUNTS, nvpad * 4);
        f.far_block_totals = (uint32_t*)ensure(ctx, SLOT_SLICE_CUM, (nvpad / 256 + 2) * 4);
        if (!state || !f.far_counts || !f.far_block_totals) return BH_ERR_OOM;
        f.rs.done_bits = f.done_bits;
        f.rs.unsat_count = f.slice_info + 2;
        if (!ctx->knob_readback_copy) {
            // how many tiles are left, for the host (to decide now, or to learn for the next frame: context.h far_direct): the
            // blend kernel stores into the pinned word itself.  Nothing of an earlier frame can still write it — every frame's
            // count readback waited behind the previous frame's blend.
            f.rs.gate_host = ctx->host_counters + HOST_GATE_WORD;
            *reinterpret_cast<volatile uint32_t*>(f.rs.gate_host) = 0u;
        }
        f.rs.state = state;
        f.rs.offsets_near = tile_offsets;
        f.rs.live_bands = f.slice_info + 4;
        {
            ProfScope ps(ctx, "Rasterize");
            BH_TRY(launch_rasterize(ctx, f.u, f.bg, f.bwd_info, f.smooth, f.isect_gids_sorted, tile_offsets, f.projected, f.gfc, f.out_f32, f.out_u8, f.visible, f.lpt,
                                    f.class_width, /*phase=*/1, &f.rs));
        }
        FarJob& j = ctx->far_job;
        j.frame = f;
        j.by_cut = by_cut;
        j.view = by_cut ? view : nullptr;
        j.view_shared = req.view_id == 0u && ctx->knob_no_view_hash;   // (one table shared by every frame without an id: the A/B knob only)
        if (by_cut) j.req = req;   // what a second attempt with complete lists needs (finish_far_slice)
        if (ctx->knob_readback_copy)
            BH_HIP(ctx, hipMemcpyAsync(ctx->host_counters + HOST_GATE_WORD, f.slice_info + 2, 4, hipMemcpyDeviceToHost, ctx->stream));
        // (per-tile cuts: the forecast is expected to hold — the host decides every time, the train step (train.hip) hides the wait behind its
        //  loss kernels)
        if (ctx->far_direct && !by_cut) {
            BH_TRY(enqueue_far_slice(ctx, j));
            ctx->gate_learn = true;
        } else {
            // the train step (req.defer_decision) queues its loss kernels next and lets the first of them signal "the blend is done" through a
            // tag word: no event behind the blend (finish_far_slice records one late if nobody queued the signal)
            if (++ctx->gate_tag == 0u) ctx->gate_tag = 1u;
            j.gate_tag = ctx->gate_tag;
            ctx->gate_signal_queued = false;
            j.gate_event_recorded = !(req.defer_decision && !ctx->knob_event_waits && !ctx->knob_readback_copy);
            if (j.gate_event_recorded) BH_HIP(ctx, hipEventRecord(ctx->gate_ev, ctx->stream));
            j.pending = true;
            if (!req.defer_decision) {
                bool again = false;
                BH_TRY(finish_far_slice(ctx, &again));
                if (by_cut && again) {   // the forecast failed and the frame was rendered a second time, with complete lists: that is the result
                    *out = ctx->latest.out;
                    return 0;
                }
            }
        }
    }

    BhRenderOut r{};
    r.num_visible = nv_true;
    r.num_listed_splats = f.nv;
    r.num_intersections = f.ni;
    r.num_tiles = f.num_tiles;
    r.tile_bw = f.u.tile_bw;
    r.tile_bh = f.u.tile_bh;
    r.flags = flags;
    r.out_img = f.bwd_info ? (float*)out_img : nullptr;
    r.out_img_packed = f.bwd_info ? nullptr : (uint32_t*)out_img;
    r.visible = f.bwd_info ? f.visible : nullptr;
    r.max_radius = max_radius;
    r.tile_offsets = tile_offsets;
    r.projected = f.projected;
    r.compact_gid_from_isect = f.isect_gids_sorted;
    r.tile_id_from_isect = f.tile_ids_sorted;
    r.global_from_compact_gid = f.gfc;
    r.cum_tiles_hit = f.cum;
    r.intersect_counts = isect_counts;
    r.depths_sorted = (float*)depths_sorted;
    r.tile_offsets_far = sliced ? f.tile_offsets_far : nullptr;
    r.list_budget = f.budget;   // (per-tile cuts: the pairs the near pass listed)
    r.generation = ++ctx->generation;
    ctx->clears.stamp(r.generation);
    *out = r;
    ForwardState& latest = ctx->latest;
    latest.out = r;
    latest.uniforms = f.u;
    latest.n = n; latest.sh_degree = sh_degree; latest.flags = flags;
    latest.bg[0] = f.bg[0]; latest.bg[1] = f.bg[1]; latest.bg[2] = f.bg[2];
    latest.lpt = f.lpt;
    latest.jobs = f.rs.jobs;
    ctx->have_forward = true;
    if (view) view_rendered(view, f.ni);   // this frame's blend kernel leaves what every tile needed
    return 0;
}

extern "C" {

int bh_set_list_slicing(bh_ctx* ctx, float near_share) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (near_share != near_share || near_share > 1.0f) return set_error(ctx, BH_ERR_INVALID_ARG, "set_list_slicing: the near slice's share must be <= 1 (<= 0: automatic)");
    ctx->slice_fraction = near_share > 0.0f ? near_share : 0.0f;
    return 0;
}

int bh_set_list_cut_threshold(bh_ctx* ctx, uint32_t min_pairs) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    ctx->cut_min_pairs = min_pairs;
    return 0;
}

int bh_set_view_id(bh_ctx* ctx, uint32_t view_id) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    ctx->view_id = view_id;
    return 0;
}

int bh_forget_views(bh_ctx* ctx) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    BH_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->far_job.pending) BH_TRY(finish_far_slice(ctx, nullptr));
    // (the depth sort's splitter tables are per-ctx state of the same kind: a run that starts over starts from the linear split)
    if (ctx->dsort_spl) { BH_HIP(ctx, hipMemsetAsync(ctx->dsort_spl, 0, DSORT_SPL_STRIDE * 4, ctx->stream)); ctx->dsort_spl_written = false; ctx->dsort_spl_keys = 0u; }
    if (ctx->views.empty()) return 0;
    BH_HIP(ctx, hipStreamSynchronize(ctx->stream));   // queued kernels may still use the tables
    deliver_pending_loss(ctx);
    for (auto& kv : ctx->views)
        if (kv.second.zcut) (void)hipFree(kv.second.zcut);
    ctx->views.clear();
    ctx->casual_views = 0;
    for (uint64_t& k : ctx->seen_keys) k = 0ull;
    ctx->far_job.view = nullptr;
    ctx->margin_scale = 1.0f;
    return 0;
}

float bh_last_list_share(bh_ctx* ctx) { return ctx ? ctx->last_slice_share : 0.0f; }
uint32_t bh_far_slices_queued(bh_ctx* ctx) { return ctx ? ctx->far_launches : 0u; }
uint32_t bh_view_table_count(bh_ctx* ctx) { return ctx ? (uint32_t)ctx->views.size() : 0u; }

// ---- backward ------------------------------------------------------------------
}  // extern "C"

namespace bh {

// The two backward kernels on the saved state `fs` (bwd/render_bwd.rs:21-171).  What the forward's kernels cleared on their way is
// recorded in ctx->clears under that forward's generation: a backward of any other forward (a retained, older one) finds nothing
// there and clears everything itself.  `call` (context.h BackwardCall) says what else: K17 does not run without a v_output; the
// terms' raw sums join the accumulator between K17 and K18 and each hands the per-splat vector it filled (v_z, Vn) to its scatter
// behind K18 — one v_z scatter serves the depth and the distortion term — on row marks too.
int backward_impl(bh_ctx* ctx, const ForwardState& fs, const float* v_output, const BackwardCall& call) {
    const float *transforms = call.transforms, *sh_coeffs = call.sh_coeffs, *raw_opacities = call.raw_opacities;
    float *v_transforms = call.v_transforms, *v_sh_coeffs = call.v_sh_coeffs, *v_raw_opacities = call.v_raw_opacities, *v_refine_weight = call.v_refine_weight;
    const size_t span_floats = call.span_floats;
    const BhRenderOut& r = fs.out;
    const uint32_t n = fs.n, nv = r.num_listed_splats, C = (fs.sh_degree + 1) * (fs.sh_degree + 1);
    const size_t nvpad = nv ? nv : 1;
    auto* v_combined = (float*)ensure(ctx, SLOT_V_COMBINED, nvpad * 10 * 4 + 16);   // + room to clear whole float4s
    if (!v_combined) return BH_ERR_OOM;
    bool row_marks = false;
    float* v_z = nullptr;         // what the depth and distortion terms leave for the v_z scatter behind K18
    const float* v_n = nullptr;   // ... and the normal term for the Vn scatter
    const float* v_f = nullptr;   // ... and the feature term for the copy into the dense v_features
    {
        ProfScope ps(ctx, "ZeroGradBuffers");
        // what the forward's kernels cleared on their way (K5: v_combined; K1: the train step's gradient span) is done
        const bool one_span = n > 0 && span_floats;
        // Consumed here, whichever forward this backward belongs to: the accumulator and the span are dirty from now on, and a
        // backward of ANOTHER forward (a retained one) finds nothing to trust (take_* check the generation).
        const bool vc_done = ctx->clears.take_accum(r.generation);
        const GradClears::Span span = ctx->clears.take_span(r.generation);
        row_marks = span == GradClears::ROW_MARKS;
        // (ROW_MARKS: the single-GPU train step reads only the rows K18 writes and marks — its forward cleared the marks)
        if (row_marks && !one_span) return set_error(ctx, BH_ERR_STATE, "internal: row-marked gradients without the train step's gradient span");
        const bool span_done = one_span && span != GradClears::NONE;
        if (one_span && (span_floats & 3u) == 0 && (reinterpret_cast<uintptr_t>(v_transforms) & 15u) == 0) {
            // v_combined and the exchange buffer's gradient span cleared by ONE launch (hipMemsetAsync spends two or
            // three launches on them, each ~5 us of latency beyond the bytes)
            const size_t na = vc_done ? 0 : (nvpad * 10 + 3) / 4, nb = span_done ? 0 : span_floats / 4;
            if (na + nb) {
                hipLaunchKernelGGL(zero_two_kernel, dim3(2048), dim3(256), 0, ctx->stream, reinterpret_cast<float4*>(v_combined), na,
                                   reinterpret_cast<float4*>(v_transforms), nb);
                BH_LAUNCH_CHECK(ctx, "zero_two_kernel");
            }
        } else {
            if (!vc_done) BH_HIP(ctx, hipMemsetAsync(v_combined, 0, nvpad * 10 * 4, ctx->stream));
            if (n > 0) {
                // dense outputs are zero-filled; the kernel scatters compact -> global (render_bwd.rs:123-138)
                if (one_span) {
                    BH_HIP(ctx, hipMemsetAsync(v_transforms, 0, span_floats * 4, ctx->stream));
                } else {
                    BH_HIP(ctx, hipMemsetAsync(v_transforms, 0, (size_t)n * 10 * 4, ctx->stream));
                    BH_HIP(ctx, hipMemsetAsync(v_sh_coeffs, 0, (size_t)n * C * 3 * 4, ctx->stream));
                    BH_HIP(ctx, hipMemsetAsync(v_raw_opacities, 0, (size_t)n * 4, ctx->stream));
                    BH_HIP(ctx, hipMemsetAsync(v_refine_weight, 0, (size_t)n * 4, ctx->stream));
                }
            }
        }
    }
    {
        ProfScope ps(ctx, "RasterizeBackwards", /*dominant=*/true);
        if (r.num_intersections > 0 && v_output)
            BH_TRY(launch_rasterize_backward(ctx, fs.uniforms, fs.bg, fs.flags & BH_FLAG_SMOOTH_CUTOFF,
                                             r.compact_gid_from_isect, r.tile_offsets, r.projected, r.out_img, v_output, v_combined, fs.lpt,
                                             r.tile_offsets_far, call.want_refine, &fs.jobs, nv));
        if (call.depth) BH_TRY(launch_depth_backward(ctx, fs, *call.depth, v_combined, &v_z));
        if (call.normal) BH_TRY(launch_normal_backward(ctx, fs, *call.normal, transforms, v_combined, &v_n));
        if (call.distortion) BH_TRY(launch_distortion_backward(ctx, fs, *call.distortion, v_combined, &v_z));   // (behind the depth term: it adds to a filled v_z)
        if (call.feature) BH_TRY(launch_feature_backward(ctx, fs, *call.feature, v_combined, &v_f));
    }
    {
        ProfScope ps(ctx, "ProjectBackwards");
        BH_TRY(launch_project_backward(ctx, fs.uniforms, nv, fs.flags & BH_FLAG_MIP, fs.sh_degree, transforms, sh_coeffs,
                                       raw_opacities, r.global_from_compact_gid, v_combined, v_transforms, v_sh_coeffs,
                                       v_raw_opacities, v_refine_weight, row_marks, r.projected));
        if (v_z) BH_TRY(launch_depth_vz_scatter(ctx, fs, v_z, v_transforms, row_marks, v_sh_coeffs, v_raw_opacities, v_refine_weight));
        if (v_n) BH_TRY(launch_normal_vn_scatter(ctx, fs, v_n, transforms, v_transforms, row_marks, v_sh_coeffs, v_raw_opacities, v_refine_weight));
        if (v_f) BH_TRY(launch_feature_scatter(ctx, fs, *call.feature, v_f));
    }
    if (call.v_viewmat) {   // (brush_hip_pose.h: only when asked for)
        ProfScope ps(ctx, "PoseGrad");
        BH_TRY(launch_pose_grad(ctx, fs.uniforms, nv, fs.flags & BH_FLAG_MIP, fs.sh_degree, transforms, sh_coeffs, r.global_from_compact_gid,
                                v_combined, call.v_viewmat));
    }
    if (call.v_intrinsics) {   // (brush_hip_intrinsics.h: only when asked for)
        ProfScope ps(ctx, "IntrinsicsGrad");
        BH_TRY(launch_intrinsics_grad(ctx, fs.uniforms, nv, fs.flags & BH_FLAG_MIP, transforms, r.global_from_compact_gid, v_combined, call.v_intrinsics));
    }
    return 0;
}

int find_saved_bwd_forward(bh_ctx* ctx, const BhRenderOut* saved, int not_bwd_code, const char* who, const ForwardState** fs) {
    if (!(saved->flags & BH_FLAG_BWD_INFO)) return set_error(ctx, not_bwd_code, std::string(who) + ": the saved forward was not a BH_FLAG_BWD_INFO forward");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->far_job.pending) BH_TRY(finish_far_slice(ctx, nullptr));
    for (const Retained& rt : ctx->retained)
        if (rt.fs.out.generation == saved->generation && rt.fs.out.out_img == saved->out_img) { *fs = &rt.fs; return 0; }
    if (ctx->have_forward && saved->generation == ctx->latest.out.generation && saved->out_img == ctx->latest.out.out_img) { *fs = &ctx->latest; return 0; }
    char msg[288];
    snprintf(msg, sizeof msg, "%s: forward #%llu is stale (the context's buffers now hold forward #%llu); call bh_render_retain "
                              "on a forward that must outlive the next one", who, (unsigned long long)saved->generation, (unsigned long long)ctx->generation);
    return set_error(ctx, BH_ERR_STATE, msg);
}

int backward_entry(bh_ctx* ctx, const char* who, int not_bwd_code, uint32_t required, const BhRenderOut* saved, const float* v_output, BackwardCall call) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    const std::string name(who);
    const float* v_depth = call.depth ? call.depth->v_depth : nullptr;
    const float* v_normal = call.normal ? call.normal->v_normal : nullptr;
    const float* v_distortion = call.distortion ? call.distortion->v_distortion : nullptr;
    const bool takes_normal = call.normal != nullptr;
    if (!saved || !call.v_transforms || !call.v_sh_coeffs || !call.v_raw_opacities || !call.v_refine_weight || ((required & NEED_V_OUTPUT) && !v_output) ||
        ((required & NEED_V_DEPTH) && !v_depth) || ((required & NEED_V_NORMAL) && !v_normal) || ((required & NEED_V_DISTORTION) && !v_distortion) ||
        ((required & NEED_V_VIEWMAT) && !call.v_viewmat) || ((required & NEED_V_INTRINSICS) && !call.v_intrinsics) ||
        ((required & NEED_V_FEATURES) && (!call.feature || !call.feature->features || !call.feature->v_map || !call.feature->v_features)))
        return set_error(ctx, BH_ERR_INVALID_ARG, name + ": null argument");
    // an optional cotangent the caller left out: no term, and its mode is not looked at
    if (!v_depth) call.depth = nullptr;
    if (!v_normal) call.normal = nullptr;
    if (!v_distortion) call.distortion = nullptr;
    if (call.distortion) BH_TRY(check_distortion_kind(ctx, call.distortion->kind, call.distortion->near_z, call.distortion->far_z, who));
    if (call.normal && call.normal->mode > BH_NORMAL_UNIT) return set_error(ctx, BH_ERR_INVALID_ARG, name + ": unknown normal mode");
    if (call.depth && call.depth->mode == BH_DEPTH_MEDIAN) return set_error(ctx, BH_ERR_INVALID_ARG, name + ": median depth has no gradient");
    if (call.depth && call.depth->mode > BH_DEPTH_MEDIAN) return set_error(ctx, BH_ERR_INVALID_ARG, name + ": unknown depth mode");
    if (call.feature && (call.feature->channels == 0 || call.feature->channels > BH_FEATURE_MAX_CHANNELS))
        return set_error(ctx, BH_ERR_INVALID_ARG, name + ": channels must be 1 .. 256");
    const ForwardState* fs = nullptr;
    BH_TRY(find_saved_bwd_forward(ctx, saved, not_bwd_code, who, &fs));
    if (takes_normal && fs->n > 0 && !call.transforms) return set_error(ctx, BH_ERR_INVALID_ARG, name + ": null transforms");
    return backward_impl(ctx, *fs, v_output, call);
}

// the arena slots a BhRenderOut points into (everything a retained forward must keep alive)
static const Slot kRetainSlots[RETAIN_SLOTS] = {SLOT_OUT_IMG, SLOT_VISIBLE, SLOT_MAX_RADIUS, SLOT_TILE_OFFSETS, SLOT_PROJECTED, SLOT_ISECT_GIDS_SORTED,
                                                SLOT_TILE_IDS_SORTED, SLOT_GLOBAL_FROM_COMPACT, SLOT_CUM_TILES_HIT, SLOT_ISECT_COUNTS, SLOT_DEPTHS_SORTED,
                                                SLOT_SLICE, SLOT_BWD_CKPT, SLOT_BWD_TOPLIST};

}  // namespace bh

extern "C" {

int bh_render_backward(bh_ctx* ctx, const float* v_output, const float* transforms, const float* sh_coeffs,
                       const float* raw_opacities, float* v_transforms, float* v_sh_coeffs, float* v_raw_opacities,
                       float* v_refine_weight) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!ctx->have_forward || !(ctx->latest.flags & BH_FLAG_BWD_INFO))
        return set_error(ctx, BH_ERR_STATE, "render_backward needs a preceding BH_FLAG_BWD_INFO forward on this context");
    // (the ctx's own record of that forward is the saved one: it is found again, and cannot be stale)
    BackwardCall call{transforms, sh_coeffs, raw_opacities, v_transforms, v_sh_coeffs, v_raw_opacities, v_refine_weight};
    return backward_entry(ctx, "render_backward", BH_ERR_STATE, NEED_V_OUTPUT, &ctx->latest.out, v_output, call);
}

// SplatBwdOps::{rasterize_bwd, project_bwd} take the forward's saved tensors explicitly (bwd/burn_glue.rs:62-92, 336-371): so does this.
int bh_render_backward_saved(bh_ctx* ctx, const BhRenderOut* saved, const float* v_output, const float* transforms, const float* sh_coeffs,
                             const float* raw_opacities, float* v_transforms, float* v_sh_coeffs, float* v_raw_opacities,
                             float* v_refine_weight) {
    BackwardCall call{transforms, sh_coeffs, raw_opacities, v_transforms, v_sh_coeffs, v_raw_opacities, v_refine_weight};
    return backward_entry(ctx, "render_backward_saved", BH_ERR_STATE, NEED_V_OUTPUT, saved, v_output, call);
}

int bh_render_retain(bh_ctx* ctx, const BhRenderOut* out) {
    if (!ctx || !out) return BH_ERR_INVALID_ARG;
    BH_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->far_job.pending) BH_TRY(finish_far_slice(ctx, nullptr));
    if (!ctx->have_forward || out->generation != ctx->latest.out.generation || out->out_img != ctx->latest.out.out_img || out->out_img_packed != ctx->latest.out.out_img_packed)
        return set_error(ctx, BH_ERR_STATE, "render_retain: only the context's most recent forward can be retained (and only once)");
    Retained rt;
    rt.fs = ctx->latest;
    for (int i = 0; i < RETAIN_SLOTS; ++i) {   // the blocks leave the arena: the next forward gets its own (from the pool, or hipMalloc)
        rt.blocks[i] = ctx->slots[kRetainSlots[i]];
        ctx->slots[kRetainSlots[i]] = Buffer{};
    }
    ctx->retained.push_back(rt);
    ctx->have_forward = false;    // bh_render_backward ("the last forward") has nothing to refer to until the next forward
    ctx->latest.lpt = nullptr;
    return 0;
}

int bh_render_release(bh_ctx* ctx, const BhRenderOut* out) {
    if (!ctx || !out) return BH_ERR_INVALID_ARG;
    BH_HIP(ctx, hipSetDevice(ctx->device));
    for (size_t k = 0; k < ctx->retained.size(); ++k) {
        Retained& rt = ctx->retained[k];
        if (rt.fs.out.generation != out->generation || rt.fs.out.out_img != out->out_img) continue;
        // stream order protects the blocks: whoever gets them next is queued behind the kernels that still read them
        for (int i = 0; i < RETAIN_SLOTS; ++i) {
            if (!rt.blocks[i].ptr) continue;
            Buffer& slot = ctx->slots[kRetainSlots[i]];
            if (!slot.ptr) slot = rt.blocks[i];
            else if (ctx->pool.size() < 64) ctx->pool.push_back(rt.blocks[i]);
            else { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(rt.blocks[i].ptr); }
        }
        ctx->retained.erase(ctx->retained.begin() + (long)k);
        return 0;
    }
    return set_error(ctx, BH_ERR_STATE, "render_release: this forward is not retained on this context");
}

int bh_last_render_out(bh_ctx* ctx, BhRenderOut* out) {
    if (!ctx || !out) return BH_ERR_INVALID_ARG;
    if (!ctx->have_forward) return set_error(ctx, BH_ERR_STATE, "no forward render on this context yet");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->far_job.pending) BH_TRY(finish_far_slice(ctx, nullptr));
    *out = ctx->latest.out;
    return 0;
}

int bh_last_list_counts(bh_ctx* ctx, uint32_t* near_pairs, uint32_t* far_pairs) {
    if (!ctx || !near_pairs || !far_pairs) return BH_ERR_INVALID_ARG;
    if (!ctx->have_forward) return set_error(ctx, BH_ERR_STATE, "no forward render on this context yet");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->far_job.pending) BH_TRY(finish_far_slice(ctx, nullptr));
    *near_pairs = ctx->latest.out.num_intersections;
    *far_pairs = 0u;
    if (!ctx->latest.out.tile_offsets_far) return 0;   // one slice: the exact lists
    // slice_info (SLOT_SLICE): [0] near splats  [1] near pairs  [2] tiles the near slice left unsaturated  [3] far pairs
    uint32_t info[4] = {0u, 0u, 0u, 0u};
    BH_HIP(ctx, hipMemcpyAsync(info, ctx->slots[SLOT_SLICE].ptr, sizeof info, hipMemcpyDeviceToHost, ctx->stream));
    BH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    deliver_pending_loss(ctx);
    *near_pairs = info[1];
    *far_pairs = info[2] ? info[3] : 0u;
    return 0;
}

const float* bh_last_v_combined(bh_ctx* ctx) { return ctx ? (const float*)ctx->slots[SLOT_V_COMBINED].ptr : nullptr; }

// ---- primitives ----------------------------------------------------------------
int bh_radix_argsort(bh_ctx* ctx, const uint32_t* keys, const uint32_t* vals, uint32_t n, uint32_t bits,
                     uint32_t* out_keys, uint32_t* out_vals) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (n > 0 && (!keys || !out_keys || !out_vals)) return set_error(ctx, BH_ERR_INVALID_ARG, "radix_argsort: null argument");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return radix_argsort(ctx, keys, vals, n, bits, out_keys, out_vals);
}

int bh_prefix_sum(bh_ctx* ctx, const uint32_t* in, uint32_t n, uint32_t* out) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (n > 0 && (!in || !out)) return set_error(ctx, BH_ERR_INVALID_ARG, "prefix_sum: null argument");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return prefix_sum(ctx, in, nullptr, n, out, false);
}

int bh_image_loss_forward(bh_ctx* ctx, const float* pred_chw, const uint32_t* gt_packed, uint32_t channels, uint32_t h,
                          uint32_t w, const BhLossConfig* cfg, float* loss_map) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!pred_chw || !gt_packed || !cfg || !loss_map || h == 0 || w == 0) return set_error(ctx, BH_ERR_INVALID_ARG, "image_loss_forward: bad argument");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return launch_image_loss_forward(ctx, pred_chw, gt_packed, channels, h, w, *cfg, loss_map);
}

int bh_image_loss_backward(bh_ctx* ctx, const float* pred_chw, const uint32_t* gt_packed, const float* dl_dmap,
                           uint32_t channels, uint32_t h, uint32_t w, const BhLossConfig* cfg, float* dl_dpred) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!pred_chw || !gt_packed || !dl_dmap || !cfg || !dl_dpred || h == 0 || w == 0) return set_error(ctx, BH_ERR_INVALID_ARG, "image_loss_backward: bad argument");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return launch_image_loss_backward(ctx, pred_chw, gt_packed, dl_dmap, 0.0f, channels, h, w, *cfg, dl_dpred);
}

int bh_image_loss_value_and_grad(bh_ctx* ctx, const float* img_hwc4, const uint32_t* gt_packed, uint32_t h, uint32_t w,
                                 const BhLossConfig* cfg, float alpha_weight, float* loss_out, float* v_output) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!img_hwc4 || !gt_packed || !cfg || !loss_out || !v_output || h == 0 || w == 0)
        return set_error(ctx, BH_ERR_INVALID_ARG, "image_loss_value_and_grad: bad argument");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    const size_t hw = (size_t)h * w;
    const bool alpha = alpha_weight > 0.0f;
    return launch_image_loss_fused(ctx, img_hwc4, gt_packed, h, w, *cfg, alpha, 1.0f / (float)(hw * 3), alpha ? alpha_weight / (float)hw : 0.0f,
                                   loss_out, v_output);
}

int bh_adam_step(bh_ctx* ctx, float* param, const float* grad, float* m1, float* m2, uint64_t rows, uint32_t row_len,
                 const float* col_scale, float lr, uint32_t t, int reduce_m2, float beta1, float beta2, float eps) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (rows > 0 && (!param || !grad || !m1 || !m2)) return set_error(ctx, BH_ERR_INVALID_ARG, "adam_step: null argument");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return launch_adam(ctx, param, grad, m1, m2, rows, row_len, col_scale, lr, t, reduce_m2 != 0, beta1, beta2, eps);
}

int bh_gather_stats(bh_ctx* ctx, float* refine_weight_norm, float* vis_weight, float* max_screen_size,
                    const float* refine_weight, const float* visible, const float* screen_radius, uint64_t n) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return launch_gather_stats(ctx, refine_weight_norm, vis_weight, max_screen_size, refine_weight, visible, screen_radius, n);
}

// ---- the stochastic terms of step() (device_rng.h) ----------------------------------------
void bh_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    const Philox4 r = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}

// sample_background_color (train.rs:896-908): base + U(-strength, strength)^3, clamped to [0,1]
void bh_sample_background(uint64_t seed, uint32_t step, const float base[3], float strength, float out[3]) {
    float u[3] = {0.5f, 0.5f, 0.5f};
    if (strength > 0.0f) {
        const Philox4 r = philox4x32_10(0u, step, 0u, RNG_STREAM_BACKGROUND, (uint32_t)seed, (uint32_t)(seed >> 32));
        u[0] = unit_open(r.x); u[1] = unit_open(r.y); u[2] = unit_open(r.z);
    }
    for (int k = 0; k < 3; ++k) {
        const float v = strength > 0.0f ? base[k] + (2.0f * u[k] - 1.0f) * strength : base[k];
        out[k] = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
    }
}

int bh_normal_samples(bh_ctx* ctx, uint64_t seed, uint32_t step, uint64_t n, float* out) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (n > 0 && !out) return set_error(ctx, BH_ERR_INVALID_ARG, "normal_samples: null argument");
    if (n > 0xFFFFFFFFull) return set_error(ctx, BH_ERR_INVALID_ARG, "normal_samples: n must fit 32 bits (the splat index is one counter word)");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return launch_normal_samples(ctx, out, n, seed, step);
}

// ---- Mip-Splatting 3D filter ---------------------------------------------------------
int bh_fold_min_scale(bh_ctx* ctx, const float* transforms, const float* raw_opacities, const float* min_scale, uint32_t n,
                      float* out_transforms, float* out_raw_opacities) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (n > 0 && (!transforms || !raw_opacities || !min_scale || !out_transforms || !out_raw_opacities))
        return set_error(ctx, BH_ERR_INVALID_ARG, "fold_min_scale: null argument");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return launch_fold_min_scale(ctx, transforms, raw_opacities, min_scale, n, out_transforms, out_raw_opacities);
}

int bh_fold_min_scale_backward(bh_ctx* ctx, const float* transforms, const float* raw_opacities, const float* min_scale, uint32_t n,
                               float* v_transforms, float* v_raw_opacities) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (n > 0 && (!transforms || !raw_opacities || !min_scale || !v_transforms || !v_raw_opacities))
        return set_error(ctx, BH_ERR_INVALID_ARG, "fold_min_scale_backward: null argument");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return launch_fold_min_scale_backward(ctx, transforms, raw_opacities, min_scale, n, v_transforms, v_raw_opacities);
}

int bh_compute_min_scale(bh_ctx* ctx, const float* transforms, uint32_t n, const float* view_cams, uint32_t num_views, float factor,
                         float* out) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    // train.rs:107-109: disabled (factor <= 0) or no cameras -> there is no floor; the caller keeps min_scale = NULL
    if (!(factor > 0.0f) || num_views == 0) return set_error(ctx, BH_ERR_INVALID_ARG, "compute_min_scale: needs factor > 0 and at least one view camera");
    if (!view_cams || (n > 0 && (!transforms || !out))) return set_error(ctx, BH_ERR_INVALID_ARG, "compute_min_scale: null argument");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    return launch_compute_min_scale(ctx, transforms, n, view_cams, num_views, factor, out);
}

}  // extern "C"

extern "C" int bh_tile_sort_offsets(bh_ctx* ctx, const uint32_t* tile_ids, const uint32_t* compact_gids, uint32_t n, uint32_t num_tiles,
                                    uint32_t* tile_ids_sorted, uint32_t* compact_gids_sorted, uint32_t* tile_offsets) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!tile_offsets || (n > 0 && (!tile_ids || !compact_gids || !tile_ids_sorted || !compact_gids_sorted)))
        return set_error(ctx, BH_ERR_INVALID_ARG, "tile_sort_offsets: null argument");
    if (num_tiles == 0) return set_error(ctx, BH_ERR_INVALID_ARG, "tile_sort_offsets: num_tiles == 0");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t bits = 0;
    while (bits < 32 && (num_tiles >> bits) != 0) bits++;  // render.rs:228
    BH_HIP(ctx, hipMemsetAsync(tile_offsets, 0, (size_t)num_tiles * 2 * 4, ctx->stream));
    if (n == 0) return 0;
    if (tile_sort_supported(bits, n) && !(ctx->knob_tile_sort == 2u))
        return tile_sort_offsets(ctx, tile_ids, compact_gids, n, bits, num_tiles, tile_ids_sorted, compact_gids_sorted, tile_offsets);
    BH_TRY(radix_argsort(ctx, tile_ids, compact_gids, n, bits, tile_ids_sorted, compact_gids_sorted));
    return launch_tile_offsets(ctx, tile_ids_sorted, n, num_tiles, tile_offsets, /*pre_zeroed=*/true);
}

#ifdef BH_TEST_HOOKS
// the split counts K1 left for the context's last forward (context.h SPLIT_MAX); returns 1 and fills out[8], or 0 when that frame split nothing by construction
extern "C" int bh_debug_split_counts(bh_ctx* ctx, uint32_t* out) {
    if (!ctx || !out) return BH_ERR_INVALID_ARG;
    if (!ctx->last_split) return 0;
    BH_HIP(ctx, hipSetDevice(ctx->device));
    BH_HIP(ctx, hipMemcpyAsync(out, ctx->last_split, 8 * 4, hipMemcpyDeviceToHost, ctx->stream));
    BH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 1;
}
// depth_sort_scan (depth_sort.hip) on the caller's device buffers, without the counter readback, and the ctx stream synchronised behind
// it.  keys / counts [n], minmax [2 * COUNTER_SLOTS] in K1's format (max key | max ~key per slot, zeros neutral), out_keys / out_vals /
// cum [n]; spl: a device table of DSORT_SPL_STRIDE words or NULL (the ctx's own); *spl_written: the host's note for that table, in and
// out (spl == NULL: out only, the ctx's note, and may be NULL); totals_out [512] (host): the digit totals of keys | of tile counts the LAST launch set left at the head
// of SLOT_SORT_HIST.
extern "C" int bh_debug_depth_sort(bh_ctx* ctx, const uint32_t* keys, const uint32_t* minmax, const uint32_t* counts, uint32_t n, uint32_t* out_keys, uint32_t* out_vals,
                                   uint32_t* cum, uint32_t* spl, int* spl_written, uint32_t* totals_out) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!keys || !minmax || !counts || !out_keys || !out_vals || !cum || !totals_out || (spl && !spl_written))
        return set_error(ctx, BH_ERR_INVALID_ARG, "debug_depth_sort: null argument");
    if (n == 0 || !depth_sort_supported(n)) return set_error(ctx, BH_ERR_INVALID_ARG, "debug_depth_sort: n is outside the fused sort's reach");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    bool written = spl_written ? *spl_written != 0 : false;
    BH_TRY(depth_sort_scan(ctx, keys, minmax, counts, n, out_keys, out_vals, cum, nullptr, nullptr, nullptr, 0u, nullptr, spl, spl ? &written : nullptr));
    if (spl) *spl_written = written ? 1 : 0;
    else if (spl_written) *spl_written = ctx->dsort_spl_written ? 1 : 0;
    BH_HIP(ctx, hipMemcpyAsync(totals_out, ctx->slots[SLOT_SORT_HIST].ptr, 2 * 256 * 4, hipMemcpyDeviceToHost, ctx->stream));
    BH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
// The dealing path of the depth order (depth_deal.h) on the caller's device buffers, the way a forward runs it: a stand-in for K1 deals the
// listed keys (!= 0xFFFFFFFF) by the table `spl` into buckets of `cap` slots (0: deal_capacity(n)), the one-launch depth_sort_scan follows,
// and if a bucket overflowed the three launches run behind it.  stride: the stand-in's thread t deals element (t * stride) % n — any stride
// coprime to n deals every element once, in another arrival order.  ctr_out [256] (host): the 255 bucket words (low half: splats, high half:
// tile counts) | the overflow word; *fell_back: the three launches ran.  spl must be a table a frame has written.
__global__ __launch_bounds__(256) void debug_deal_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ counts, uint32_t n, uint32_t stride, bh::DealArgs d) {
    __shared__ uint32_t s_spl[bh::DEAL_SPL_WORDS];
    bh::deal_stage(d, s_spl);
    __syncthreads();
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    const uint32_t e = (uint32_t)(((unsigned long long)t * stride) % n);
    const uint32_t key = keys[e];
    if (key != 0xFFFFFFFFu) bh::deal_put(d, bh::deal_take(d, s_spl, key, counts[e]), key, e);
}
extern "C" int bh_debug_depth_deal(bh_ctx* ctx, const uint32_t* keys, const uint32_t* minmax, const uint32_t* counts, uint32_t n, uint32_t* out_keys, uint32_t* out_vals,
                                   uint32_t* cum, uint32_t* spl, uint32_t cap, uint32_t stride, unsigned long long* ctr_out, int* fell_back) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!keys || !minmax || !counts || !out_keys || !out_vals || !cum || !spl || !ctr_out || !fell_back || stride == 0u)
        return set_error(ctx, BH_ERR_INVALID_ARG, "debug_depth_deal: bad argument");
    if (n == 0 || !depth_sort_supported(n)) return set_error(ctx, BH_ERR_INVALID_ARG, "debug_depth_deal: n is outside the fused sort's reach");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    DealArgs d;
    d.spl = spl;
    d.cap = cap ? cap : deal_capacity(n);
    d.region = (uint2*)ensure(ctx, SLOT_DEAL_REGION, (size_t)DEAL_BUCKETS * d.cap * sizeof(uint2));
    if (!d.region) return BH_ERR_OOM;
    if (hipMalloc((void**)&d.ctr, (size_t)DEAL_SET_U64 * 8) != hipSuccess) { (void)hipGetLastError(); return BH_ERR_OOM; }
    int rc = check_hip(ctx, hipMemsetAsync(d.ctr, 0, (size_t)DEAL_SET_U64 * 8, ctx->stream), "debug_depth_deal: clear");
    if (rc == 0) {
        hipLaunchKernelGGL(debug_deal_kernel, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, keys, counts, n, stride, d);
        rc = check_hip(ctx, hipGetLastError(), "debug_deal_kernel");
    }
    bool written = true;
    if (rc == 0) rc = depth_sort_scan(ctx, keys, minmax, counts, n, out_keys, out_vals, cum, nullptr, nullptr, nullptr, 0u, nullptr, spl, &written, &d);
    unsigned long long host[DEAL_BUCKETS + 1u];
    if (rc == 0) rc = check_hip(ctx, hipMemcpy2DAsync(host, 8, d.ctr, (size_t)DEAL_LINE_U64 * 8, 8, DEAL_BUCKETS + 1u, hipMemcpyDeviceToHost, ctx->stream), "debug_depth_deal: counters");
    if (rc == 0) rc = check_hip(ctx, hipStreamSynchronize(ctx->stream), "debug_depth_deal: sync");
    if (rc == 0) {
        for (uint32_t i = 0; i <= DEAL_BUCKETS; ++i) ctr_out[i] = host[i];
        *fell_back = host[DEAL_BUCKETS] != 0ull ? 1 : 0;
        if (*fell_back) {
            ctx->deal_fallbacks++;
            rc = depth_sort_scan(ctx, keys, minmax, counts, n, out_keys, out_vals, cum, nullptr, nullptr, nullptr, 0u, nullptr, spl, &written);
            if (rc == 0) rc = check_hip(ctx, hipStreamSynchronize(ctx->stream), "debug_depth_deal: sync");
        }
    } else {
        (void)hipStreamSynchronize(ctx->stream);
    }
    (void)hipFree(d.ctr);
    return rc;
}
// slots per bucket for every later forward of this ctx whose K1 deals, instead of deal_capacity(n) (0: back to it): a real frame's
// overflow recovery — the bucket launch that does nothing, the speculative K5 that hears "nothing listed", the three launches and K5
// queued again — is reached with a small scene
extern "C" int bh_debug_set_deal_capacity(bh_ctx* ctx, uint32_t cap) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    ctx->deal_cap_override = cap;
    return 0;
}
// out[0]: forwards (and debug_depth_deal calls) whose depth order took the dealing path, out[1]: of those, the ones that fell back to the three launches
extern "C" int bh_debug_dsort_deal_counts(bh_ctx* ctx, uint32_t* out) {
    if (!ctx || !out) return BH_ERR_INVALID_ARG;
    out[0] = ctx->deal_frames;
    out[1] = ctx->deal_fallbacks;
    return 0;
}
// launch_image_loss_fused_window (loss_fused.hip) on the caller's device buffers, with the chain factors of bh_image_loss_value_and_grad
// (means over the WHOLE image, as the train step's strips use them), no pinned host words, and the ctx stream synchronised behind it.
// Tile rows [tile_y0, tile_y1) of 16 pixel rows; tile_y1 is clipped to the image's; loss_out [1]: the window's share of the loss;
// v_output [h, w, 4]: written in the window's pixel rows only.
extern "C" int bh_debug_image_loss_window(bh_ctx* ctx, const float* img_hwc4, const uint32_t* gt_packed, uint32_t h, uint32_t w, const BhLossConfig* cfg,
                                          float alpha_weight, uint32_t tile_y0, uint32_t tile_y1, float* loss_out, float* v_output) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!img_hwc4 || !gt_packed || !cfg || !loss_out || !v_output || h == 0 || w == 0)
        return set_error(ctx, BH_ERR_INVALID_ARG, "debug_image_loss_window: bad argument");
    if (tile_y0 >= tile_y1) return set_error(ctx, BH_ERR_INVALID_ARG, "debug_image_loss_window: empty tile-row window");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    const size_t hw = (size_t)h * w;
    const bool alpha = alpha_weight > 0.0f;
    // (a window that starts behind the last tile row is the launcher's to refuse: it clips tile_y1 first)
    BH_TRY(launch_image_loss_fused_window(ctx, img_hwc4, gt_packed, h, w, *cfg, alpha, 1.0f / (float)(hw * 3), alpha ? alpha_weight / (float)hw : 0.0f, tile_y0,
                                          tile_y1, loss_out, v_output, nullptr, nullptr, 0u));
    BH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
#endif
