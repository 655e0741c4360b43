// lists.hip — the per-tile cut-list policy of the depth-sliced forward (BH_FLAG_SLICED_LISTS, automatic mode; api.hip forward_impl
// has the whole story): which table a frame uses, when a view cuts and when it falls back to complete lists, how a failed forecast
// is scored, and the far job that finishes a sliced frame.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "context.h"

namespace bh {

// Which table a frame uses.  A caller that knows its views names them (bh_set_view_id / BhTrainBatch.view_id); one that does not
// — the reference's SplatTrainer::step receives a SceneBatch without a view index (train.rs:176, brush-dataset/src/scene.rs:138-147)
// — is keyed by the camera itself: a dataset's views are fixed cameras, and the same camera gives the same bits every time.
// Bit 63 separates the two key spaces.
static uint64_t view_key(const bh_ctx* ctx, uint32_t view_id, const BhCamera& c) {
    if (view_id != 0u || ctx->knob_no_view_hash) return (uint64_t)view_id;
    uint64_t h = 0x9E3779B97F4A7C15ull;
    auto mix = [&](uint32_t w) {   // splitmix64 finaliser over a running sum: order-sensitive, cheap, well spread
        h += (uint64_t)w + 0x9E3779B97F4A7C15ull;
        uint64_t z = h;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        h = z ^ (z >> 31);
    };
    auto bits = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
    for (int i = 0; i < 12; ++i) mix(bits(c.vm[i]));
    mix(bits(c.fx)); mix(bits(c.fy)); mix(bits(c.cx)); mix(bits(c.cy));
    mix(c.img_w); mix(c.img_h); mix(c.tile_row_begin); mix(c.tile_row_end); mix(c.model);
    if (c.model != BH_CAMERA_PINHOLE) for (int i = 0; i < 8; ++i) mix(bits(c.dist[i]));
    return h | (1ull << 63);
}

// The per-tile depth-cut table of view `key` for a (tile_bw x tile_bh) grid: created (all ZCUT_ALL = "list everything") on first
// use, re-created when the grid changes; beyond MAX_VIEW_STATES tables (or VIEW_TABLE_BYTES of them) the least recently used view
// gives its table up — to the new view when the grids match (no free, no host wait: the clears are ordered on the stream).
// touch = false: a second attempt at the frame that has just been counted (finish_far_slice): the view's gap and stamp stay
// casual = a forward-only frame keyed by its camera hash (viewer / eval renders): never more than CASUAL_VIEW_STATES such tables,
// and none at all for a camera met for the first time (returns nullptr: the frame runs in index order, nothing is allocated).
static ViewState* view_state(bh_ctx* ctx, uint64_t key, uint32_t tile_bw, uint32_t tile_bh, bool touch, bool casual) {
    const size_t words = (size_t)tile_bw * tile_bh ? (size_t)tile_bw * tile_bh : 1;
    auto it = ctx->views.find(key);
    uint32_t* recycled = nullptr;
    auto forget = [&](std::unordered_map<uint64_t, ViewState>::iterator v, bool keep_block) {
        if (ctx->far_job.view == &v->second) ctx->far_job.view = nullptr;
        if (v->second.casual && ctx->casual_views) ctx->casual_views--;
        if (keep_block) recycled = v->second.zcut;
        else {
            (void)hipStreamSynchronize(ctx->stream);   // queued kernels may still use the block
            (void)hipFree(v->second.zcut);
        }
        ctx->views.erase(v);
    };
    if (it != ctx->views.end() && (it->second.tile_bw != tile_bw || it->second.tile_bh != tile_bh)) {
        forget(it, false);
        it = ctx->views.end();
    }
    if (it == ctx->views.end()) {
        if (casual) {
            bool seen = false;
            for (uint64_t k : ctx->seen_keys) seen = seen || k == key;
            if (!seen) {   // first meeting: remember the camera, allocate nothing
                ctx->seen_keys[ctx->seen_pos++ % SEEN_KEYS] = key;
                return nullptr;
            }
            while (ctx->casual_views >= CASUAL_VIEW_STATES) {   // the least recently used casual table makes room (its block is reused when the grids match)
                auto old = ctx->views.end();
                for (auto k = ctx->views.begin(); k != ctx->views.end(); ++k)
                    if (k->second.casual && (old == ctx->views.end() || k->second.last_used < old->second.last_used)) old = k;
                if (old == ctx->views.end()) { ctx->casual_views = 0; break; }
                forget(old, recycled == nullptr && old->second.tile_bw == tile_bw && old->second.tile_bh == tile_bh);
            }
        }
        const size_t max_views = std::min(MAX_VIEW_STATES, std::max<size_t>(8, VIEW_TABLE_BYTES / ((2 * words + VIEW_SPL_WORDS) * 4)));
        while (ctx->views.size() >= max_views) {
            auto old = ctx->views.begin();
            for (auto k = ctx->views.begin(); k != ctx->views.end(); ++k)
                if (k->second.last_used < old->second.last_used) old = k;
            forget(old, recycled == nullptr && old->second.tile_bw == tile_bw && old->second.tile_bh == tile_bh);
        }
        ViewState vs;
        vs.tile_bw = tile_bw;
        vs.tile_bh = tile_bh;
        vs.casual = casual;
        // [T] depth cuts (all "everything") | [T] per-tile work of the last frame (all zero) | [VIEW_SPL_WORDS] depth-sort splitter tables (none valid)
        vs.zcut = recycled;
        if (!vs.zcut && hipMalloc((void**)&vs.zcut, (2 * words + VIEW_SPL_WORDS) * 4) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(vs.zcut), (int)ZCUT_ALL, words, ctx->stream) != hipSuccess ||
            hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(vs.zcut + words), 0, words + VIEW_SPL_WORDS, ctx->stream) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(vs.zcut);
            return nullptr;
        }
        vs.gap = (uint32_t)ctx->views.size() + 1u;   // (a new view of a dataset: it will come back after about as many frames as there are views)
        vs.last_used = ++ctx->view_clock;
        if (casual) ctx->casual_views++;
        return &ctx->views.emplace(key, vs).first->second;
    }
    if (it->second.casual && !casual) {   // a training frame adopts the table: it now counts as a dataset view
        it->second.casual = false;
        if (ctx->casual_views) ctx->casual_views--;
    }
    if (touch) {
        const uint64_t now = ++ctx->view_clock;
        it->second.gap = (uint32_t)std::min<uint64_t>(now - it->second.last_used, 1u << 20);
        it->second.last_used = now;
    }
    return &it->second;
}

ViewState* frame_view(bh_ctx* ctx, const ForwardRequest& req, uint32_t tile_bw, uint32_t tile_bh, bool casual) {
    const uint64_t vkey = view_key(ctx, req.view_id, req.cam);
    // (a forward-only frame without a view id — a viewer's moving camera, an eval render — must not mint a table per frame)
    return view_state(ctx, vkey, tile_bw, tile_bh, /*touch=*/req.allow_cut, casual && (vkey >> 63) != 0ull);
}

// (a frame with few pairs has nothing to save: the near count in K1 and an occasional second attempt cost more than listing and
//  sorting them all — 100 k splats at 512 x 512 trained 4 % slower with cuts; the view's last frame tells)
bool cut_this_frame(const bh_ctx* ctx, ViewState* vs, bool allow_cut) {
    if (!allow_cut) return false;   // (the forecast has just failed: this attempt re-seeds the table)
    if (vs->seeded && vs->exact_frames == 0u && vs->last_pairs >= ctx->cut_min_pairs) {
        // (a view whose last cut frame listed nearly everything — a scene whose tiles no longer saturate early: a converging
        //  training run ends up there, bench.py train_loop — gains nothing from its cuts and pays for them: the near count in K1,
        //  and a whole second frame whenever a forecast fails.  Such a view renders complete lists, and tries a cut again later)
        if (vs->complete_frames == 0u) return true;
        vs->complete_frames--;
    } else if (vs->exact_frames) {
        vs->exact_frames--;
    }
    return false;
}

uint32_t* view_table(const ViewState* vs) { return vs ? vs->zcut : nullptr; }

uint32_t* view_splitters(ViewState* vs, bool cut, bool** written, uint32_t** listed) {
    *written = vs ? &vs->spl_written[cut ? 1 : 0] : nullptr;
    if (listed) *listed = vs ? &vs->spl_keys[cut ? 1 : 0] : nullptr;
    return vs ? vs->zcut + 2 * (size_t)vs->tile_bw * vs->tile_bh + (cut ? DSORT_SPL_STRIDE : 0u) : nullptr;
}

uint32_t cut_margin_pct(const bh_ctx* ctx, const ViewState* vs) {
    if (ctx->knob_fixed_margin) return ctx->knob_cut_margin_pct;
    const float gap = vs && vs->gap > 2u ? (float)vs->gap : 2.0f;
    const float m = (float)ctx->knob_cut_margin_pct * ctx->margin_scale * std::pow(gap * 0.5f, ctx->ctrl_gap_exp);
    return m < 6400.0f ? (m > 10.0f ? (uint32_t)m : 10u) : 6400u;
}

uint32_t list_budget(bh_ctx* ctx, ViewState* cut_view, uint32_t near_total, uint32_t ni) {
    uint32_t budget = ni;
    const float share = ctx->slice_fraction;
    if (share > 0.0f) {   // a fixed share of the pair list (bh_set_list_slicing: tests, A/B): the slot-budget slices
        if (share < 1.0f) {
            const double b = (double)share * (double)ni;
            const uint32_t floor_b = ni < 1024u ? ni : 1024u;
            budget = b < (double)floor_b ? floor_b : (uint32_t)b;
            if (budget > ni) budget = ni;
        }
        ctx->last_slice_share = (float)((double)budget / (double)ni);
    } else if (cut_view && near_total < ni) {   // per-tile depth cuts from this view's last frame
        budget = near_total;
        const float cut_share = (float)((double)near_total / (double)ni);
        ctx->last_slice_share = cut_share;
        if (ctx->auto_exact_share > 0.0f && cut_share > ctx->auto_exact_share) cut_view->complete_frames = AUTO_EXACT_FRAMES;
    } else {
        if (cut_view && ctx->auto_exact_share > 0.0f) cut_view->complete_frames = AUTO_EXACT_FRAMES;   // (the cut removed nothing at all)
        // no history for this view yet (or its forecast keeps failing, or it cut nothing): complete lists; the blend
        // kernel seeds / refreshes the view's table
        ctx->last_slice_share = 1.0f;
    }
    return budget;
}

void view_rendered(ViewState* vs, uint32_t ni) {
    vs->seeded = true;
    vs->last_pairs = ni;
}

// Outcome of a per-tile-cut frame of `vs`: did the forecast fail for some tile (the frame was then rendered a second time with
// complete lists, which re-seeds the table)?  Every outcome moves the ctx's margin factor (x ctrl_up on a miss, x ctrl_down on a
// hit: about one miss in 200 cut frames at equilibrium).  Six misses within the view's last eight cut frames (a scene that
// changes faster than any margin) and the view's next eight frames are rendered with complete lists from the start.
static void view_outcome(bh_ctx* ctx, ViewState* vs, bool missed, bool shared_table) {
    if (!ctx->knob_fixed_margin) {
        const float s = ctx->margin_scale * (missed ? ctx->ctrl_up : ctx->ctrl_down);
        ctx->margin_scale = s < ctx->ctrl_floor ? ctx->ctrl_floor : (s > 16.0f ? 16.0f : s);
    }
    if (!vs) return;
    vs->penalty = ((vs->penalty << 1) | (missed ? 1u : 0u)) & 0xFFu;   // (the history of the last eight cut frames, one bit each)
    // (BH_NO_VIEW_HASH only: the table of view id 0 shared by every frame that names no view — alternating cameras miss on every
    //  other frame there: three misses are enough, and the table stays untrusted for longer)
    if (__builtin_popcount(vs->penalty) >= (shared_table ? 3 : 6)) {
        vs->exact_frames = shared_table ? 32u : 8u;
        vs->penalty = 0u;
    }
}

// ---- the far slice of a depth-sliced forward (see forward_impl) -------------------------------------------------------------------
// count -> emit (the scan between them folded into the emit kernel) the remaining splats into the tiles that still have live pixels, sort them behind the near list (absolute
// offsets: one array for the backward), blend from the parked state.  Every kernel is gated on the device by the number of
// unsaturated tiles, so queueing it for a frame that does not need it is correct, just ~50 us of empty launches.
int enqueue_far_slice(bh_ctx* ctx, const FarJob& j) {
    const Frame& f = j.frame;
    const uint32_t* gate = f.slice_info + 2;
    const uint32_t far_max = f.ni;   // the host's bound; the live count is slice_info[3] on the device (the emit kernel's last block)
    {
        ProfScope ps(ctx, "MapGaussiansToIntersect");
        BH_TRY(launch_map_gaussians_far(ctx, f.nv, f.u, f.proj_by_gid, f.gfc, f.projected, f.cum, f.budget, f.done_bits, gate, f.far_counts, f.far_block_totals,
                                        f.far_group_totals, f.slice_info, f.tile_ids, f.isect_gids));
    }
    {
        ProfScope ps(ctx, "TileSort");
        BH_TRY(radix_argsort_dev(ctx, f.tile_ids, f.isect_gids, far_max, f.slice_info + 3, gate, f.slice_info + 1, f.tile_bits, f.tile_ids_sorted,
                                 f.isect_gids_sorted));
    }
    {
        ProfScope ps(ctx, "GetTileOffsets");
        BH_TRY(launch_tile_offsets_dev(ctx, f.tile_ids_sorted, far_max, f.slice_info + 3, gate, f.slice_info + 1, f.num_tiles, f.tile_offsets_far));
    }
    {
        ProfScope ps(ctx, "Rasterize");
        BH_TRY(launch_rasterize(ctx, f.u, f.bg, f.bwd_info, f.smooth, f.isect_gids_sorted, f.tile_offsets_far, f.projected, f.gfc, f.out_f32, f.out_u8, f.visible,
                                f.lpt, f.class_width, /*phase=*/2, &f.rs));
    }
    ctx->far_launches++;
    return 0;
}

// A sliced forward that left the decision to the host: wait for the near pass's gate word.  Slot-budget slices: queue the far slice
// if some tile is still unsaturated.  Per-tile cuts: there is no far pass (only the splats that own a near pair were sorted) — a
// tile that is still live behind a cut list means the view's forecast failed, and the whole forward is run again with complete
// lists (which also re-seeds the view's table).  *launched (optional) tells the caller whether out_img changed after the near pass.
int finish_far_slice(bh_ctx* ctx, bool* launched) {
    if (launched) *launched = false;
    if (!ctx->far_job.pending) return 0;
    ctx->far_job.pending = false;
    if (!ctx->far_job.gate_event_recorded && ctx->gate_signal_queued) {
        // (bh_train_step: its loss kernel, queued behind the near blend, stores the job's tag when it starts)
        BH_TRY(wait_host_tag(ctx, reinterpret_cast<const volatile uint32_t*>(ctx->host_counters) + HOST_GATE_TAG_WORD, ctx->far_job.gate_tag, "near-pass gate"));
    } else {
        if (!ctx->far_job.gate_event_recorded) BH_HIP(ctx, hipEventRecord(ctx->gate_ev, ctx->stream));   // (nobody queued a signal: an event behind whatever is queued now)
        BH_HIP(ctx, hipEventSynchronize(ctx->gate_ev));
    }
    ctx->gate_signal_queued = false;
    const uint32_t unsat = reinterpret_cast<const volatile uint32_t*>(ctx->host_counters)[HOST_GATE_WORD];
    if (ctx->far_job.by_cut) {
        FarJob& j = ctx->far_job;
        view_outcome(ctx, j.view, unsat != 0u, j.view_shared);
        if (unsat == 0u) return 0;
        if (launched) *launched = true;
        ctx->far_launches++;
        // the same call again (same outputs, same view), with complete lists
        ForwardRequest again = j.req;
        again.allow_cut = false;
        again.defer_decision = false;
        BhRenderOut out;
        return forward_impl(ctx, again, &out);
    }
    ctx->far_direct = unsat != 0u;   // ... and the next sliced frame starts from what this one needed
    if (unsat == 0u) return 0;
    if (launched) *launched = true;
    return enqueue_far_slice(ctx, ctx->far_job);
}

// A view whose forecast keeps missing (two of its last eight cut frames) decides FIRST — the host waits for the near pass's blend,
// ~15 us of bubble — instead of queueing loss kernels that a second attempt would make worthless (~120 us).  One isolated miss
// does not switch: eight bubbles cost more than the one wasted loss they would insure against at a 3 % miss rate.
bool far_job_decides_first(const bh_ctx* ctx) {
    return ctx->far_job.pending && ctx->far_job.view && __builtin_popcount(ctx->far_job.view->penalty) >= 2;
}

// A step that fails behind its forward must not leave a deferred far-slice decision behind: the job holds the CALLER's parameter
// pointers (a per-tile-cut job replays the whole forward from them) and the caller is free to release or re-allocate them after a
// failed step (a refine changes n and every buffer).  Drop it; the frame it belonged to is incomplete, so nothing may be replayed
// from it either, and the view's next frame is rendered with complete lists.
void drop_far_job(bh_ctx* ctx) {
    FarJob& j = ctx->far_job;
    if (j.pending) {
        j.pending = false;
        if (j.by_cut && j.view && j.view->exact_frames == 0u) j.view->exact_frames = 1u;
    }
    j.view = nullptr;
}

}  // namespace bh
