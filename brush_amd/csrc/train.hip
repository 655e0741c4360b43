// brush_hip: the train step (bh_train_step).  plan_step reads the arguments and the ctx's attached terms (context.h StepTerms) ONCE,
// before anything is queued: it issues every refusal of the step and leaves a StepPlan; train_step_impl then runs the step's phases
// over that plan, in order.  A new term: a field of StepTerms with its accessor and setter, its refusals and its flag in plan_step, its
// launches in the phase where its value is known (step_image_loss for what acts on the image, step_map_terms for what joins the backward).
#include <cmath>
#include <string>

#include "context.h"
#include "param_table.h"

using namespace bh;

namespace {

// bh_train_step's arguments, as the phases pass them on
struct StepArgs {
    const BhTrainConfig* cfg;
    BhTrainState* st;
    const BhTrainBatch* batch;
    bh_grad_hook hook;
    void* hook_user;
    float grad_scale;
    BhTrainStats* stats;
};

// What a step does, decided before anything is queued
struct StepPlan {
    // the terms that count this step (StepTerms' accessors); a table is its own flag
    bool lpips = false, depth = false, normal = false, distortion = false, feature = false;
    bh_exposure* exposure = nullptr;
    bh_bilagrid* bilagrid = nullptr;
    bh_envmap* envmap = nullptr;
    // the camera's tile-row window, and whether this rank has the whole frame to itself: every term but the image loss needs that
    uint32_t tile_y0 = 0, tile_y1 = 0;
    bool whole_frame = true, window_partial = false;
    // one frame split over the ranks by strips of tile rows: the caller's image hook moves the strips / halos, or — no hook, a
    // communicator on the ctx, a proper tile-row window in the camera — the library exchanges the halos itself (comm.hip)
    bool native_tiles = false, tile_mode = false;
    bool exchanging = false;     // somebody but this step's own update reads the gradients: the caller's hook or the library's communicator
    bool keyed = false;          // ... and only the rows of splats some rank saw travel (exchange.hip)
    bool masked_grads = false;   // nobody else reads them: K18 marks the rows it writes instead of the span being zero-filled
    uint32_t n = 0, C = 0, W = 0, H = 0;
    uint32_t step = 0;           // train.rs:183 — committed to `st` only once the update is queued: a step that fails half-way (OOM, hook /
                                 // RCCL error) applied no update, so Adam's t and the lr_mean schedule must not have advanced for the retry
    // the exchange buffer: visible[N] | v_transforms[10N] | v_sh[3CN] | v_raw_opac[N] | v_refine[N], every section starting on a
    // 16-byte boundary (padded to a multiple of 4 floats; the padding stays zero) so the update kernel can move it with 128-bit
    // accesses whatever N is.  One buffer = one collective per step for a multi-GPU caller.
    size_t o_tr = 0, o_sh = 0, o_op = 0, o_ref = 0, exch_count = 0;
};

// What the phases hand to one another
struct StepWork {
    float* exch = nullptr;        // the exchange buffer (SLOT_GRADS); the visible flags are its first section
    float* s_radius = nullptr;
    const float* r_transforms = nullptr;   // the parameters the frame is rendered from: the state's, or their fold with min_scale
    const float* r_raw_opac = nullptr;
    BhRenderOut ro{};
    float* v_output = nullptr;    // dL/dimg [H,W,4]
    float* loss_dev = nullptr;
    float* loss_host = nullptr;   // the loss scalar goes straight into pinned host memory (bh_sync hands it to stats->loss): no copy launch
    float* composited = nullptr;  // with an environment map the frame over the map lives in a slot of its own too: the loss, LPIPS and the colour tables read it
    float* corrected = nullptr;   // with an exposure or a bilateral-grid table the loss reads the exposed / sliced frame from a slot of its own: out_img is what K17 replays from
    BackwardCall bwd;
    DepthTerm depth_term;
    NormalTerm normal_term;
    DistortionTerm distortion_term;
    FeatureTerm feature_term;
    float* v_features = nullptr;
    uint32_t* union_idx = nullptr;
    bool flags_on_side = false;
    float* visible() const { return exch; }
    // what the image terms see of the frame: the rasterizer's image, or that image over the environment map
    float* frame() const { return composited ? composited : ro.out_img; }
};

// the image loss of one attempt: queue_loss runs once, or twice when a far slice had to follow
struct LossCall {
    BhLossConfig lc{};
    bool alpha_match = false;
    float dl_rgb = 0.0f, dl_alpha = 0.0f;
};

// the two families of refusals a term of the step can meet, by the term's noun
int refuse_partial_frame(bh_ctx* ctx, const char* term) {
    return set_error(ctx, BH_ERR_INVALID_ARG, std::string("train_step: the ") + term + " needs the whole frame on this rank (no tile-row partition)");
}
int refuse_with_pose_grad(bh_ctx* ctx, const char* a_term, const char* the_term) {
    return set_error(ctx, BH_ERR_INVALID_ARG, std::string("train_step: ") + a_term + " and a pose-gradient buffer cannot be attached together (the pose pass does not carry the " +
                                                  the_term + "'s gradient)");
}
// (brush_hip_intrinsics.h: the intrinsics pass carries every term but these two, the environment map and the normal term)
int refuse_with_intrinsics_grad(bh_ctx* ctx, const char* a_term, const char* why) {
    return set_error(ctx, BH_ERR_STATE, std::string("train_step: ") + a_term + " and an intrinsics-gradient buffer cannot be attached together (" + why + ")");
}
// ... in the order every map term meets them (`a_term` NULL: the term has no pose rule)
int check_frame_and_pose(bh_ctx* ctx, const StepPlan& p, const char* the_term, const char* a_term) {
    if (!p.whole_frame) return refuse_partial_frame(ctx, the_term);
    if (a_term && ctx->terms.pose_grad) return refuse_with_pose_grad(ctx, a_term, the_term);
    return 0;
}

// Every refusal of the step, in this order: null arguments, exposure, bilagrid, environment map (camera, frame, pose, intrinsics, alpha), depth (map, size, kind, frame, pose), normal (camera,
// frame, pose, intrinsics), distortion, feature (frame, pose, rows, size), strip_loss, LPIPS.  Nothing is queued, no device is touched.
int plan_step(bh_ctx* ctx, const BhTrainConfig* cfg, const BhTrainState* st, const BhTrainBatch* batch, bh_grad_hook hook, const BhTrainStats* stats, StepPlan* plan) {
    if (!cfg || !st || !batch || !stats) return set_error(ctx, BH_ERR_INVALID_ARG, "train_step: null argument");
    if (!st->transforms || !st->sh_coeffs || !st->raw_opacities || !st->m1_transforms || !st->m2_transforms || !st->m1_sh ||
        !st->m2_sh || !st->m1_opac || !st->m2_opac || !st->refine_weight_norm || !st->vis_weight || !st->max_screen_size ||
        !batch->gt_packed)
        return set_error(ctx, BH_ERR_INVALID_ARG, "train_step: null state tensor");
    StepPlan& p = *plan;
    const StepTerms& t = ctx->terms;
    const BhCamera& cam = batch->camera;
    const ViewUniforms win_u = make_uniforms(cam);
    p.tile_y0 = win_u.tile_y0;
    p.tile_y1 = win_u.tile_y1;
    p.window_partial = win_u.tile_y0 != 0u || win_u.tile_y1 != win_u.tile_bh;
    p.whole_frame = !batch->image_hook && !p.window_partial;
    // an exposure table (brush_hip_exposure.h): the batch's view names the row
    if ((p.exposure = t.exposure)) {
        if (batch->view_id == 0u || batch->view_id > p.exposure->n_views)
            return set_error(ctx, BH_ERR_INVALID_ARG, "train_step: with an exposure table the batch's view_id must be 1 .. n_views");
        BH_TRY(check_frame_and_pose(ctx, p, "exposure term", nullptr));
    }
    // a bilateral-grid table (brush_hip_bilagrid.h): the exposure table's rules, and the two are alternatives
    if ((p.bilagrid = t.bilagrid)) {
        if (p.exposure)
            return set_error(ctx, BH_ERR_INVALID_ARG, "train_step: an exposure table and a bilateral-grid table cannot be attached together (they are alternatives: detach one)");
        if (batch->view_id == 0u || batch->view_id > p.bilagrid->n_views)
            return set_error(ctx, BH_ERR_INVALID_ARG, "train_step: with a bilateral-grid table the batch's view_id must be 1 .. n_views");
        BH_TRY(check_frame_and_pose(ctx, p, "bilateral-grid term", nullptr));
        if ((uint64_t)cam.img_w * cam.img_h > 0x7FFFFFFFull)
            return set_error(ctx, BH_ERR_INVALID_ARG, "train_step: with a bilateral-grid table h * w must stay below 2^31");
    }
    // an environment map (brush_hip_envmap.h): rays exist for a pinhole alone, the pose pass does not carry the lookup's dependence on
    // the rotation, and a target with real alpha says what lies behind the splats itself
    if ((p.envmap = t.envmap)) {
        if (cam.model != BH_CAMERA_PINHOLE)
            return set_error(ctx, BH_ERR_INVALID_ARG, "train_step: the environment map needs a pinhole camera (no other model can be unprojected to a ray)");
        BH_TRY(check_frame_and_pose(ctx, p, "environment map", "an environment map"));
        if (t.intrinsics_grad) return refuse_with_intrinsics_grad(ctx, "an environment map", "the ray directions depend on the intrinsics");
        if (batch->has_alpha && !batch->alpha_is_mask)
            return set_error(ctx, BH_ERR_INVALID_ARG, "train_step: an environment map and a target with real alpha cannot be combined (a mask is fine)");
        if ((uint64_t)cam.img_w * cam.img_h > 0x7FFFFFFFull)
            return set_error(ctx, BH_ERR_INVALID_ARG, "train_step: with an environment map h * w must stay below 2^31");
    }
    // a depth target (brush_hip_depth_loss.h); weight <= 0 is no term at all
    if ((p.depth = t.depth_on())) {
        const BhDepthTarget& d = t.depth_target;
        if (!d.gt) return set_error(ctx, BH_ERR_INVALID_ARG, "train_step: the depth target has no depth map");
        if (d.h != cam.img_h || d.w != cam.img_w) return set_error(ctx, BH_ERR_INVALID_ARG, "train_step: the depth target's size differs from the camera's");
        if (d.kind > BH_DEPTH_LOSS_DISPARITY) return set_error(ctx, BH_ERR_INVALID_ARG, "train_step: unknown depth loss kind");
        BH_TRY(check_frame_and_pose(ctx, p, "depth term", "a depth target"));
    }
    // a normal-consistency term (brush_hip_normal_loss.h); weight <= 0 is no term at all
    if ((p.normal = t.normal_on())) {
        if (cam.model != BH_CAMERA_PINHOLE)
            return set_error(ctx, BH_ERR_INVALID_ARG, "train_step: the normal term needs a pinhole camera (the normals of a depth map are defined for it alone)");
        BH_TRY(check_frame_and_pose(ctx, p, "normal term", "a normal term"));
        if (t.intrinsics_grad) return refuse_with_intrinsics_grad(ctx, "a normal term", "its depth-to-normal stencil uses fx, fy");
    }
    // a distortion term (brush_hip_distortion.h): attached only with a weight > 0 and a checked kind
    if ((p.distortion = t.distortion_on())) BH_TRY(check_frame_and_pose(ctx, p, "distortion term", "a distortion term"));
    // a feature term (brush_hip_feature_train.h): no field, no target or a weight <= 0 (or not a number) is no term at all
    if ((p.feature = t.feature_on())) {
        BH_TRY(check_frame_and_pose(ctx, p, "feature term", "a feature term"));
        if (t.feature_field.n != st->n)
            return set_error(ctx, BH_ERR_INVALID_ARG, "train_step: the feature term's field has " + std::to_string(t.feature_field.n) + " rows, the state " +
                                                          std::to_string(st->n) + " splats (a refine re-rows the splats: carry the field with bh_refine_carry_rows)");
        if (t.feature_target.h != cam.img_h || t.feature_target.w != cam.img_w)
            return set_error(ctx, BH_ERR_INVALID_ARG, "train_step: the feature term's target size differs from the camera's");
    }
    // (knob_force_exchange: a one-rank communicator still walks the whole exchange path — its kernels, readback and host logic —
    // with the collectives themselves degenerate: the one-GPU measurement of what the path costs per step)
    p.exchanging = hook || (ctx->comm && (ctx->comm_world > 1 || ctx->knob_force_exchange));
    // (a one-rank communicator has no neighbours: a window without strip_loss then runs as it does without a communicator)
    p.native_tiles = !batch->image_hook && p.window_partial && ctx->comm != nullptr && !hook && (batch->strip_loss || ctx->comm_world > 1);
    if (p.native_tiles && !batch->strip_loss)
        return set_error(ctx, BH_ERR_INVALID_ARG, "train_step: a tile-row window without an image hook needs strip_loss = 1 (the library exchanges the strips' halos, not whole frames)");
    p.tile_mode = batch->image_hook != nullptr || p.native_tiles;
    if ((p.lpips = t.lpips_on()) && !p.whole_frame) return refuse_partial_frame(ctx, "LPIPS term");
    p.n = st->n;
    p.C = (st->sh_degree + 1) * (st->sh_degree + 1);
    p.W = cam.img_w;
    p.H = cam.img_h;
    p.step = st->step_count + 1;
    p.masked_grads = !p.exchanging && !p.tile_mode && !ctx->knob_zero_grads && p.n > 0;
    p.keyed = p.exchanging && batch->exchange_mode == 1 && p.n > 0;
    auto pad4 = [](size_t x) { return (x + 3) & ~(size_t)3; };
    p.o_tr = pad4(p.n);
    p.o_sh = p.o_tr + pad4((size_t)p.n * 10);
    p.o_op = p.o_sh + pad4((size_t)p.n * 3 * p.C);
    p.o_ref = p.o_op + pad4(p.n);
    p.exch_count = p.o_ref + pad4(p.n);
    return 0;
}

// "sum `cnt` floats at `ptr` over the ranks, in place": the caller's hook, or the library's communicator
int sum_over_ranks(bh_ctx* ctx, const StepArgs& a, float* ptr, uint64_t cnt) {
    if (a.hook) return a.hook(a.hook_user, ptr, cnt) == 0 ? 0 : set_error(ctx, BH_ERR_STATE, "gradient hook failed");
    return comm_allreduce(ctx, ptr, cnt, false);
}

// ---- the exchange buffer, the radius vector, and the parameters the frame is rendered from
int step_buffers(bh_ctx* ctx, const StepArgs& a, const StepPlan& p, StepWork& w) {
    const BhTrainState* st = a.st;
    w.exch = (float*)ensure(ctx, SLOT_GRADS, (p.exch_count ? p.exch_count : 4) * 4);
    w.s_radius = (float*)ensure(ctx, SLOT_STATS, (size_t)(p.n ? p.n : 1) * 4);
    if (!w.exch || !w.s_radius) return BH_ERR_OOM;
    // Mip-Splatting 3D filter: render fold_min_scale(params) (bwd/burn_glue.rs:260-270)
    w.r_transforms = st->transforms;
    w.r_raw_opac = st->raw_opacities;
    if (st->min_scale && p.n > 0) {
        ProfScope ps(ctx, "FoldMinScale");
        auto* ft = (float*)ensure(ctx, SLOT_FOLDED_TRANSFORMS, (size_t)p.n * 10 * 4);
        auto* fo = (float*)ensure(ctx, SLOT_FOLDED_RAW_OPAC, (size_t)p.n * 4);
        if (!ft || !fo) return BH_ERR_OOM;
        BH_TRY(launch_fold_min_scale(ctx, st->transforms, st->raw_opacities, st->min_scale, p.n, ft, fo));
        w.r_transforms = ft;
        w.r_raw_opac = fo;
    }
    return 0;
}

// ---- forward (train.rs:211-215); `visible` lands directly in the exchange buffer.  A tile-partitioned frame then fetches the other
// ranks' strips (not in the reference: SURVEY.md §8e)
int step_forward(bh_ctx* ctx, const StepArgs& a, const StepPlan& p, StepWork& w) {
    const BhTrainBatch* batch = a.batch;
    ForwardRequest fwd;
    fwd.cam = batch->camera;
    fwd.n = p.n; fwd.sh_degree = a.st->sh_degree;
    fwd.flags = BH_FLAG_BWD_INFO | (a.cfg->render_mip ? BH_FLAG_MIP : 0) | (a.cfg->exact_lists ? 0 : BH_FLAG_SLICED_LISTS);
    fwd.transforms = w.r_transforms; fwd.sh_coeffs = a.st->sh_coeffs; fwd.raw_opacities = w.r_raw_opac;
    fwd.bg[0] = batch->background[0]; fwd.bg[1] = batch->background[1]; fwd.bg[2] = batch->background[2];
    fwd.view_id = batch->view_id;
    fwd.visible = w.visible();
    fwd.visible_floats = p.o_tr;  // the forward clears the section incl. its padding
    fwd.max_radius = w.s_radius;
    fwd.grad_begin = w.exch + p.o_tr;       // ... and the whole gradient span (padding included): K1 does both on its way
    fwd.grad_floats = p.exch_count - p.o_tr;
    // ... unless nobody but this step's own update reads the gradients (one GPU, no hook): then only the refine-weight vector
    // (N floats, the span's last section) is cleared.  K18 writes the rows of the splats that received a gradient and marks them in
    // that vector's sign bit, the update kernel takes every unmarked row as zero — at SH degree 3 the zero-fill was most of K1's
    // HBM traffic (236 of 330 MB per step at 1 M splats).
    if (p.masked_grads) {
        fwd.grad_begin = w.exch + p.o_ref;
        fwd.grad_floats = p.exch_count - p.o_ref;
    }
    // depth-sliced lists: whether the far slice has to run is known once the near slice's blend has; a single-GPU step does not
    // wait for that — the loss kernels are queued behind the near slice first (step_image_loss) and the host reads the answer while
    // they run (a tile-partitioned frame hands the image to its hook right after the forward: there the forward waits itself)
    fwd.defer_decision = !p.tile_mode;
    BH_TRY(render_forward(ctx, fwd, &w.ro));
    if (p.tile_mode) {
        ProfScope ps(ctx, "ImageExchange");
        const uint32_t r0 = p.tile_y0 * TILE_WIDTH, r1 = p.tile_y1 * TILE_WIDTH < p.H ? p.tile_y1 * TILE_WIDTH : p.H;
        if (p.native_tiles) BH_TRY(comm_exchange_strip_halos(ctx, w.ro.out_img, p.H, p.W, r0, r1));
        else if (batch->image_hook(batch->image_hook_user, w.ro.out_img, p.H, p.W, r0, r1) != 0) return set_error(ctx, BH_ERR_STATE, "image hook failed");
    }
    return 0;
}

// fused forward + backward of the loss on the rasterizer's [H,W,4] image (loss_fused.hip)
int queue_loss(bh_ctx* ctx, const StepArgs& a, const StepPlan& p, const StepWork& w, const LossCall& l) {
    const BhTrainBatch* batch = a.batch;
    // a deferred far-slice decision without an event behind the blend: this loss kernel tells the host when it starts
    uint32_t* started_host = nullptr;
    uint32_t started_tag = 0u;
    if (ctx->far_job.pending && !ctx->far_job.gate_event_recorded && !ctx->gate_signal_queued) {
        started_host = ctx->host_counters + HOST_GATE_TAG_WORD;
        started_tag = ctx->far_job.gate_tag;
        ctx->gate_signal_queued = true;
    }
    if (p.tile_mode && batch->strip_loss) {
        // one frame over several ranks: the hook delivered only the 21-px halos; loss and dL/dimg for this rank's strip
        // (stats->loss is the strip's share of the mean: the ranks' shares add up to the frame's loss)
        return launch_image_loss_fused_window(ctx, w.ro.out_img, batch->gt_packed, p.H, p.W, l.lc, l.alpha_match, l.dl_rgb, l.dl_alpha, p.tile_y0, p.tile_y1,
                                              w.loss_dev, w.v_output, w.loss_host, started_host, started_tag);
    }
    if (p.envmap) {   // (inside queue_loss: a second attempt after a failed forecast composites the finished image again)
        ProfScope ps(ctx, "EnvMap");
        BH_TRY(launch_envmap_composite(ctx, p.envmap, batch->camera, w.ro.out_img, p.H, p.W, w.composited));
    }
    if (p.exposure) {   // (likewise; the map is part of the scene, the colour model part of the camera: it acts on the composited frame)
        ProfScope ps(ctx, "Exposure");
        BH_TRY(launch_exposure_apply(ctx, p.exposure, batch->view_id, w.frame(), p.H, p.W, w.corrected));
    }
    if (p.bilagrid) {   // (likewise)
        ProfScope ps(ctx, "Bilagrid");
        BH_TRY(launch_bilagrid_slice(ctx, p.bilagrid, batch->view_id, w.frame(), p.H, p.W, w.corrected));
    }
    return launch_image_loss_fused(ctx, w.corrected ? w.corrected : w.frame(), batch->gt_packed, p.H, p.W, l.lc, l.alpha_match, l.dl_rgb, l.dl_alpha, w.loss_dev, w.v_output,
                                   w.loss_host, started_host, started_tag);
}

// ---- loss (train.rs:227-260), with the far slice's decision behind it, and the terms that act on the image: LPIPS, the backward
// of the exposure table or the bilateral grid, and the backward of the environment map
int step_image_loss(bh_ctx* ctx, const StepArgs& a, const StepPlan& p, StepWork& w) {
    const BhTrainConfig* cfg = a.cfg;
    const BhTrainBatch* batch = a.batch;
    const bool ssim_on = cfg->ssim_weight > 0.0f;
    LossCall l;
    BhLossConfig& lc = l.lc;
    lc.l1_weight = ssim_on ? 1.0f - cfg->ssim_weight : 1.0f;
    lc.ssim_weight = ssim_on ? -cfg->ssim_weight : 0.0f;
    const bool bg_nonzero = batch->background[0] != 0.0f || batch->background[1] != 0.0f || batch->background[2] != 0.0f;
    lc.composite_bg = (batch->has_alpha && bg_nonzero) ? 1 : 0;
    lc.bg[0] = batch->background[0]; lc.bg[1] = batch->background[1]; lc.bg[2] = batch->background[2];
    lc.mask = batch->alpha_is_mask ? 1 : 0;
    l.alpha_match = batch->has_alpha && !batch->alpha_is_mask && cfg->match_alpha_weight > 0.0f;
    const size_t hw = (size_t)p.W * p.H;
    w.v_output = (float*)ensure(ctx, SLOT_V_OUTPUT, hw * 16);
    w.loss_dev = (float*)ensure(ctx, SLOT_LOSS_SCALAR, 16);
    if (!w.v_output || !w.loss_dev) return BH_ERR_OOM;
    if (p.envmap && !(w.composited = (float*)ensure(ctx, SLOT_ENVMAP_FRAME, hw * 16))) return BH_ERR_OOM;
    if ((p.exposure || p.bilagrid) && !(w.corrected = (float*)ensure(ctx, SLOT_CORRECTED, hw * 16))) return BH_ERR_OOM;
    w.loss_host = reinterpret_cast<float*>(ctx->host_counters) + HOST_LOSS_WORD;
    l.dl_rgb = 1.0f / (float)(hw * 3);
    l.dl_alpha = l.alpha_match ? cfg->match_alpha_weight / (float)hw : 0.0f;
#ifdef BH_TEST_HOOKS
    if (ctx->knob_fail_loss_at && ++ctx->train_steps_seen == ctx->knob_fail_loss_at)   // (the forward is queued, a deferred far slice may be pending)
        return set_error(ctx, BH_ERR_OOM, "train_step: injected failure between the forward and the loss (BH_TEST_FAIL_LOSS_AT)");
#endif
    if (far_job_decides_first(ctx)) {   // (a view whose forecast keeps missing: lists.hip)
        BH_TRY(finish_far_slice(ctx, nullptr));
        w.ro = ctx->latest.out;   // (a second attempt replaces the frame's outputs)
    }
    BH_TRY(queue_loss(ctx, a, p, w, l));
    if (ctx->far_job.pending) {
        // The loss above ran on the near slice's image, which is the frame's image unless some tile was left unsaturated — the
        // host finds out while it runs.  Then (rare: the near lists carry a margin over what the view needed last time)
        // the far slice is queued and the loss is evaluated again on the finished image.
        bool far_ran = false;
        BH_TRY(finish_far_slice(ctx, &far_ran));
        if (far_ran) {
            w.ro = ctx->latest.out;
            BH_TRY(queue_loss(ctx, a, p, w, l));
        }
    }
    float* const final_img = w.corrected ? w.corrected : w.frame();
    // LPIPS (train.rs:265-273): on the frame's final image, GT composited as the loss above does it; loss and dL/dimg grow in place
    // on the device (no host wait)
    if (p.lpips) BH_TRY(lpips_train_term(ctx, final_img, batch->gt_packed, p.H, p.W, lc.composite_bg ? lc.bg : nullptr, w.v_output, w.loss_dev, w.loss_host));
    // exposure backward: v_output becomes A^T v' in place (x = the frame as rendered, or over the map), the view's row takes its Adam step
    if (p.exposure) {
        ProfScope ps(ctx, "Exposure");
        BH_TRY(launch_exposure_backward(ctx, p.exposure, batch->view_id, w.frame(), w.v_output, p.H, p.W, w.v_output, /*update=*/true));
    }
    // bilateral grid: loss += tv_weight TV(grid) in f32 (no launch at weight 0), then v_output becomes v_img in place and the view's
    // grid takes its Adam step on v_g + tv_weight dTV
    if (p.bilagrid) {
        ProfScope ps(ctx, "Bilagrid");
        const float tvw = ctx->terms.bilagrid_tv_weight;
        if (tvw != 0.0f) {
            float* tv_value = bilagrid_tv_scratch(ctx);
            if (!tv_value) return BH_ERR_OOM;
            BH_TRY(launch_bilagrid_tv(ctx, p.bilagrid, batch->view_id, tv_value, tvw, w.loss_dev, w.loss_host));
        }
        BH_TRY(launch_bilagrid_backward(ctx, p.bilagrid, batch->view_id, w.frame(), w.v_output, p.H, p.W, w.v_output, tvw, /*update=*/true));
    }
    // environment map, behind the colour tables' backward: v_output's alpha takes the sky's term in place (the render backward then pulls
    // alpha down where the sky explains the pixel), v_E is left in the map and — unless it has to be summed over the ranks first
    // (step_grad_exchange, step_update) — the table takes its Adam step
    if (p.envmap) {
        ProfScope ps(ctx, "EnvMap");
        BH_TRY(launch_envmap_backward(ctx, p.envmap, batch->camera, w.ro.out_img, w.v_output, p.H, p.W, w.v_output, /*update=*/!p.exchanging, a.grad_scale,
                                      /*check_host=*/false));
    }
    return 0;
}

// ---- the terms that join the backward (w.bwd), each on the frame's final image — a second attempt with complete lists has replaced
// it, if there was one — and each adding its value to the loss in f32 behind the one before: LPIPS, depth, normal, distortion, feature.
int step_map_terms(bh_ctx* ctx, const StepArgs& a, const StepPlan& p, StepWork& w) {
    const size_t hw = (size_t)p.W * p.H;
    const bool frame_listed = ctx->latest.out.num_intersections > 0 && p.n > 0;   // (an empty frame has no valid pixel)
    // depth term (brush_hip_depth_loss.h): the expected depth is that of the state the backward replays.  E and v_depth live in a slot
    // of their own until the backward (SLOT_DEPTH is the depth backward's scratch and may move).
    // normal term (brush_hip_normal_loss.h): with the same expected-depth map (rendered once).  N and v_normal live in a slot of their
    // own too (SLOT_NORMAL is the normal backward's scratch).  The fused operator adds its v_depth to the depth loss's, or writes it
    // where there is none.
    const bool depth_on = p.depth && frame_listed;
    const bool normal_on = p.normal && frame_listed;
    if (depth_on || normal_on) {
        ProfScope ps(ctx, "DepthTerm");
        auto* e_map = (float*)ensure(ctx, SLOT_DEPTH_TERM, (hw * 2 + 4) * 4);
        if (!e_map) return BH_ERR_OOM;
        float* v_depth = e_map + hw;
        BH_TRY(launch_depth_forward(ctx, ctx->latest, BH_DEPTH_EXPECTED, e_map));
        if (depth_on) BH_TRY(launch_depth_loss(ctx, e_map, ctx->terms.depth_target, v_depth + hw, v_depth, w.loss_dev, w.loss_host));
        w.depth_term.v_depth = v_depth;
        w.depth_term.mode = BH_DEPTH_EXPECTED;
        w.bwd.depth = &w.depth_term;
        if (normal_on) {
            ProfScope pn(ctx, "NormalTerm");
            auto* n_map = (float*)ensure(ctx, SLOT_NORMAL_TERM, (hw * 6 + 4) * 4);
            if (!n_map) return BH_ERR_OOM;
            float* v_normal = n_map + hw * 3;
            BH_TRY(launch_normal_map(ctx, ctx->latest, w.r_transforms, BH_NORMAL_ACCUMULATED, n_map));
            BH_TRY(launch_normal_loss(ctx, a.batch->camera, n_map, e_map, ctx->latest.out.out_img, p.H, p.W, ctx->terms.normal_term.weight, /*accumulate_v_depth=*/depth_on,
                                      v_normal + hw * 3, v_normal, v_depth, w.loss_dev, w.loss_host));
            w.normal_term.v_normal = v_normal;
            w.normal_term.mode = BH_NORMAL_ACCUMULATED;
            w.bwd.normal = &w.normal_term;
        }
    }
    // distortion term (brush_hip_distortion.h): the moment map lives in a slot of its own until the backward, which reads it instead
    // of rendering it again; the cotangent is the constant weight / (H W), so no [H,W] map of it exists.
    if (p.distortion && frame_listed && ctx->latest.out.num_listed_splats > 0) {
        ProfScope pd(ctx, "DistortionTerm");
        auto* moments = (float*)ensure(ctx, SLOT_DISTORTION_TERM, (hw * 4 + 4) * 4);
        if (!moments) return BH_ERR_OOM;
        const BhDistortionTermConfig& dc = ctx->terms.distortion_term;
        DistortionTerm& dt = w.distortion_term;
        dt.kind = dc.kind;
        dt.near_z = dc.near_z;
        dt.far_z = dc.far_z;
        dt.gain = (float)((double)dc.weight / (double)hw);
        BH_TRY(launch_distortion_map(ctx, ctx->latest, dt, /*moments=*/true, moments));
        BH_TRY(launch_distortion_loss(ctx, moments, p.H, p.W, 4u, dc.weight, moments + hw * 4, w.loss_dev, w.loss_host));
        dt.moments = moments;
        w.bwd.distortion = &dt;
    }
    // feature term (brush_hip_feature_train.h): the map is blended ONCE: it and the compact rows behind it go to the backward, which
    // then skips its own gather and forward; the map and v_map live in a slot of their own, the dense v_features in another until the
    // field's update.  A frame that lists nothing: the map is all +0, the loss is still evaluated, the backward leaves v_features all +0.
    if (p.feature) {
        ProfScope pf(ctx, "FeatureTerm");
        const BhFeatureField& ff = ctx->terms.feature_field;
        const size_t map_floats = hw * ff.channels;
        auto* f_map = (float*)ensure(ctx, SLOT_FEATURE_TERM, (map_floats * 2 + 4) * 4);
        w.v_features = (float*)ensure(ctx, SLOT_FEATURE_GRAD, (size_t)(p.n ? p.n : 1) * ff.channels * 4);
        if (!f_map || !w.v_features) return BH_ERR_OOM;
        float* v_map = f_map + map_floats;
        float* rows = nullptr;
        BH_TRY(feature_term_rows(ctx, ctx->latest, ff.channels, &rows));
        if (frame_listed && ctx->latest.out.num_listed_splats > 0) {
            BH_TRY(launch_feature_gather(ctx, ctx->latest, ff.features, ff.channels, rows));
            BH_TRY(launch_feature_forward(ctx, ctx->latest, ff.channels, rows, f_map));
        } else {
            BH_HIP(ctx, hipMemsetAsync(f_map, 0, map_floats * 4, ctx->stream));
        }
        BH_TRY(launch_feature_loss(ctx, f_map, ctx->terms.feature_target, v_map + map_floats, v_map, w.loss_dev, w.loss_host));
        FeatureTerm& ft = w.feature_term;
        ft.features = ff.features;
        ft.channels = ff.channels;
        ft.v_map = v_map;
        ft.v_features = w.v_features;
        ft.map_acc = f_map;
        ft.compact = rows;
        w.bwd.feature = &ft;
    }
    return 0;
}

// ---- multi-GPU exchange, part 1 (mask-keyed mode, exchange.hip): the visible flags are final once the forward (incl. a far slice, if
// it had to run) is, so they are summed, the union of contributing splats is listed and its size starts travelling to the host NOW —
// the backward hides the collective's latency and the readback, and the host finds the count ready
int step_flag_exchange(bh_ctx* ctx, const StepArgs& a, const StepPlan& p, StepWork& w) {
    if (!p.keyed) return 0;
    ProfScope ps(ctx, "FlagExchange");
    const uint32_t nblk = (p.n + 4095u) / 4096u;
    auto* blocks = (uint32_t*)ensure(ctx, SLOT_EXCH_BLOCKS, ((size_t)nblk + 2) * 4);   // [nblk] block offsets, then the total
    w.union_idx = (uint32_t*)ensure(ctx, SLOT_EXCH_IDX, (size_t)p.n * 4);
    if (!blocks || !w.union_idx) return BH_ERR_OOM;   // (the compact block is sized once the union's size is known, step_grad_exchange)
    // The library's communicator runs this on its own stream: the flag sum (4 B per splat over xGMI), the union listing and the
    // count's way to the host then overlap the backward on the ctx stream instead of standing in front of it; nothing on the
    // ctx stream touches the flag section before the update, which waits for the side stream (step_grad_exchange).  (A caller's hook
    // decides its own streams.)
    w.flags_on_side = !a.hook && ctx->comm_stream != nullptr;
    hipStream_t main_stream = ctx->stream;
    if (w.flags_on_side) {
        BH_HIP(ctx, hipEventRecord(ctx->comm_ev, main_stream));
        BH_HIP(ctx, hipStreamWaitEvent(ctx->comm_stream, ctx->comm_ev, 0));
        ctx->stream = ctx->comm_stream;   // (single-threaded ctx: the launchers below take the stream from it)
    }
    int rc = sum_over_ranks(ctx, a, w.exch, (uint64_t)p.o_tr);
    if (rc == 0) rc = launch_union_index(ctx, w.visible(), p.n, blocks, blocks + nblk, w.union_idx);
    if (rc == 0) rc = check_hip(ctx, hipMemcpyAsync(reinterpret_cast<uint32_t*>(ctx->host_counters) + 8, blocks + nblk, 4, hipMemcpyDeviceToHost, ctx->stream), "flag count readback");
    if (rc == 0) rc = check_hip(ctx, hipEventRecord(ctx->readback_ev, ctx->stream), "flag count event");
    ctx->stream = main_stream;
    return rc;
}

// ---- backward (train.rs:278), into the exchange buffer's gradient sections
int step_backward(bh_ctx* ctx, const StepArgs& a, const StepPlan& p, StepWork& w) {
    const BhTrainState* st = a.st;
    float* g_tr = w.exch + p.o_tr;
    float* g_op = w.exch + p.o_op;
    // masked gradients rely on last step's row marks (sign bits of the refine-weight vector) being gone: K1 of the frame's (last)
    // forward clears the vector on its way when the span is float4-addressable (always, with the pad4 layout and hipMalloc's
    // alignment) - not an implicit invariant: if it could not, clear it here.  Decided HERE, behind every second attempt a failed
    // forecast may have caused: the record describes the forward the backward is about to replay.
    if (p.masked_grads) {
        if (ctx->clears.span != GradClears::ZEROED) BH_HIP(ctx, hipMemsetAsync(w.exch + p.o_ref, 0, (p.exch_count - p.o_ref) * sizeof(float), ctx->stream));
        ctx->clears.mark_rows();   // this step's backward runs K18 in marking mode and fills nothing
    }
    // the refine weight's one consumer stops reading it at growth_stop_iter (train.rs:589-614): from then on the blend backward
    // runs without it (refine_weight_norm stays as refine() zeroed it).  g_tr .. the end of the exchange buffer is one span
    // (padding included): one zero-fill, if the forward's K1 did not clear it.
    const bool skip_refine = a.cfg->growth_stop_iter != 0u && p.step >= a.cfg->growth_stop_iter;
    BackwardCall& bwd = w.bwd;
    bwd.transforms = w.r_transforms; bwd.sh_coeffs = st->sh_coeffs; bwd.raw_opacities = w.r_raw_opac;
    bwd.v_transforms = g_tr; bwd.v_sh_coeffs = w.exch + p.o_sh; bwd.v_raw_opacities = g_op; bwd.v_refine_weight = w.exch + p.o_ref;
    bwd.span_floats = p.exch_count - p.o_tr;
    bwd.want_refine = !skip_refine;
    bwd.v_viewmat = ctx->terms.pose_grad;
    bwd.v_intrinsics = ctx->terms.intrinsics_grad;
    BH_TRY(backward_impl(ctx, ctx->latest, w.v_output, bwd));
    if (st->min_scale && p.n > 0) {  // chain d/d(folded) -> d/d(raw) through the fold (autodiff of gaussian_splats.rs:86-111)
        ProfScope ps(ctx, "FoldMinScaleBackward");
        BH_TRY(launch_fold_min_scale_backward(ctx, st->transforms, st->raw_opacities, st->min_scale, p.n, g_tr, g_op));
    }
    return 0;
}

// ---- multi-GPU exchange, part 2 (not in the reference: SURVEY.md §8e)
int step_grad_exchange(bh_ctx* ctx, const StepArgs& a, const StepPlan& p, StepWork& w) {
    float *exch = w.exch, *g_tr = exch + p.o_tr, *g_sh = exch + p.o_sh, *g_op = exch + p.o_op;
    a.stats->exchange_rows = 0;
    if (p.exchanging) {
        ProfScope ps(ctx, "GradExchange");
        if (p.keyed) {
            // only the gradient rows of splats some rank saw (the count was requested right after the forward).  One frame
            // split over the ranks: the strips' refine weights are partial sums too and travel as one more column.
            float* g_ref = p.tile_mode ? exch + p.o_ref : nullptr;
            const uint32_t c3 = 3 * p.C, k = 11 + c3 + (p.tile_mode ? 1u : 0u);
            BH_HIP(ctx, hipEventSynchronize(ctx->readback_ev));
            if (w.flags_on_side) BH_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->readback_ev, 0));   // the union list and the summed flags are the side stream's
            const uint32_t rows = reinterpret_cast<uint32_t*>(ctx->host_counters)[8];
            if (rows == 0) {
                // no rank saw any splat: every gradient row is zero everywhere, nothing to send (same decision on all ranks)
            } else if ((uint64_t)rows * 2 <= p.n) {
                // sized by what this step sends (grow-only arena): megabytes for a view's worth of rows, not n / 2 rows up front
                auto* compact = (float*)ensure(ctx, SLOT_EXCH_COMPACT, (size_t)rows * k * 4);
                if (!compact) return BH_ERR_OOM;
                BH_TRY(launch_exchange_rows(ctx, true, w.union_idx, rows, c3, g_tr, g_sh, g_op, g_ref, compact));
                BH_TRY(sum_over_ranks(ctx, a, compact, (uint64_t)rows * k));
                BH_TRY(launch_exchange_rows(ctx, false, w.union_idx, rows, c3, g_tr, g_sh, g_op, g_ref, compact));
                a.stats->exchange_rows = rows;
            } else {
                BH_TRY(sum_over_ranks(ctx, a, g_tr, (uint64_t)((p.tile_mode ? p.exch_count : p.o_ref) - p.o_tr)));
            }
        } else if (p.tile_mode) {
            BH_TRY(sum_over_ranks(ctx, a, exch, (uint64_t)p.exch_count));
        } else {
            BH_TRY(sum_over_ranks(ctx, a, exch, (uint64_t)p.o_ref));
        }
    }
    // ... and the feature term's v_features by one more sum of the same kind: N C floats, dense (brush_hip_feature_train.h)
    if (p.feature && p.exchanging && p.n > 0) {
        ProfScope ps(ctx, "FeatureExchange");
        BH_TRY(sum_over_ranks(ctx, a, w.v_features, (uint64_t)p.n * ctx->terms.feature_field.channels));
    }
    // ... and the environment map's v_E by one more: 6 R R 3 floats (brush_hip_envmap.h)
    if (p.envmap && p.exchanging) {
        ProfScope ps(ctx, "EnvMapExchange");
        BH_TRY(sum_over_ranks(ctx, a, p.envmap->grad, p.envmap->row));
    }
    return 0;
}

// ---- refine statistics (train.rs:280-298) + optimizer (train.rs:300-381): one launch; then the step counts, and the mean noise that
// could not ride on that launch follows it
int step_update(bh_ctx* ctx, const StepArgs& a, const StepPlan& p, StepWork& w) {
    const BhTrainConfig* cfg = a.cfg;
    BhTrainState* st = a.st;
    const BhTrainBatch* batch = a.batch;
    const uint32_t n = p.n;
    const double decay = std::pow(cfg->lr_mean_end / cfg->lr_mean, 1.0 / (double)cfg->total_train_iters);
    const double lr_mean = cfg->lr_mean * std::pow(decay, (double)((int)p.step - 1)) * (double)cfg->median_scene_scale;
    // visibility-gated noise on the means (train.rs:389-416): injected samples, or drawn on the device (device_rng.h)
    const bool noise_on = cfg->mean_noise_weight > 0.0f && n > 0 && (batch->noise_samples || batch->device_noise);
    const float noise_scale = (float)lr_mean * cfg->mean_noise_weight;
    // device-drawn noise without a 3D-filter floor rides on the update launch (the gate reads the opacity that launch just wrote)
    const bool noise_fused = noise_on && !batch->noise_samples && !st->min_scale;
    {
        ProfScope ps(ctx, "OptimizerStep");
        const NoiseArgs na{batch->noise_seed, p.step, noise_scale, cfg->median_scene_scale};
        UpdateCall uc;
        uc.g_transforms = w.exch + p.o_tr; uc.g_sh = w.exch + p.o_sh; uc.g_opac = w.exch + p.o_op;
        uc.refine_weight = w.exch + p.o_ref; uc.visible = w.visible(); uc.screen_radius = w.s_radius;
        uc.gscale = a.grad_scale; uc.vis_clamp = p.tile_mode;
        for (int i = 0; i < 3; ++i) uc.tab_t[i] = (float)lr_mean;
        for (int i = 3; i < 7; ++i) uc.tab_t[i] = (float)cfg->lr_rotation;
        for (int i = 7; i < 10; ++i) uc.tab_t[i] = (float)cfg->lr_scale;
        // sh: DC at full lr, bands >= 1 scaled by 1/lr_coeffs_sh_scale
        uc.lr_sh = (float)cfg->lr_coeffs_dc; uc.sh_rest_scale = 1.0f / cfg->lr_coeffs_sh_scale; uc.lr_opac = (float)cfg->lr_opac;
        uc.t = p.step; uc.beta1 = 0.9f; uc.beta2 = 0.999f; uc.eps = 1e-15f;
        uc.noise = noise_fused ? &na : nullptr; uc.masked_rows = p.masked_grads;
        BH_TRY(launch_train_update(ctx, st, uc));
        if (p.feature && n > 0) {   // the field's Adam step on grad_scale * v_features (launch_adam's arithmetic, full second moment); no rows, no update to count
            BhFeatureField& ff = ctx->terms.feature_field;
            BH_TRY(launch_adam(ctx, ff.features, w.v_features, ff.m1, ff.m2, n, ff.channels, nullptr, ff.lr, ff.step + 1, false, ff.beta1, ff.beta2, ff.eps, a.grad_scale));
            ff.step += 1;
        }
        if (p.envmap && p.exchanging) BH_TRY(launch_envmap_adam(ctx, p.envmap, a.grad_scale));   // the map's step on grad_scale * the summed v_E
    }
    st->step_count = p.step;   // the update is queued: the step counts
    if (noise_on && !noise_fused) {
        ProfScope ps(ctx, "MeanNoise");
        // the gate reads splats.opacities() of the UPDATED parameters (train.rs:389), i.e. through the fold when a floor is set
        const float* gate_opac = st->raw_opacities;
        if (st->min_scale && n > 0) {
            auto* ft = (float*)ctx->slots[SLOT_FOLDED_TRANSFORMS].ptr;
            auto* fo = (float*)ctx->slots[SLOT_FOLDED_RAW_OPAC].ptr;
            BH_TRY(launch_fold_min_scale(ctx, st->transforms, st->raw_opacities, st->min_scale, n, ft, fo));
            gate_opac = fo;
        }
        BH_TRY(launch_mean_noise(ctx, st->transforms, gate_opac, w.visible(), batch->noise_samples, n, noise_scale, cfg->median_scene_scale,
                                 batch->noise_seed, p.step));
    }
    a.stats->num_visible = w.ro.num_visible;
    a.stats->num_intersections = w.ro.num_intersections;
    a.stats->lr_mean = lr_mean;
    // the loss kernel wrote the scalar into pinned staging (a copy into the caller's pageable struct would
    // stall the host until the whole step has run); bh_sync moves it into stats->loss
    ctx->pending_loss_dst = &a.stats->loss;
    a.stats->loss = 0.0f;
    return 0;
}

int train_step_impl(bh_ctx* ctx, const StepArgs& a) {
    StepPlan plan;
    BH_TRY(plan_step(ctx, a.cfg, a.st, a.batch, a.hook, a.stats, &plan));
    BH_HIP(ctx, hipSetDevice(ctx->device));
    StepWork work;
    BH_TRY(step_buffers(ctx, a, plan, work));
    BH_TRY(step_forward(ctx, a, plan, work));
    BH_TRY(step_image_loss(ctx, a, plan, work));
    BH_TRY(step_map_terms(ctx, a, plan, work));
    BH_TRY(step_flag_exchange(ctx, a, plan, work));
    BH_TRY(step_backward(ctx, a, plan, work));
    BH_TRY(step_grad_exchange(ctx, a, plan, work));
    return step_update(ctx, a, plan, work);
}

}  // namespace

extern "C" int bh_train_step(bh_ctx* ctx, const BhTrainConfig* cfg, BhTrainState* st, const BhTrainBatch* batch,
                             bh_grad_hook hook, void* hook_user, float grad_scale, BhTrainStats* stats) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    const int rc = train_step_impl(ctx, StepArgs{cfg, st, batch, hook, hook_user, grad_scale, stats});
    if (rc != 0) {   // (the frame is incomplete: nothing may be replayed or backpropagated from it)
        drop_far_job(ctx);
        ctx->have_forward = false;
        ctx->clears.begin_forward();
    }
    return rc;
}

#ifdef BH_TEST_HOOKS
extern "C" int bh_debug_fill_train_scratch(bh_ctx* ctx, uint32_t pattern) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    const Buffer& s = ctx->slots[SLOT_GRADS];
    if (!s.ptr || s.cap < 4) return set_error(ctx, BH_ERR_STATE, "debug_fill_train_scratch: no train step on this context yet");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    BH_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(s.ptr), (int)pattern, s.cap / 4, ctx->stream));
    return 0;
}
#endif
