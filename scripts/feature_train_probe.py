"""Developer tool (GPU box): what the feature term of the train step (include/brush_hip_feature_train.h) costs at
brush_amd/synth.py's 1 M splats / 1080p workload (the headline scene, SH degree 0) with a field of --channels channels (default 16)
and the L1 loss.  Prints one JSON line:
  * step_ms_plain / step_ms_term: device time of a whole SplatTrainer.step without and with the term (the same trainer, the term
    switched by TrainConfig.feature_loss_weight), medians of `--rounds` rounds of `--reps` steps each, the two alternated in a round;
  * stages: per profiled stage of the step (Context.profile) the mean ms per step without and with the term and their difference.
    The term's own stages: FeatureTerm = gather + blend + fused loss; RasterizeBackwards grows by the clear of v_features and of
    the compact V and by the term's replay; ProjectBackwards by the scatter into the dense v_features; OptimizerStep by the
    field's Adam pass over three [N,C] tables;
  * carry_ms: bh_refine_carry_rows of one [N,C] table through a plan of the same state (the refine the stats of the steps above
    ask for), and the rows it pruned / added.
    python scripts/feature_train_probe.py [--reps 5] [--rounds 5] [--channels 16]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import brush_amd as ba   # noqa: E402
from brush_amd import _ffi, host, synth   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--channels", type=int, default=16)
    args = ap.parse_args()
    ch = args.channels
    torch.cuda.set_device(0)
    ctx = ba.Context(torch.device("cuda:0"))
    sc, w, h = synth.config_scene("1m_1080p", sh_degree=0)
    splats = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device="cuda")
    n = splats.num_splats()
    cp = synth.default_camera_params(w, h)
    cam = ba.Camera(position=cp["pos"], rotation=cp["rot_xyzw"], fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
    gt = torch.from_numpy(np.ascontiguousarray(synth.synthetic_gt_packed(w, h)).view(np.int32)).cuda()
    gen = torch.Generator(device="cuda").manual_seed(5)
    field = ba.FeatureField(n, ch, lr=1e-3, device="cuda", ctx=ctx)
    field.features.copy_(torch.randn((n, ch), generator=gen, device="cuda") * 0.5)
    target = torch.randn((h, w, ch), generator=gen, device="cuda")
    cfg = ba.TrainConfig()
    tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx, feature_field=field)
    batch = ba.SceneBatch(gt, cam, view_id=1, features=target)

    def steps(weight, reps):
        cfg.feature_loss_weight = weight
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            tr.step(batch, splats)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    for wgt in (0.0, 1.0, 0.0, 1.0):   # warm-up: the view's cuts, every slot's allocation
        steps(wgt, 3)
    times = {0.0: [], 1.0: []}
    for _ in range(args.rounds):
        for wgt in times:
            times[wgt].append(steps(wgt, args.reps))
    stages = {}
    ctx.profile(True)
    for wgt in (0.0, 1.0):
        ctx.profile_fetch()
        steps(wgt, args.reps)
        stages[wgt] = {k: ms / args.reps for k, (ms, _calls) in ctx.profile_fetch().items()}
    ctx.profile(False)
    rows = {k: dict(plain_ms=round(stages[0.0].get(k, 0.0), 4), term_ms=round(stages[1.0].get(k, 0.0), 4),
                    added_ms=round(stages[1.0].get(k, 0.0) - stages[0.0].get(k, 0.0), 4)) for k in sorted(set(stages[0.0]) | set(stages[1.0]))}
    # the carry: one [N,C] table through the plan the steps' statistics ask for
    st_in = tr._train_state(splats, tr.state)
    rc = _ffi.BhRefineConfig()
    c = tr.config
    rc.iter, rc.total_train_iters, rc.growth_stop_iter, rc.max_splats = tr.step_count, c.total_train_iters, c.growth_stop_iter, c.max_splats
    rc.growth_grad_threshold, rc.growth_select_fraction, rc.split_at_screen_size, rc.opac_decay = c.growth_grad_threshold, c.growth_select_fraction, c.split_at_screen_size, c.opac_decay
    center, extent = ba.splat_bounds(splats, ctx=ctx)
    for k in range(3):
        rc.bounds_center[k], rc.bounds_extent[k] = center[k], extent[k]
    rc.seed = 1
    rs = _ffi.BhRefineStats()
    ctx.check(ctx.lib.bh_refine_plan(ctx._h, C.byref(rc), C.byref(st_in), C.byref(rs)))
    out = torch.empty((rs.total_splats, ch), dtype=torch.float32, device="cuda")
    carry = []
    for mode in (_ffi.CARRY_COPY, _ffi.CARRY_ZERO_SPLIT):
        ctx.lib.bh_refine_carry_rows(ctx._h, host._ptr(field.features), host._ptr(out), ch, mode)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            ctx.check(ctx.lib.bh_refine_carry_rows(ctx._h, host._ptr(field.features), host._ptr(out), ch, mode))
        e1.record()
        torch.cuda.synchronize()
        carry.append(round(e0.elapsed_time(e1) / args.reps, 4))
    res = dict(n=n, w=w, h=h, channels=ch, step_ms_plain=round(float(np.median(times[0.0])), 4), step_ms_term=round(float(np.median(times[1.0])), 4),
               step_ms_plain_range=[round(min(times[0.0]), 4), round(max(times[0.0]), 4)], step_ms_term_range=[round(min(times[1.0]), 4), round(max(times[1.0]), 4)],
               stages=rows, carry_ms=dict(copy=carry[0], zero_split=carry[1]), carry_rows=dict(pruned=rs.num_pruned, added=rs.num_added, total=rs.total_splats))
    print(json.dumps(res), flush=True)
    ctx.sync()
    ctx.close()


if __name__ == "__main__":
    main()
