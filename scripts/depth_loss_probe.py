"""Developer tool (GPU box): what depth supervision (include/brush_hip_depth_loss.h) costs at 1 M splats / 1080p.
Prints one JSON line:
  * loss_us / loss_nograd_us / metrics_us: depth_loss_value_and_grad with and without v_depth (the streaming kernel and the
    one-block final kernel together) and eval_depth_metrics on the frame's expected-depth map (device events, medians of `--rounds`
    rounds of `--reps` calls each, alternated inside a round), next to the bytes they move (8 B read + 4 B written per pixel:
    24.9 MB at 1080p) and the share of that traffic's HBM time at `--hbm-tbs`;
  * step_ms / step_depth_ms: SplatTrainer.step at brush_amd/synth.py's 1 M splats / 1080p workload without and with a depth map in
    the batch (wall clock over `--steps` steps, the two trainers alternated in blocks of `--block` steps inside one process).
    python scripts/depth_loss_probe.py [--reps 50] [--rounds 7] [--steps 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import brush_amd as ba   # noqa: E402
from brush_amd import synth   # noqa: E402


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--block", type=int, default=25)
    ap.add_argument("--hbm-tbs", type=float, default=6.29, help="the HBM rate the achieved shares are quoted against, TB/s (a float4 copy reaches 6.29 of the 8.0 peak)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = ba.Context(torch.device("cuda:0"))
    sc, w, h = synth.config_scene("1m_1080p", sh_degree=0)
    cp = synth.default_camera_params(w, h)
    cam = ba.Camera(position=cp["pos"], rotation=cp["rot_xyzw"], fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
    spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device="cuda")
    e = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx).depth("expected").clone()
    ctx.sync()
    rng = np.random.default_rng(3)
    gt = (e * torch.from_numpy(rng.uniform(0.9, 1.1, (h, w)).astype(np.float32)).cuda()).contiguous()
    cands = {"loss_us": lambda: ba.depth_loss_value_and_grad(e, gt, "l1", 0.5, ctx=ctx),
             "loss_nograd_us": lambda: ba.depth_loss_value_and_grad(e, gt, "l1", 0.5, ctx=ctx, want_grad=False),
             "loss_disparity_us": lambda: ba.depth_loss_value_and_grad(e, gt, "disparity", 0.5, ctx=ctx),
             "metrics_us": lambda: ba.eval_depth_metrics(e, gt, ctx=ctx)}
    times = {k: [] for k in cands}
    for fn in cands.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, fn in cands.items():
            times[k].append(timed(fn, args.reps))
    res = dict(w=w, h=h)
    res.update({k: round(float(np.median(t)) * 1e3, 2) for k, t in times.items()})
    px = w * h
    res["loss_bytes"] = px * 12
    res["loss_hbm_share"] = round(px * 12 / (args.hbm_tbs * 1e12) / (res["loss_us"] * 1e-6), 3)
    gtp = torch.from_numpy(np.ascontiguousarray(synth.synthetic_gt_packed(w, h)).view(np.int32)).cuda()
    runs = {}
    for key, depth in (("step_ms", None), ("step_depth_ms", gt)):
        s = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device="cuda")
        batch = ba.SceneBatch(gtp, cam, view_id=1, depth=depth)
        runs[key] = (ba.SplatTrainer(ba.TrainConfig(depth_loss_weight=0.5), ctx=ctx), s, batch, [])
        for _ in range(20):
            runs[key][0].step(batch, s)
    ctx.sync()
    for _ in range(max(1, args.steps // args.block)):
        for key, (tr, s, batch, ts) in runs.items():
            t0 = time.perf_counter()
            for _ in range(args.block):
                tr.step(batch, s)
            ctx.sync()
            ts.append((time.perf_counter() - t0) / args.block * 1e3)
    for key, (_, _, _, ts) in runs.items():
        res[key] = round(float(np.median(ts)), 4)
        res[key + "_min_max"] = [round(min(ts), 4), round(max(ts), 4)]
    print(json.dumps(res), flush=True)
    ctx.sync()
    ctx.close()


if __name__ == "__main__":
    main()
