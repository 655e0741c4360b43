"""Developer tool (GPU box): what per-view bilateral grids (include/brush_hip_bilagrid.h) cost at 1080p, next to the
exposure table on the same frame (the yardstick for a streaming pass over the same bytes).  Prints one JSON line:
  * slice_us / backward_us: BilateralGridTable.slice and BilateralGridTable.backward(tv_weight=10, update=True) (the v_g pass, the
    per-pixel pass, the final and the step kernel together) for a (16,16,8) grid on a 1920x1080 frame; exposure_apply_us /
    exposure_backward_us: ExposureTable.apply / backward(update=True) on the same frame (device events, medians of `--rounds`
    rounds of `--reps` calls each, alternated inside a round), and the share of the HBM time of their compulsory traffic they reach
    (slice 32 B per pixel, backward 48 B per pixel, at `--hbm-tbs`);
  * step_ms / step_exposure_ms / step_bilagrid_ms: SplatTrainer.step at brush_amd/synth.py's 1 M splats / 1080p workload plain, with
    an exposure table and with a grid table (wall clock over `--steps` steps, the trainers alternated in blocks of `--block` steps
    inside one process).
Kernel times (bilagrid_slice_kernel, bilagrid_vg_kernel, bilagrid_pixel_kernel, bilagrid_final_kernel, bilagrid_step_kernel) come from a
separate trace of the same loops:
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bilagrid_probe.py --trace
    python scripts/bilagrid_probe.py [--reps 50] [--rounds 7] [--steps 200]
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
    ap.add_argument("--trace", action="store_true", help="the kernels only, few reps (for a rocprofv3 run)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = ba.Context(torch.device("cuda:0"))
    w, h = 1920, 1080
    grid = (16, 16, 8)
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float32)).cuda()
    v = torch.from_numpy((rng.uniform(-1.0, 1.0, (h, w, 4)) / (h * w)).astype(np.float32)).cuda()
    y, v_img = torch.empty_like(x), torch.empty_like(x)
    tab = ba.BilateralGridTable(4, grid=grid, lr=1e-4, ctx=ctx)
    ident = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (grid[1], grid[0], grid[2], 1))
    tab.set_view(2, ident + rng.uniform(-0.3, 0.3, ident.shape).astype(np.float32))
    exp = ba.ExposureTable(4, lr=1e-4, ctx=ctx)
    exp.set_view(2, (np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]) + rng.uniform(-0.3, 0.3, 12)).astype(np.float32))
    cands = {"slice_us": lambda: tab.slice(2, x, out=y), "backward_us": lambda: tab.backward(2, x, v, tv_weight=10.0, update=True, out=v_img),
             "exposure_apply_us": lambda: exp.apply(2, x, out=y), "exposure_backward_us": lambda: exp.backward(2, x, v, update=True, out=v_img)}
    reps, rounds = (20, 2) if args.trace else (args.reps, args.rounds)
    times = {k: [] for k in cands}
    for fn in cands.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in cands.items():
            times[k].append(timed(fn, reps))
    res = dict(w=w, h=h, grid=list(grid))
    res.update({k: round(float(np.median(t)) * 1e3, 2) for k, t in times.items()})
    px = w * h
    res["slice_hbm_share"] = round(px * 32 / (args.hbm_tbs * 1e12) / (res["slice_us"] * 1e-6), 3)
    res["backward_hbm_share"] = round(px * 48 / (args.hbm_tbs * 1e12) / (res["backward_us"] * 1e-6), 3)
    if not args.trace:
        sc, sw, sh_ = synth.config_scene("1m_1080p", sh_degree=0)
        cp = synth.default_camera_params(sw, sh_)
        cam = ba.Camera(position=cp["pos"], rotation=cp["rot_xyzw"], fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
        gt = torch.from_numpy(np.ascontiguousarray(synth.synthetic_gt_packed(sw, sh_)).view(np.int32)).cuda()
        batch = ba.SceneBatch(gt, cam, view_id=1)
        runs = {}
        for key, kw in (("step_ms", {}), ("step_exposure_ms", dict(exposure=ba.ExposureTable(4, lr=1e-4, ctx=ctx))),
                        ("step_bilagrid_ms", dict(bilagrid=ba.BilateralGridTable(4, grid=grid, lr=1e-4, ctx=ctx)))):
            spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device="cuda")
            runs[key] = (ba.SplatTrainer(ba.TrainConfig(), ctx=ctx, **kw), spl, [])
            for _ in range(20):
                runs[key][0].step(batch, spl)
        ctx.sync()
        for _ in range(max(1, args.steps // args.block)):
            for key, (tr, spl, ts) in runs.items():
                t0 = time.perf_counter()
                for _ in range(args.block):
                    tr.step(batch, spl)
                ctx.sync()
                ts.append((time.perf_counter() - t0) / args.block * 1e3)
        for key, (_, _, ts) in runs.items():
            res[key] = round(float(np.median(ts)), 4)
            res[key + "_min_max"] = [round(min(ts), 4), round(max(ts), 4)]
    print(json.dumps(res), flush=True)
    ctx.sync()
    ctx.close()


if __name__ == "__main__":
    main()
