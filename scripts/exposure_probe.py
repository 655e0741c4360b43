"""Developer tool (GPU box): what per-view exposure compensation (include/brush_hip_exposure.h) costs at 1080p.
Prints one JSON line:
  * apply_us / backward_us: ExposureTable.apply and ExposureTable.backward(update=True) (the backward kernel and the one-block
    final kernel together) on a 1920x1080 frame (device events, medians of `--rounds` rounds of `--reps` calls each, alternated
    inside a round), and the share of the HBM time of their traffic they reach (apply 66 MB, backward 100 MB at `--hbm-tbs`);
  * step_ms / step_exposure_ms: SplatTrainer.step at brush_amd/synth.py's 1 M splats / 1080p workload without and with a table
    (wall clock over `--steps` steps, the two trainers alternated in blocks of `--block` steps inside one process).
Kernel times (exposure_apply_kernel, exposure_backward_kernel, exposure_final_kernel) come from a separate trace of the same loops:
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/exposure_probe.py --trace
    python scripts/exposure_probe.py [--reps 50] [--rounds 7] [--steps 200]
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
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float32)).cuda()
    v = torch.from_numpy((rng.uniform(-1.0, 1.0, (h, w, 4)) / (h * w)).astype(np.float32)).cuda()
    y, v_img = torch.empty_like(x), torch.empty_like(x)
    tab = ba.ExposureTable(4, lr=1e-4, ctx=ctx)
    tab.set_view(2, (np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]) + rng.uniform(-0.3, 0.3, 12)).astype(np.float32))
    cands = {"apply_us": lambda: tab.apply(2, x, out=y), "backward_us": lambda: tab.backward(2, x, v, update=True, out=v_img)}
    reps, rounds = (20, 2) if args.trace else (args.reps, args.rounds)
    times = {k: [] for k in cands}
    for fn in cands.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in cands.items():
            times[k].append(timed(fn, reps))
    res = dict(w=w, h=h)
    res.update({k: round(float(np.median(t)) * 1e3, 2) for k, t in times.items()})
    px = w * h
    res["apply_hbm_share"] = round(px * 32 / (args.hbm_tbs * 1e12) / (res["apply_us"] * 1e-6), 3)
    res["backward_hbm_share"] = round(px * 48 / (args.hbm_tbs * 1e12) / (res["backward_us"] * 1e-6), 3)
    if not args.trace:
        sc, sw, sh_ = synth.config_scene("1m_1080p", sh_degree=0)
        cp = synth.default_camera_params(sw, sh_)
        cam = ba.Camera(position=cp["pos"], rotation=cp["rot_xyzw"], fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
        gt = torch.from_numpy(np.ascontiguousarray(synth.synthetic_gt_packed(sw, sh_)).view(np.int32)).cuda()
        batch = ba.SceneBatch(gt, cam, view_id=1)
        runs = {}
        for key, table in (("step_ms", None), ("step_exposure_ms", ba.ExposureTable(4, lr=1e-4, ctx=ctx))):
            spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device="cuda")
            runs[key] = (ba.SplatTrainer(ba.TrainConfig(), ctx=ctx, exposure=table), spl, [])
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
