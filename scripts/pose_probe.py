"""Developer tool (GPU box): what the pose gradient (include/brush_hip_pose.h) costs at brush_amd/synth.py's 1 M
splats / 1080p workload (the headline scene, SH degree 0).  Prints one JSON line:
  * backward_ms / backward_pose_ms: bh_render_backward_saved and bh_render_backward_pose_saved on the same forward (device events,
    medians of `--rounds` rounds of `--reps` calls each, alternated inside a round);
  * step_ms / step_pose_ms: SplatTrainer.step without and with a PoseOptimizer (wall clock over `--steps` steps after a warm-up;
    the second includes the 48-byte readback and its synchronisation, every step), readback_us: that readback alone.
Kernel times (pose_grad_kernel, pose_grad_final_kernel next to project_backward_kernel) come from a separate trace of the same loops:
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/pose_probe.py --trace
    python scripts/pose_probe.py [--reps 20] [--rounds 7] [--steps 200]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--trace", action="store_true", help="the two backwards only, few reps (for a rocprofv3 run)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = ba.Context(torch.device("cuda:0"))
    sc, w, h = synth.config_scene("1m_1080p", sh_degree=0)
    splats = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device="cuda")
    cp = synth.default_camera_params(w, h)
    cam = ba.Camera(position=cp["pos"], rotation=cp["rot_xyzw"], fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
    v_out = torch.from_numpy((np.random.default_rng(3).uniform(-1.0, 1.0, (h, w, 4)) / (h * w)).astype(np.float32)).cuda()
    node = ba.render_splats_diff(splats, cam, (w, h), ctx=ctx)
    cands = {"backward_ms": lambda: node.backward(v_out), "backward_pose_ms": lambda: node.backward(v_out, pose=True)}
    reps, rounds = (3, 2) if args.trace else (args.reps, args.rounds)
    times = {k: [] for k in cands}
    for fn in cands.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in cands.items():
            times[k].append(timed(fn, reps))
    res = dict(n=splats.num_splats(), w=w, h=h, listed_splats=int(node.out.num_listed_splats))
    res.update({k: round(float(np.median(v)), 4) for k, v in times.items()})
    if not args.trace:
        gt = torch.from_numpy(np.ascontiguousarray(synth.synthetic_gt_packed(w, h)).view(np.int32)).cuda()
        for key, po in (("step_ms", None), ("step_pose_ms", ba.PoseOptimizer(lr_rotation=1e-5, lr_translation=1e-5))):
            spl = splats.clone()
            tr = ba.SplatTrainer(ba.TrainConfig(), ctx=ctx, pose_optimizer=po)
            batch = ba.SceneBatch(gt, cam, view_id=1)
            for _ in range(20):
                tr.step(batch, spl)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                tr.step(batch, spl)
            ctx.sync()
            res[key] = round((time.perf_counter() - t0) / args.steps * 1e3, 4)
        buf = torch.zeros(12, device="cuda")
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(200):
            buf.cpu()
        res["readback_us"] = round((time.perf_counter() - t0) / 200 * 1e6, 1)
    print(json.dumps(res), flush=True)
    ctx.sync()
    ctx.close()


if __name__ == "__main__":
    main()
