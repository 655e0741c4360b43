"""Developer tool (GPU box): what the intrinsics gradient (include/brush_hip_intrinsics.h) costs at
brush_amd/synth.py's 1 M splats / 1080p workload (the headline scene, SH degree 0).  Prints one JSON line:
  * backward_ms / backward_pose_ms / backward_pose_intrinsics_ms / backward_intrinsics_ms: bh_render_backward_saved,
    bh_render_backward_pose_saved and bh_render_backward_intrinsics_saved with and without v_viewmat on the same forward (device
    events, medians of `--rounds` rounds of `--reps` calls each, alternated inside a round);
  * step_ms / step_attached_ms / step_optimizer_ms: SplatTrainer.step plain, with a buffer attached by
    bh_train_set_intrinsics_grad (no readback), and with an IntrinsicsOptimizer (the 16-byte readback and its synchronisation every
    step); wall clock over `--steps` steps after a warm-up, the three alternated in `--rounds` rounds, medians.
Kernel times (intrinsics_grad_kernel, intrinsics_grad_final_kernel next to pose_grad_kernel) come from a separate trace of the same
loops:
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/intrinsics_probe.py --trace
    python scripts/intrinsics_probe.py [--reps 20] [--rounds 7] [--steps 100]
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
from brush_amd.host import _ptr   # noqa: E402


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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--trace", action="store_true", help="the backwards only, few reps (for a rocprofv3 run)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = ba.Context(torch.device("cuda:0"))
    sc, w, h = synth.config_scene("1m_1080p", sh_degree=0)
    splats = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device="cuda")
    cp = synth.default_camera_params(w, h)
    cam = ba.Camera(position=cp["pos"], rotation=cp["rot_xyzw"], fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
    v_out = torch.from_numpy((np.random.default_rng(3).uniform(-1.0, 1.0, (h, w, 4)) / (h * w)).astype(np.float32)).cuda()
    node = ba.render_splats_diff(splats, cam, (w, h), ctx=ctx)
    cands = {"backward_ms": lambda: node.backward(v_out), "backward_pose_ms": lambda: node.backward(v_out, pose=True),
             "backward_pose_intrinsics_ms": lambda: node.backward(v_out, pose=True, intrinsics=True),
             "backward_intrinsics_ms": lambda: node.backward(v_out, intrinsics=True)}
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
        buf = torch.zeros(4, device="cuda")
        runs = {}
        for key, io in (("step_ms", None), ("step_attached_ms", None), ("step_optimizer_ms", ba.IntrinsicsOptimizer(lr_focal=1e-6, lr_center=1e-7))):
            runs[key] = (ba.SplatTrainer(ba.TrainConfig(), ctx=ctx, intrinsics_optimizer=io), splats.clone())
        batch = ba.SceneBatch(gt, cam, view_id=1)

        def steps(key, count):
            tr, spl = runs[key]
            attach = key == "step_attached_ms"
            if attach:
                ctx.check(ctx.lib.bh_train_set_intrinsics_grad(ctx._h, _ptr(buf)))
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(count):
                tr.step(batch, spl)
            ctx.sync()
            dt = (time.perf_counter() - t0) / count * 1e3
            if attach:
                ctx.check(ctx.lib.bh_train_set_intrinsics_grad(ctx._h, None))
            return dt

        for key in runs:
            steps(key, 20)
        step_times = {k: [] for k in runs}
        for _ in range(rounds):
            for key in runs:
                step_times[key].append(steps(key, max(1, args.steps // rounds)))
        res.update({k: round(float(np.median(v)), 4) for k, v in step_times.items()})
    print(json.dumps(res), flush=True)
    ctx.sync()
    ctx.close()


if __name__ == "__main__":
    main()
