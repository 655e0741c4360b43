"""Developer tool (GPU box): what an environment map (include/brush_hip_envmap.h) costs at 1080p.
Prints one JSON line:
  * per resolution R (64, 256) and per frame — "scene": brush_amd/synth.py's 1 M splats rendered on black, "empty": alpha 0 everywhere,
    where every pixel contributes and a texel of R = 64 takes ~2000 of them (maximal contention) —
    copy_us / composite_us / backward_us: a device copy of the same [H,W,4] f32 bytes, EnvironmentMap.composite and
    EnvironmentMap.backward(update=True) (the max pass, the tile kernel and the final kernel together, and the entry point's 4-byte
    readback) on a 1920x1080 frame (device events, medians of `--rounds` rounds of `--reps` calls each, the three alternated inside a
    round, with the spread of the rounds), the two ratios to the copy, and
    atomics: the 64-bit global atomics one backward issues, counted on the host from the restatement's taps (distinct texels per
    16 x 16 tile times three channels: an upper bound, sums of zero are skipped), beside the contributions one atomic each would cost;
  * step_ms / step_envmap_ms: SplatTrainer.step at the 1 M splats / 1080p workload without and with a map of R = 64 (wall clock over
    `--steps` steps, the two trainers alternated in blocks of `--block` steps inside one process).
Kernel times (envmap_composite_kernel, envmap_max_kernel, envmap_backward_kernel, envmap_final_kernel) come from a separate trace:
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/envmap_probe.py --trace
    python scripts/envmap_probe.py [--reps 50] [--rounds 7] [--steps 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import brush_amd as ba   # noqa: E402
from brush_amd import synth   # noqa: E402
import envmap_ref as vr   # noqa: E402


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


_TAPS = {}


def count_atomics(cam_u, alpha, res, tile=16):
    """(global atomics of one backward: distinct (tile, texel) pairs among the contributing pixels x 3, contributions x 3)."""
    h, w = alpha.shape
    if res not in _TAPS:
        ref_cam = dict(vm=np.array(list(cam_u.vm), np.float32), fx=np.float32(cam_u.fx), fy=np.float32(cam_u.fy), cx=np.float32(cam_u.cx),
                       cy=np.float32(cam_u.cy))
        _TAPS[res] = vr.taps(ref_cam, h, w, res)[0]
    texel = _TAPS[res]
    yy, xx = np.mgrid[0:h, 0:w]
    tiles = ((yy // tile) * ((w + tile - 1) // tile) + xx // tile).astype(np.int64)
    on = alpha != 1.0
    keys = (tiles[on][:, None] * (6 * res * res) + texel[on]).reshape(-1)
    return int(np.unique(keys).size) * 3, int(keys.size) * 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--block", type=int, default=25)
    ap.add_argument("--trace", action="store_true", help="the kernels only, few reps (for a rocprofv3 run)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = ba.Context(torch.device("cuda:0"))
    sc, w, h = synth.config_scene("1m_1080p", sh_degree=0)
    cp = synth.default_camera_params(w, h)
    cam = ba.Camera(position=cp["pos"], rotation=cp["rot_xyzw"], fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
    cam_u = cam.uniforms((w, h))
    rng = np.random.default_rng(3)
    spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device="cuda")
    scene_frame, _ = ba.render_splats(spl, cam, (w, h), (0.0, 0.0, 0.0), ba.RasterPass.Backward, ctx=ctx)
    frames = {"scene": scene_frame, "empty": torch.zeros_like(scene_frame)}
    v = torch.from_numpy((rng.uniform(-1.0, 1.0, (h, w, 4)) / (h * w)).astype(np.float32)).cuda()
    y, v_img = torch.empty_like(v), torch.empty_like(v)
    reps, rounds = (20, 2) if args.trace else (args.reps, args.rounds)
    res = dict(w=w, h=h, sky_share_scene=round(float((scene_frame[..., 3] < 0.5).float().mean()), 3))
    for r in (64, 256):
        env = ba.EnvironmentMap(r, lr=1e-4, ctx=ctx)
        env.params = rng.uniform(0.2, 0.8, (6, r, r, 3)).astype(np.float32)
        for name, x in frames.items():
            cands = {"copy_us": lambda: y.copy_(x), "composite_us": lambda: env.composite(x, cam_u, out=y),
                     "backward_us": lambda: env.backward(x, cam_u, v, update=True, out=v_img)}
            times = {k: [] for k in cands}
            for fn in cands.values():
                fn()
            torch.cuda.synchronize()
            for _ in range(rounds):
                for k, fn in cands.items():
                    times[k].append(timed(fn, reps))
            row = {k: round(float(np.median(t)) * 1e3, 2) for k, t in times.items()}
            row.update({k + "_min_max": [round(min(t) * 1e3, 2), round(max(t) * 1e3, 2)] for k, t in times.items()})
            row["composite_over_copy"] = round(row["composite_us"] / row["copy_us"], 3)
            row["backward_over_copy"] = round(row["backward_us"] / row["copy_us"], 3)
            if not args.trace:
                row["atomics"], row["contributions"] = count_atomics(cam_u, x[..., 3].cpu().numpy(), r)
            res["R%d_%s" % (r, name)] = row
        env.close()
    if not args.trace:
        gt = torch.from_numpy(np.ascontiguousarray(synth.synthetic_gt_packed(w, h)).view(np.int32)).cuda()
        batch = ba.SceneBatch(gt, cam, view_id=1)
        runs = {}
        for key, env in (("step_ms", None), ("step_envmap_ms", ba.EnvironmentMap(64, lr=1e-4, ctx=ctx))):
            s = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device="cuda")
            runs[key] = (ba.SplatTrainer(ba.TrainConfig(), ctx=ctx, envmap=env), s, [])
            for _ in range(20):
                runs[key][0].step(batch, s)
        ctx.sync()
        for _ in range(max(1, args.steps // args.block)):
            for key, (tr, s, ts) in runs.items():
                t0 = time.perf_counter()
                for _ in range(args.block):
                    tr.step(batch, s)
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
