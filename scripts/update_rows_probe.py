#!/usr/bin/env python
"""How many rows of an update block (256 consecutive splats at SH degree 0) are NOT dormant, in the protocols bench.py times.
  headline: two views, the 1 M scene, the default stochastic step — sampled at steps inside the timed range of the default command
            (steps [10, 110)) and of `--steps 20 --warmup 5` (steps [5, 25));
  loop:     the converging loop of `bench.py --loop-only exact_lists --loop-steps 1500` (a teacher rendered from 64 orbit cameras,
            a perturbed student, SceneLoader, refine every 200 steps) — sampled in its late phase.
Per sample, from the state tensors in front of the step: the histogram of non-dormant rows per block (the mark is the bit pattern of
m2_sh, -0.0 = dormant) and the share of splats non-dormant; from the step itself: the share of splats whose gradient row was written.
The step's refine weight (whose sign bit is K18's mark) lives in the context's scratch and has no host accessor, so "written" is read
off the result: a row's second moment of the transforms is beta2 x its old value to the bit unless a gradient term was added.
    python scripts/update_rows_probe.py [--rows 256] [--skip-loop] [--loop-steps 1500]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def sample(tag, step, trainer, rows, do_step):
    """The marks as the next step will read them; then that step (do_step()), and which rows it wrote."""
    st = trainer.state
    n = st["m2_sh"].numel()
    live = st["m2_sh"].view(torch.int32) != -2147483648
    pad = (-n) % rows
    per_block = torch.nn.functional.pad(live.to(torch.int32), (0, pad)).view(-1, rows).sum(1)
    before = st["m2_t"].clone()
    beta2 = 0.999   # the train step's Adam (adam_scaled.rs)
    do_step()
    torch.cuda.synchronize()
    st = trainer.state
    written = None
    if st["m2_t"].shape == before.shape:
        decayed = before * torch.tensor(beta2, dtype=torch.float32, device=before.device)
        written = (st["m2_t"].view(torch.int32) != decayed.view(torch.int32)).any(1)
    pb = per_block.cpu().numpy()
    hist = np.bincount(np.minimum(pb // 8, rows // 8), minlength=rows // 8 + 1)
    q = {p: int(np.percentile(pb, p)) for p in (1, 10, 50, 90, 99)}
    rec = {"protocol": tag, "step": step, "splats": n, "rows_per_block": rows, "blocks": int(pb.size),
           "non_dormant_share": round(float(live.float().mean()), 4),
           "written_share": None if written is None else round(float(written.float().mean()), 4),
           "written_of_non_dormant": None if written is None else round(float((written & live).float().sum() / max(1.0, float(live.sum()))), 4),
           "rows_per_block_mean": round(float(pb.mean()), 2), "rows_per_block_min": int(pb.min()), "rows_per_block_max": int(pb.max()),
           "rows_per_block_percentiles": q, "blocks_at_most": {t: round(float((pb <= t).mean()), 4) for t in (25, 32, 51, 64, 76, 102, 128, 255)},
           "histogram_bins_of_8": hist.tolist()}
    print(json.dumps(rec), flush=True)
    return rec


def headline(ba, synth, dev, ctx, rows, out):
    scene, w, h = synth.config_scene("1m_1080p", 0)
    cp = synth.default_camera_params(w, h)
    batches = []
    for v in range(2):   # bench.py view_cameras: (0,0,z) and (2,0,z), identity rotation
        cam = ba.Camera(position=(cp["pos"][0] + 2.0 * v, cp["pos"][1], cp["pos"][2]), rotation=(0.0, 0.0, 0.0, 1.0), fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
        gt = torch.from_numpy(synth.synthetic_gt_packed(w, h, seed=7 + 100 * v).view(np.int32)).to(dev)
        batches.append(ba.SceneBatch(gt, cam.uniforms((w, h)), view_id=v + 1))
    splats = ba.Splats(scene["transforms"], scene["sh"], scene["raw_opac"], device=dev)
    trainer = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=5.0, ctx=ctx, seed=0xB5EED)
    at = {5: "headline --steps 20 --warmup 5", 15: "headline --steps 20 --warmup 5", 24: "headline --steps 20 --warmup 5",
          10: "headline default", 40: "headline default", 75: "headline default", 109: "headline default"}
    for s in range(110):
        step = lambda: trainer.step(batches[s % 2], splats)   # noqa: E731
        if s in at:
            out.append(sample(at[s], s, trainer, rows, step))
        else:
            step()


def loop(ba, synth, dev, ctx, rows, out, total_steps, nviews=64, refine_every=200):
    scene, w, h = synth.config_scene("1m_1080p", 0)
    cp = synth.default_camera_params(w, h)
    teacher = ba.Splats(scene["transforms"], scene["sh"], scene["raw_opac"], device=dev)
    host_views = []
    for v in range(nviews):
        ang = 2.0 * math.pi * v / nviews
        pos = (cp["pos"][0] + math.cos(ang) - 1.0, cp["pos"][1] + 0.5 * math.sin(ang), cp["pos"][2])
        yaw = -math.atan2(pos[0] - cp["pos"][0], 7.0)
        c = ba.Camera(position=pos, rotation=(0.0, math.sin(yaw / 2.0), 0.0, math.cos(yaw / 2.0)), fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
        img, _ = ba.render_splats(teacher, c, (w, h), (0.0, 0.0, 0.0), ba.RasterPass.Backward, ctx=ctx)
        host_views.append((np.ascontiguousarray((img[..., :3].clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8).cpu().numpy()), c.uniforms((w, h))))
    del teacher
    rng = np.random.default_rng(0x57D)   # the student of bench.py train_loop
    n0 = scene["transforms"].shape[0]
    st_tr = scene["transforms"].copy()
    st_tr[:, 0:3] += rng.normal(scale=0.02, size=(n0, 3)).astype(np.float32)
    st_tr[:, 3:7] += rng.normal(scale=0.15, size=(n0, 4)).astype(np.float32)
    st_tr[:, 7:10] += rng.normal(loc=-0.1, scale=0.25, size=(n0, 3)).astype(np.float32)
    st_sh = scene["sh"].copy()
    st_sh[:, 0, :] = 0.5 * st_sh[:, 0, :] + rng.normal(scale=0.3, size=(n0, 3)).astype(np.float32)
    st_op = (scene["raw_opac"] + rng.normal(scale=1.0, size=n0).astype(np.float32)).astype(np.float32)
    holder = [ba.Splats(st_tr, st_sh, st_op, device=dev)]
    trainer = ba.SplatTrainer(ba.TrainConfig(exact_lists=True, refine_every=refine_every), median_scene_scale=5.0, ctx=ctx, seed=0xB5EED)
    trainer.set_bounds(*ba.splat_bounds(holder[0], ctx=ctx))
    ctx.check(ctx.lib.bh_forget_views(ctx._h))
    loader = ba.SceneLoader(host_views, seed=3, slots=3, ctx=ctx)
    at = {total_steps - 390, total_steps - 250, total_steps - 50, total_steps - 1}
    try:
        for it in range(1, total_steps + 1):
            step = lambda: trainer.step(loader.next_batch(), holder[0])   # noqa: E731
            if it in at:
                out.append(sample("loop exact_lists, %d steps" % total_steps, it, trainer, rows, step))
            else:
                step()
            if it % refine_every == 0 and it < total_steps:
                holder[0], _ = trainer.refine(it, holder[0])
    finally:
        loader.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--loop-steps", type=int, default=1500)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import brush_amd as ba
    from brush_amd import synth
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ctx = ba.get_context(dev)
    out = []
    headline(ba, synth, dev, ctx, args.rows, out)
    if not args.skip_loop:
        loop(ba, synth, dev, ctx, args.rows, out, args.loop_steps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
