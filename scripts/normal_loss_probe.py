"""Developer tool (GPU box): what the normal-consistency regulariser (include/brush_hip_normal_loss.h) costs at
brush_amd/synth.py's 1 M splats / 1080p workload (the headline scene, SH degree 0).  Prints one JSON line:
  * fused_us: bh_normal_consistency_value_and_grad on the frame's accumulated normals, expected depth and image;
  * composed_us: the three-call composition it replaces — bh_depth_to_normal, the loss and its two cotangents in torch
    (v_normal = -c A u, v_u = -c A N), bh_depth_to_normal_backward — with composed_parts_us = [depth_to_normal, torch, backward];
  * step_plain_ms / step_normal_ms: bh_train_step without and with the term (weight 0.05) on two copies of the scene.
Device events, medians of `--rounds` (default five) rounds of `--reps` calls each, the candidates alternated inside a round.
    python scripts/normal_loss_probe.py [--reps 20] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import brush_amd as ba   # noqa: E402
from brush_amd import synth   # noqa: E402


def timed(fn, reps):
    """mean device ms per call over `reps` back-to-back calls"""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--weight", type=float, default=0.05)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    ctx = ba.Context(dev)   # (on torch's current stream: the torch part of the composition is ordered with the library's calls)
    sc, w, h = synth.config_scene("1m_1080p", sh_degree=0)
    splats = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device="cuda")
    cp = synth.default_camera_params(w, h)
    cam = ba.Camera(position=cp["pos"], rotation=cp["rot_xyzw"], fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
    node = ba.render_splats_diff(splats, cam, (w, h), ctx=ctx)
    normal, depth, image = node.normal("accumulated").clone(), node.depth("expected").clone(), node.img.clone()
    ctx.sync()
    c = float(np.float32(np.float64(np.float32(args.weight)) / np.float64(h * w)))
    alpha = image[..., 3:4]
    parts = {"depth_to_normal": [], "torch": [], "backward": []}
    keep = {}

    def fused():
        keep["fused"] = ba.normal_consistency_value_and_grad(normal, depth, image, cam, args.weight, ctx=ctx)

    def p_u():
        keep["u"] = ba.depth_to_normal(depth, cam, ctx=ctx)

    def p_torch():
        u = keep["u"]
        valid = (u != 0).any(-1, keepdim=True)
        keep["loss"] = c * (alpha * (1.0 - (normal * u).sum(-1, keepdim=True)) * valid).sum()
        keep["v_normal"] = (-c * alpha) * u
        keep["v_u"] = (-c * alpha) * normal

    def p_bwd():
        keep["v_depth"] = ba.depth_to_normal_backward(depth, keep["v_u"], cam, ctx=ctx)

    def composed():
        p_u()
        p_torch()
        p_bwd()

    # the two answers agree before anything is timed
    fused()
    composed()
    torch.cuda.synchronize()
    loss, v_normal, v_depth = keep["fused"]
    agree = dict(loss=[float(loss[0]), float(keep["loss"])],
                 v_normal=float((v_normal - keep["v_normal"]).abs().max() / keep["v_normal"].abs().max()),
                 v_depth=float((v_depth - keep["v_depth"]).abs().max() / keep["v_depth"].abs().max()))

    gt = torch.from_numpy(np.ascontiguousarray(synth.synthetic_gt_packed(w, h)).view(np.int32)).to(dev)
    runs = {}
    for name, weight in (("step_plain_ms", 0.0), ("step_normal_ms", args.weight)):
        spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device="cuda")
        tr = ba.SplatTrainer(ba.TrainConfig(normal_loss_weight=weight), median_scene_scale=3.0, ctx=ctx)
        runs[name] = (lambda tr=tr, spl=spl: tr.step(ba.SceneBatch(gt, cam, view_id=1), spl))
    cands = dict(fused_us=fused, composed_us=composed, **runs)
    times = {k: [] for k in cands}
    for fn in cands.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, fn in cands.items():
            times[k].append(timed(fn, args.reps))
        for k, fn in (("depth_to_normal", p_u), ("torch", p_torch), ("backward", p_bwd)):
            parts[k].append(timed(fn, args.reps))
    res = dict(n=splats.num_splats(), w=w, h=h, weight=args.weight, valid_pixels=int(loss[1]), agree=agree)
    for k, v in times.items():
        med = float(np.median(v))
        res[k] = round(med * 1e3, 1) if k.endswith("_us") else round(med, 4)
        res[k.rsplit("_", 1)[0] + "_rounds"] = [round(x * (1e3 if k.endswith("_us") else 1.0), 4 if k.endswith("_ms") else 1) for x in v]
    res["composed_parts_us"] = [round(float(np.median(parts[k])) * 1e3, 1) for k in ("depth_to_normal", "torch", "backward")]
    print(json.dumps(res), flush=True)
    ctx.sync()
    ctx.close()


if __name__ == "__main__":
    main()
