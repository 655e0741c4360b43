"""Developer tool (GPU box): what distortion maps (include/brush_hip_distortion.h) cost at brush_amd/synth.py's 1 M splats
/ 1080p workload (the headline scene, SH degree 0), next to the depth kernels on the SAME saved forward.  Prints one JSON line:
  * forward_ms: the BH_FLAG_BWD_INFO forward (K16 inside);
  * depth_accumulated_us / depth_expected_us: bh_render_depth, the kernel the distortion forward is measured against;
  * distortion_z_us / distortion_ndc_us / distortion_moments_us: bh_render_distortion (NDC: the per-splat depth kernel + the blend) and
    bh_render_distortion_moments; distortion_loss_us: bh_distortion_loss on the moment map;
  * backward_depth_ms: bh_render_backward_depth_saved with v_output = NULL (depth forward into scratch + replay + K18 + the v_z scatter);
  * backward_distortion_{z,ndc}_ms: bh_render_backward_distortion_saved with the distortion term alone (moment forward into scratch +
    replay + K18 + the v_z scatter; NDC: the two per-splat kernels as well);
  * step_plain_ms / step_distortion_ms: SplatTrainer.step without and with TrainConfig.distortion_loss_weight (the moment forward, the
    loss and the term's replay inside the step's one backward), every round's figure beside the median.
Device events, medians of `--rounds` rounds of `--reps` calls each, the candidates alternated inside a round.
    python scripts/distortion_probe.py [--reps 20] [--rounds 7] [--weight 100]
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--weight", type=float, default=100.0)
    ap.add_argument("--near", type=float, default=0.2)
    ap.add_argument("--far", type=float, default=1000.0)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    ctx = ba.Context(dev)
    sc, w, h = synth.config_scene("1m_1080p", sh_degree=0)
    splats = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device="cuda")
    cp = synth.default_camera_params(w, h)
    cam = ba.Camera(position=cp["pos"], rotation=cp["rot_xyzw"], fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
    rng = np.random.default_rng(3)
    v_dep = torch.from_numpy((rng.uniform(-1.0, 1.0, (h, w)) / (h * w)).astype(np.float32)).cuda()
    v_dis = torch.from_numpy((rng.uniform(0.0, 1.0, (h, w)) / (h * w)).astype(np.float32)).cuda()
    out_d = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    out_m = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    ndc = ("ndc", args.near, args.far)
    state = {}

    def forward():
        state["node"] = ba.render_splats_diff(splats, cam, (w, h), ctx=ctx)

    forward()
    o = state["node"].out
    moments = ba.render_distortion(state["node"], "z", moments=True).clone()
    mean_dist = float(ba.distortion_loss(moments, 1.0, ctx=ctx).cpu()[0])
    gt = torch.from_numpy(np.ascontiguousarray(synth.synthetic_gt_packed(w, h)).view(np.int32)).to(dev)
    runs = {}
    for name, weight in (("step_plain_ms", 0.0), ("step_distortion_ms", args.weight)):
        spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device="cuda")
        tr = ba.SplatTrainer(ba.TrainConfig(distortion_loss_weight=weight), median_scene_scale=3.0, ctx=ctx)
        runs[name] = (lambda tr=tr, spl=spl: tr.step(ba.SceneBatch(gt, cam, view_id=1), spl))
    # (the map and backward candidates act on the most recent differentiable forward: `forward` runs in front of them in every round)
    cands = {
        "forward_ms": forward,
        "depth_accumulated_us": lambda: ba.render_depth(state["node"], "accumulated", out=out_d),
        "depth_expected_us": lambda: ba.render_depth(state["node"], "expected", out=out_d),
        "distortion_z_us": lambda: ba.render_distortion(state["node"], "z", out=out_d),
        "distortion_ndc_us": lambda: ba.render_distortion(state["node"], *ndc, out=out_d),
        "distortion_moments_us": lambda: ba.render_distortion(state["node"], "z", out=out_m, moments=True),
        "distortion_loss_us": lambda: ba.distortion_loss(moments, args.weight, ctx=ctx),
        "backward_depth_ms": lambda: state["node"].backward(None, v_depth=v_dep, depth_mode="accumulated"),
        "backward_distortion_z_ms": lambda: state["node"].backward(None, v_distortion=v_dis, distortion="z"),
        "backward_distortion_ndc_ms": lambda: state["node"].backward(None, v_distortion=v_dis, distortion="ndc", distortion_near=args.near, distortion_far=args.far),
    }
    times = {k: [] for k in list(cands) + list(runs)}
    for fn in cands.values():
        fn()
    for fn in runs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, fn in cands.items():
            times[k].append(timed(fn, args.reps))
        for k, fn in runs.items():
            times[k].append(timed(fn, args.reps))
    res = dict(n=splats.num_splats(), w=w, h=h, pairs=int(o.num_intersections), listed_splats=int(o.num_listed_splats), weight=args.weight,
               mean_distortion=mean_dist)
    for k, v in times.items():
        med = float(np.median(v))
        res[k] = round(med * 1e3, 1) if k.endswith("_us") else round(med, 4)
        if k.startswith("step_"):
            res[k.rsplit("_", 1)[0] + "_rounds"] = [round(x, 4) for x in v]
    print(json.dumps(res), flush=True)
    ctx.sync()
    ctx.close()


if __name__ == "__main__":
    main()
