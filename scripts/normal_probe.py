"""Developer tool (GPU box): what normal maps (include/brush_hip_normal.h) cost at brush_amd/synth.py's 1 M splats /
1080p workload (the headline scene, SH degree 0), next to the depth and colour kernels on the SAME saved forward.  Prints one JSON
line:
  * forward_ms: the BH_FLAG_BWD_INFO forward (K16 inside);
  * splat_normals_us: bh_splat_normals over all N splats;
  * normal_{accumulated,unit}_us: bh_render_normal (the compact splat normals + the blend), beside depth_expected_us: bh_render_depth;
  * depth_to_normal_us / depth_to_normal_backward_us: the two streaming kernels on the frame's expected depth;
  * backward_colour_ms: bh_render_backward_saved (K17 + K18);
  * backward_depth_ms: bh_render_backward_depth_saved with v_output = NULL (depth forward into scratch + depth backward + K18 + v_z);
  * backward_normal_ms: bh_render_backward_normal_saved with the normal term alone (compact normals + normal forward into scratch +
    normal backward + K18 + the Vn kernel), backward_all_ms: the same with a v_output and a v_depth (K17 and the depth term as well).
Device events, medians of `--rounds` rounds of `--reps` calls each, the candidates alternated inside a round.
Kernel times come from a separate trace of the same loops (few reps):
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/normal_probe.py --trace
    python scripts/normal_probe.py [--reps 20] [--rounds 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import brush_amd as ba   # noqa: E402
from brush_amd import host, synth   # noqa: E402


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
    ap.add_argument("--trace", action="store_true", help="few reps (for a rocprofv3 run)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = ba.Context(torch.device("cuda:0"))
    sc, w, h = synth.config_scene("1m_1080p", sh_degree=0)
    splats = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device="cuda")
    cp = synth.default_camera_params(w, h)
    cam = ba.Camera(position=cp["pos"], rotation=cp["rot_xyzw"], fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
    rng = np.random.default_rng(3)
    v_out = torch.from_numpy((rng.uniform(-1.0, 1.0, (h, w, 4)) / (h * w)).astype(np.float32)).cuda()
    v_dep = torch.from_numpy((rng.uniform(-1.0, 1.0, (h, w)) / (h * w)).astype(np.float32)).cuda()
    v_nrm = torch.from_numpy((rng.uniform(-1.0, 1.0, (h, w, 3)) / (h * w)).astype(np.float32)).cuda()
    out_d = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    out_n = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    reps = 3 if args.trace else args.reps
    rounds = 2 if args.trace else args.rounds
    state = {}

    def forward():
        state["node"] = ba.render_splats_diff(splats, cam, (w, h), ctx=ctx)

    forward()
    o = state["node"].out
    to = host._view(o.tile_offsets, (o.num_tiles, 2), torch.int32, "cuda").cpu().numpy().astype(np.int64)
    lists = to[:, 1] - to[:, 0]
    depth = ba.render_depth(state["node"], "expected").clone()
    # (the map and backward candidates act on the most recent forward)
    cands = {
        "forward_ms": forward,
        "splat_normals_us": lambda: ba.splat_normals(splats, cam, ctx=ctx),
        "depth_expected_us": lambda: ba.render_depth(state["node"], "expected", out=out_d),
        "normal_accumulated_us": lambda: ba.render_normal(state["node"], "accumulated", out=out_n),
        "normal_unit_us": lambda: ba.render_normal(state["node"], "unit", out=out_n),
        "depth_to_normal_us": lambda: ba.depth_to_normal(depth, cam, ctx=ctx),
        "depth_to_normal_backward_us": lambda: ba.depth_to_normal_backward(depth, v_nrm, cam, ctx=ctx),
        "backward_colour_ms": lambda: state["node"].backward(v_out),
        "backward_depth_ms": lambda: state["node"].backward(None, v_depth=v_dep, depth_mode="expected"),
        "backward_normal_ms": lambda: state["node"].backward(None, v_normal=v_nrm, normal_mode="unit"),
        "backward_all_ms": lambda: state["node"].backward(v_out, v_depth=v_dep, depth_mode="expected", v_normal=v_nrm, normal_mode="unit"),
    }
    times = {k: [] for k in cands}
    for fn in cands.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in cands.items():
            times[k].append(timed(fn, reps))
    res = dict(n=splats.num_splats(), w=w, h=h, pairs=int(o.num_intersections), blended_pairs=int(lists.sum()), longest_list=int(lists.max()),
               listed_splats=int(o.num_listed_splats))
    for k, v in times.items():
        med = float(np.median(v))
        res[k] = round(med * 1e3, 1) if k.endswith("_us") else round(med, 4)
    print(json.dumps(res), flush=True)
    ctx.sync()
    ctx.close()


if __name__ == "__main__":
    main()
