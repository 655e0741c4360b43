"""Developer tool (GPU box): what feature maps (include/brush_hip_features.h) cost at brush_amd/synth.py's 1 M splats /
1080p workload (the headline scene, SH degree 0), per channel count and per forced chunk width (option feature_chunk), next to the
normal-map kernels on the SAME saved forward.  Prints one JSON line:
  * normal_forward_ms / normal_backward_ms: bh_render_normal (accumulated) and bh_render_backward_normal_saved with the normal term
    alone — the yardsticks of the C = 3 rows (same skeleton, same three folds);
  * features: for every C in --channels and chunk width in 4, 8, 16: forward_ms (bh_render_features: gather + blend), backward_ms
    (bh_render_backward_features_saved with the feature term alone: gather + forward into scratch + replay + K18 + the copy into
    the dense v_features), and ns per (blended pair, channel) of both;
  * chosen: the width the library picks by itself per C (feature_chunk = 0), timed the same way.
Device events, medians of `--rounds` rounds of `--reps` calls each, the candidates alternated inside a round.
    python scripts/feature_probe.py [--reps 3] [--rounds 5] [--channels 3,16,64,256]
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--channels", default="3,16,64,256")
    args = ap.parse_args()
    channels = [int(c) for c in args.channels.split(",")]
    torch.cuda.set_device(0)
    ctx = ba.Context(torch.device("cuda:0"))
    sc, w, h = synth.config_scene("1m_1080p", sh_degree=0)
    splats = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device="cuda")
    n = splats.num_splats()
    cp = synth.default_camera_params(w, h)
    cam = ba.Camera(position=cp["pos"], rotation=cp["rot_xyzw"], fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
    node = ba.render_splats_diff(splats, cam, (w, h), ctx=ctx)
    o = node.out
    to = host._view(o.tile_offsets, (o.num_tiles, 2), torch.int32, "cuda").cpu().numpy().astype(np.int64)
    lists = to[:, 1] - to[:, 0]
    pairs = int(lists.sum())
    gen = torch.Generator(device="cuda").manual_seed(3)
    v_nrm = (torch.rand((h, w, 3), generator=gen, device="cuda") * 2.0 - 1.0) / (h * w)
    out_n = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")

    def with_chunk(width, fn):
        def run():
            ctx.set_option("feature_chunk", width)
            fn()
        return run

    cands = {
        ("normal", 0, "forward"): lambda: ba.render_normal(node, "accumulated", out=out_n),
        ("normal", 0, "backward"): lambda: node.backward(None, v_normal=v_nrm, normal_mode="accumulated"),
    }
    keep = []
    for c in channels:
        f = torch.randn((n, c), generator=gen, device="cuda")
        v = (torch.rand((h, w, c), generator=gen, device="cuda") * 2.0 - 1.0) / (h * w)
        out = torch.zeros((h, w, c), dtype=torch.float32, device="cuda")
        keep.append((f, v, out))
        for width in (4, 8, 16, 0):
            cands[(c, width, "forward")] = with_chunk(width, lambda f=f, out=out: ba.render_features(node, f, out=out))
            cands[(c, width, "backward")] = with_chunk(width, lambda f=f, v=v: node.backward(None, v_features=v, features=f))
    times = {k: [] for k in cands}
    for fn in cands.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, fn in cands.items():
            times[k].append(timed(fn, args.reps))
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = dict(n=n, w=w, h=h, pairs=int(o.num_intersections), blended_pairs=pairs, longest_list=int(lists.max()), listed_splats=int(o.num_listed_splats),
               normal_forward_ms=round(med[("normal", 0, "forward")], 4), normal_backward_ms=round(med[("normal", 0, "backward")], 4), features=[], chosen=[])
    for c in channels:
        for width in (4, 8, 16, 0):
            fw, bw = med[(c, width, "forward")], med[(c, width, "backward")]
            row = dict(channels=c, chunk=width, forward_ms=round(fw, 4), backward_ms=round(bw, 4),
                       forward_ns_per_pair_channel=round(fw * 1e6 / (pairs * c), 4), backward_ns_per_pair_channel=round(bw * 1e6 / (pairs * c), 4))
            (res["chosen"] if width == 0 else res["features"]).append(row)
    print(json.dumps(res), flush=True)
    ctx.set_option("feature_chunk", 0)
    ctx.sync()
    ctx.close()


if __name__ == "__main__":
    main()
