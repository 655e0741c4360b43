"""Developer tool (GPU box): what LPIPS (crates/lpips/src/lib.rs; the lpips_loss_weight term of train.rs:265-273) costs.  Test
weights (Lpips.random: the timings do not depend on the values).  Prints JSON lines:
  * {"what": "lpips", size}: bh_lpips_forward and bh_lpips_value_and_grad at 1920x1080 and 3840x2160, device events, medians of
    `--rounds` rounds of `--reps` calls; the shape-derived FLOPs (2 P Cin Cout 9 per conv: 2 images forward + pred's data
    gradient of convs 2..13) over the time, against the 157.3 TF f32 matrix peak;
  * {"what": "train_step"}: bh_train_step at brush_amd/synth.py's 1 M splats / 1080p workload with lpips_loss_weight 0.2 and 0,
    alternated step by step in one run (two trainers on the same ctx), medians.
Per-conv-layer kernel times come from a separate trace of value_and_grad at 1080p alone:
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python scripts/lpips_probe.py --trace
    python scripts/lpips_probe.py --layers <dir>/.../run_kernel_trace.csv
which labels the last call's 39 conv dispatches (GT forward, pred forward, pred data gradient) and prints per layer: µs, TFLOP/s
and the share of the f32 matrix peak.
    python scripts/lpips_probe.py [--reps 5] [--rounds 5] [--sizes 1080p,4k] [--no-train]
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import brush_amd as ba   # noqa: E402
from brush_amd import host, synth   # noqa: E402

PEAK_TF = 157.3   # f32-input MFMA peak of the MI355X (MI355X_MICROARCH.md)
SIZES = {"1080p": (1920, 1080), "4k": (3840, 2160)}
BLOCK_OF = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)
NAMES = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3", "conv5_1",
         "conv5_2", "conv5_3")


def dims(w, h):
    hw = [(h, w)]
    for _ in range(4):
        hw.append((hw[-1][0] // 2, hw[-1][1] // 2))
    return [a * b for a, b in hw]


def layer_flops(w, h):
    P = dims(w, h)
    return [2.0 * P[BLOCK_OF[L]] * ci * co * 9 for L, (ci, co) in enumerate(host.LPIPS_CONVS)]


def total_flops(w, h, grad):
    f = layer_flops(w, h)
    return 2 * sum(f) + (sum(f[1:]) + f[0] if grad else 0.0)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def inputs(w, h, seed=0):
    rng = np.random.default_rng(seed)
    img = torch.from_numpy(rng.uniform(0, 1, (h, w, 4)).astype(np.float32)).cuda()
    gt = torch.from_numpy(rng.integers(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
    return img, gt


def probe_sizes(ctx, model, sizes, reps, rounds):
    for name in sizes:
        w, h = SIZES[name]
        img, gt = inputs(w, h)
        v_out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        fwd = lambda: ba.lpips(img, gt, model, ctx=ctx)   # noqa: E731
        vg = lambda: ba.lpips_value_and_grad(img, gt, model, v_output=v_out, ctx=ctx)   # noqa: E731
        fwd()
        vg()
        torch.cuda.synchronize()
        tf, tg = [], []
        for _ in range(rounds):
            tf.append(timed(fwd, reps))
            tg.append(timed(vg, reps))
        mf, mg = float(np.median(tf)), float(np.median(tg))
        ff, fg = total_flops(w, h, False), total_flops(w, h, True)
        print(json.dumps({"what": "lpips", "size": name, "forward_ms": round(mf, 3), "value_and_grad_ms": round(mg, 3),
                          "forward_ms_range": [round(min(tf), 3), round(max(tf), 3)], "value_and_grad_ms_range": [round(min(tg), 3), round(max(tg), 3)],
                          "forward_tflops": round(ff / mf / 1e9, 1), "value_and_grad_tflops": round(fg / mg / 1e9, 1),
                          "forward_peak_share": round(ff / mf / 1e9 / PEAK_TF, 3), "value_and_grad_peak_share": round(fg / mg / 1e9 / PEAK_TF, 3),
                          "forward_tflop": round(ff / 1e12, 3), "value_and_grad_tflop": round(fg / 1e12, 3)}), flush=True)
        del img, gt, v_out


def probe_train(ctx, model, steps):
    sc, w, h = synth.config_scene("1m_1080p", sh_degree=3)
    cp = synth.default_camera_params(w, h)
    cam = ba.Camera(position=cp["pos"], rotation=cp["rot_xyzw"], fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
    gt = torch.from_numpy(synth.synthetic_gt_packed(w, h).view(np.int32)).cuda()
    runs = {}
    for key, wgt in (("lpips", 0.2), ("plain", 0.0)):
        spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device="cuda")
        tr = ba.SplatTrainer(ba.TrainConfig(lpips_loss_weight=wgt, growth_stop_iter=0), median_scene_scale=3.0, ctx=ctx, lpips=model)
        runs[key] = (spl, tr, [])
    batch = ba.SceneBatch(gt, cam)
    for i in range(steps + 3):
        for key in ("lpips", "plain"):
            spl, tr, ts = runs[key]
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.step(batch, spl)
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                ts.append(e0.elapsed_time(e1))
    a, b = runs["lpips"][2], runs["plain"][2]
    print(json.dumps({"what": "train_step", "workload": "1m_1080p sh3", "lpips_weight": 0.2, "with_lpips_ms": round(float(np.median(a)), 2),
                      "without_ms": round(float(np.median(b)), 2), "with_range": [round(min(a), 2), round(max(a), 2)],
                      "without_range": [round(min(b), 2), round(max(b), 2)], "steps": steps}), flush=True)


def layers_from_trace(path):
    rows = list(csv.DictReader(open(path)))
    convs = [r for r in rows if "lpips_conv3x3" in r["Kernel_Name"]]
    per_call = 39
    last = convs[-per_call:]
    w, h = SIZES["1080p"]
    fl = layer_flops(w, h)
    labels = [("gt_fwd", L) for L in range(13)] + [("pred_fwd", L) for L in range(13)] + [("pred_dgrad", L) for L in range(12, -1, -1)]
    out = []
    for (kind, L), r in zip(labels, last):
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        tf = fl[L] / us / 1e6
        out.append({"layer": NAMES[L], "pass": kind, "us": round(us, 1), "tflops": round(tf, 1), "peak_share": round(tf / PEAK_TF, 3),
                    "kernel": r["Kernel_Name"][:60]})
    for o in out:
        print(json.dumps(o))
    for kind in ("gt_fwd", "pred_fwd", "pred_dgrad"):
        sel = [o for o in out if o["pass"] == kind and o["layer"] in NAMES[1:10]]
        us = sum(o["us"] for o in sel)
        f = sum(fl[NAMES.index(o["layer"])] for o in sel)
        print(json.dumps({"pass": kind, "layers": "conv1_2..conv4_3", "us": round(us, 1), "tflops": round(f / us / 1e6, 1),
                          "peak_share": round(f / us / 1e6 / PEAK_TF, 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--train-steps", type=int, default=12)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--trace", action="store_true", help="value_and_grad at 1080p only, 3 calls (for a rocprofv3 run)")
    ap.add_argument("--layers", help="label the conv dispatches of a rocprofv3 kernel_trace.csv of --trace")
    args = ap.parse_args()
    if args.layers:
        layers_from_trace(args.layers)
        return
    torch.cuda.set_device(0)
    ctx = ba.get_context()
    model = ba.Lpips.random(seed=1, ctx=ctx)
    if args.trace:
        w, h = SIZES["1080p"]
        img, gt = inputs(w, h)
        for _ in range(3):
            ba.lpips_value_and_grad(img, gt, model, ctx=ctx)
        torch.cuda.synchronize()
        return
    probe_sizes(ctx, model, [s for s in args.sizes.split(",") if s], args.reps, args.rounds)
    if not args.no_train:
        probe_train(ctx, model, args.train_steps)


if __name__ == "__main__":
    main()
