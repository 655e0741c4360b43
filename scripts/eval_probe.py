"""Developer tool (GPU box): what held-out evaluation (brush-train/src/eval.rs:23-63) costs at brush_amd/synth.py's 1 M splats /
1080p workload, SH degrees 0 and 3, GT = synth.synthetic_gt_packed.  Prints one JSON line per SH degree:
  * fused_us / composed_us: bh_eval_metrics against the composed path on the same f32 image — torch quantise, [H,W,4] -> [3,H,W],
    two bh_image_loss_forward maps (l1 1 ssim 0, l1 0 ssim 1), two torch sums — alternated in one run, device events, medians of
    `--rounds` rounds of `--reps` calls each;
  * eval_view_ms / forward_ms: bh_eval_view end to end against the BH_FLAG_BWD_INFO forward alone (the same camera, alternated);
  * fused_gbps / roofline_share: 20 bytes per pixel (the f32 image + the GT word) over the fused time, against 6.29 TB/s.
  * metrics_equal: the fused metrics equal the composed ones within one f32 ulp.
Kernel times come from a separate trace of the timing loops alone:
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/eval_probe.py --trace
    python scripts/eval_probe.py [--sh-degrees 0,3] [--reps 50] [--rounds 7]
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

HBM_TBPS = 6.29   # measured stream bandwidth of the MI355X


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
    ap.add_argument("--sh-degrees", default="0,3")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--trace", action="store_true", help="only the metric loops, SH 0, few reps (for a rocprofv3 run)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = ba.get_context()
    degrees = [0] if args.trace else [int(d) for d in args.sh_degrees.split(",")]
    for deg in degrees:
        sc, w, h = synth.config_scene("1m_1080p", sh_degree=deg)
        splats = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device="cuda")
        cp = synth.default_camera_params(w, h)
        cam = ba.Camera(position=cp["pos"], rotation=cp["rot_xyzw"], fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
        gt = torch.from_numpy(synth.synthetic_gt_packed(w, h).view(np.int32)).cuda()
        img, _ = ba.render_splats(splats, cam, (w, h), (0.0, 0.0, 0.0), ba.RasterPass.Backward, ctx=ctx)
        fused_out = torch.empty(3, dtype=torch.float32, device="cuda")
        l1_map = torch.empty((3, h, w), dtype=torch.float32, device="cuda")
        ss_map = torch.empty_like(l1_map)
        cfg_l1, cfg_ss = host._loss_cfg(1.0, 0.0, None, False), host._loss_cfg(0.0, 1.0, None, False)
        composed_out = torch.empty(2, dtype=torch.float64, device="cuda")
        d255 = torch.full((h, w, 3), 255.0, dtype=torch.float32, device="cuda")   # a true divide (a scalar divisor is a reciprocal multiply in torch)

        def fused():
            ba.eval_metrics(img, gt, ctx=ctx, out=fused_out)

        def composed():
            q = torch.round(img[..., :3] * 255.0) / d255
            chw = q.permute(2, 0, 1).contiguous()
            ctx.check(ctx.lib.bh_image_loss_forward(ctx._h, host._ptr(chw), host._ptr(gt), 3, h, w, host.C.byref(cfg_l1), host._ptr(l1_map)))
            ctx.check(ctx.lib.bh_image_loss_forward(ctx._h, host._ptr(chw), host._ptr(gt), 3, h, w, host.C.byref(cfg_ss), host._ptr(ss_map)))
            composed_out[0] = (l1_map * l1_map).sum(dtype=torch.float64)
            composed_out[1] = ss_map.sum(dtype=torch.float64)

        reps = 5 if args.trace else args.reps
        fused(), composed()
        torch.cuda.synchronize()
        tf, tc = [], []
        for _ in range(3 if args.trace else args.rounds):
            tf.append(timed(fused, reps))
            tc.append(timed(composed, reps))
        if args.trace:
            continue
        m = fused_out.cpu().numpy()
        cnt = 3.0 * h * w
        c = composed_out.cpu().numpy()
        c_mse, c_ssim = np.float32(c[0] / cnt), np.float32(c[1] / cnt)
        equal = bool(abs(float(m[0]) - float(c_mse)) <= float(np.spacing(c_mse)) and abs(float(m[2]) - float(c_ssim)) <= float(np.spacing(c_ssim)))

        # bh_eval_view end to end against the BWD_INFO forward alone
        bh_cam = cam.uniforms((w, h))
        view_out = torch.empty(3, dtype=torch.float32, device="cuda")

        def eval_view():
            host._eval_view(ctx, splats, bh_cam, gt, view_out, None)

        def forward():
            host._forward(ctx, splats, bh_cam, (w, h), (0.0, 0.0, 0.0), ba.RasterPass.Backward)

        for _ in range(3):
            eval_view(), forward()
        torch.cuda.synchronize()
        tv, tw = [], []
        for _ in range(args.rounds):
            tv.append(timed(eval_view, 10))
            tw.append(timed(forward, 10))
        view_equal = bool(torch.equal(view_out, fused_out))
        fused_us = 1e3 * float(np.median(tf))
        gbps = 20.0 * h * w / (fused_us * 1e-6) / 1e9
        print(json.dumps(dict(
            sh_degree=deg, n=splats.num_splats(), w=w, h=h,
            fused_us=round(fused_us, 2), composed_us=round(1e3 * float(np.median(tc)), 2),
            fused_us_range=[round(1e3 * min(tf), 2), round(1e3 * max(tf), 2)], composed_us_range=[round(1e3 * min(tc), 2), round(1e3 * max(tc), 2)],
            eval_view_ms=round(float(np.median(tv)), 4), forward_ms=round(float(np.median(tw)), 4),
            fused_gbps=round(gbps, 1), hbm_bound_us=round(20.0 * h * w / (HBM_TBPS * 1e12) * 1e6, 2), roofline_share=round(gbps / (HBM_TBPS * 1e3), 3),
            mse=float(m[0]), psnr=float(m[1]), ssim=float(m[2]), metrics_equal=equal, eval_view_equals_fused=view_equal)), flush=True)


if __name__ == "__main__":
    main()
