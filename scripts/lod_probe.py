"""Developer tool (GPU box): what a LOD boundary costs (brush-train/src/lod.rs; brush-process/src/train_stream.rs:248-303) at
brush_amd/synth.py's 1 M splats / 1080p workload, 16 views around the synthetic frustum scene, GT = the scene's own 8-bit render.
Prints
  * per-view ms of the fused bh_pup_accumulate_view, end to end (device events, profiler off) and split into forward / loss /
    backward / accumulate (bh_profile_* stages, a separate pass);
  * bh_pup_scores and bh_decimate_to_count (keep 50 %) in us;
  * the reference's accumulate shape in torch ops (cat, [N,6,6] broadcast outer product, add) beside bh_pup_accumulate;
  * held-out PSNR (4 views between the training views) of the top-50 %, bottom-50 % and a random 50 % set.
    python scripts/lod_probe.py [--sh-degree 3] [--views 16]
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import brush_amd as ba   # noqa: E402
from brush_amd import host, synth   # noqa: E402

FORWARD = ("ProjectSplats", "DepthSort", "MapGaussiansToIntersect", "PrefixSumGaussHits", "ProjectVisible", "TileSort", "GetTileOffsets", "Rasterize")
BACKWARD = ("ZeroGradBuffers", "RasterizeBackwards", "ProjectBackwards")


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def cameras(k, cp, yaw0, spread):
    """k cameras at the origin turned by small yaw / pitch angles (the scene fills the default frustum)"""
    out = []
    for v in range(k):
        yaw = yaw0 + spread * (v / max(k - 1, 1) - 0.5)
        pitch = 0.03 * math.sin(2.7 * v)
        qy = np.array([0.0, math.sin(yaw / 2), 0.0, math.cos(yaw / 2)])
        qx = np.array([math.sin(pitch / 2), 0.0, 0.0, math.cos(pitch / 2)])
        x1, y1, z1, w1 = qy
        x2, y2, z2, w2 = qx
        q = (w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2,
             w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2)
        out.append(ba.Camera(position=(0.02 * math.sin(v), 0.0, 0.0), rotation=tuple(float(c) for c in q), fov_x=cp["fov_x"], fov_y=cp["fov_y"]))
    return out


def render_rgb(splats, cam, w, h, ctx):
    img, _ = ba.render_splats(splats, cam, (w, h), (0.0, 0.0, 0.0), pass_=ba.RasterPass.Backward, ctx=ctx)
    return img[..., :3].clamp(0, 1)


def psnr(a, b):
    mse = float(torch.mean((a.double() - b.double()) ** 2))
    return 10.0 * math.log10(1.0 / max(mse, 1e-12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--views", type=int, default=16)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = ba.get_context()
    sc, w, h = synth.config_scene("1m_1080p", sh_degree=args.sh_degree)
    splats = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device="cuda")
    n = splats.num_splats()
    cp = synth.default_camera_params(w, h)
    train = cameras(args.views, cp, 0.0, 0.3)
    held = cameras(4, cp, 0.3 / (2 * (args.views - 1)), 0.3 * 0.75)
    views = [((render_rgb(splats, c, w, h, ctx) * 255.0 + 0.5).to(torch.uint8).cpu().numpy(), c) for c in train]
    print("workload: %d splats, SH degree %d, %dx%d, %d views" % (n, args.sh_degree, w, h, len(views)), flush=True)

    # GT packed once on the device (opaque RGB: view_to_packed_data's a = 255); the uploader is timed with it at the end
    gts = []
    for img, _ in views:
        t = torch.from_numpy(img).cuda().to(torch.int64)
        packed = t[..., 0] | (t[..., 1] << 8) | (t[..., 2] << 16) | (255 << 24)
        gts.append(torch.where(packed >= 2**31, packed - 2**32, packed).to(torch.int32).contiguous())
    hess = torch.zeros((host.PUP_PLANES, n), dtype=torch.float32, device="cuda")

    def all_views():
        hess.zero_()
        for (_, cam), gt in zip(views, gts):
            host.pup_accumulate_view(splats, cam, gt, hess, ctx)

    ms = timed(all_views, reps=3, warm=1)
    print("fused view call: %.3f ms per view (%d views, device events, profiler off)" % (ms / len(views), len(views)), flush=True)
    ctx.profile(True)
    all_views()
    torch.cuda.synchronize()
    prof = ctx.profile_fetch()
    ctx.profile(False)
    split = {"forward": sum(prof.get(k, (0, 0))[0] for k in FORWARD), "loss": prof.get("PupLoss", (0, 0))[0],
             "backward": sum(prof.get(k, (0, 0))[0] for k in BACKWARD), "accumulate": prof.get("PupAccumulate", (0, 0))[0]}
    print("per view (profiled pass): " + ", ".join("%s %.3f ms" % (k, v / len(views)) for k, v in split.items()), flush=True)
    print("  stages: " + ", ".join("%s %.3f" % (k, v[0] / len(views)) for k, v in sorted(prof.items(), key=lambda kv: -kv[1][0])), flush=True)

    scores = host.pup_scores(hess, ctx)
    us = timed(lambda: host.pup_scores(hess, ctx)) * 1e3
    print("bh_pup_scores: %.1f us (%d splats)" % (us, n), flush=True)
    k = ba.lod_target_count(n, 50)
    us = timed(lambda: ba.decimate_to_count(splats, scores, k, ctx=ctx)) * 1e3
    print("bh_decimate_to_count keep 50 %%: %.1f us (incl. the output allocation)" % us, flush=True)

    # the reference's accumulate shape (lod.rs:120-126) restated in torch, beside the kernel, on one view's gradients
    node = ba.render_splats_diff(splats, views[0][1], (w, h), ctx=ctx)
    _, v_out = ba.image_loss_value_and_grad(node.img, gts[0], l1_weight=1.0, ssim_weight=0.0, ctx=ctx)
    vt = node.backward(v_out)["v_transforms"]
    h36 = torch.zeros((n, 6, 6), dtype=torch.float32, device="cuda")

    def torch_shape():
        nonlocal h36
        j = torch.cat([vt[:, 0:3], vt[:, 7:10]], 1)
        h36 = h36 + j.unsqueeze(2) * j.unsqueeze(1)

    t_torch = timed(torch_shape)
    t_kernel = timed(lambda: host.pup_accumulate(vt, hess, ctx=ctx))
    nz = int((vt[:, [0, 1, 2, 7, 8, 9]] != 0).any(1).sum())
    print("accumulate one view: torch [N,6,6] shape %.1f us, bh_pup_accumulate dense %.1f us (%d of %d rows non-zero)"
          % (t_torch * 1e3, t_kernel * 1e3, nz, n), flush=True)
    del h36, node

    # held-out PSNR of the kept halves
    bottom_scores = -scores.nan_to_num(nan=-math.inf)
    top, bottom = ba.decimate_to_count(splats, scores, k, ctx=ctx), ba.decimate_to_count(splats, bottom_scores, k, ctx=ctx)
    perm = torch.from_numpy(np.random.default_rng(1).permutation(n)[:k]).cuda()
    rand = ba.Splats(splats.transforms[perm], splats.sh_coeffs[perm], splats.raw_opacities[perm], device="cuda")
    res = {"top": [], "bottom": [], "random": []}
    for c in held:
        gt = torch.round(render_rgb(splats, c, w, h, ctx) * 255.0) / 255.0
        for name, s in (("top", top), ("bottom", bottom), ("random", rand)):
            res[name].append(psnr(render_rgb(s, c, w, h, ctx), gt))
    print("held-out PSNR keep 50 %%: top %.2f dB, bottom %.2f dB, random %.2f dB (%d views)"
          % (np.mean(res["top"]), np.mean(res["bottom"]), np.mean(res["random"]), len(held)), flush=True)
    t0 = time.time()
    ba.compute_pup_scores(splats, views, ctx=ctx)
    torch.cuda.synchronize()
    print("compute_pup_scores end to end incl. GT upload: %.3f s for %d views" % (time.time() - t0, len(views)), flush=True)


if __name__ == "__main__":
    main()
