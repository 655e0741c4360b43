"""Developer tool (GPU box): what mesh extraction (include/brush_hip_mesh.h) costs.  Per volume size (256^3 and 512^3
samples with colour, eight 1920x1080 views of an analytic sphere around it) one JSON line:
  * single_ms / batched_ms: eight single-view calls of TsdfVolume.integrate against one eight-view call on a cleared volume (device
    events, medians of `--rounds` rounds, the two alternated inside a round);
  * touched / touched_single: the samples some view updated (per call); *_tbs: the achieved rate counting one read plus one write of the
    touched samples' 20 bytes per launch, and *_swept_tbs counting what the kernel moves (it reads every sample once per launch and
    writes the touched ones), next to `--hbm-tbs`, the rate a float4 copy reaches on this chip;
  * classify_ms / scan_ms / emit_ms: the three phases of extract_mesh (the library's stage events), and the mesh's counts.
Each size runs in a child process of its own under `--step-timeout` seconds; the first failure ends the run.
    python scripts/mesh_probe.py [--sizes 256 512] [--rounds 5]
"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def probe(size, rounds, hbm_tbs):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import brush_amd as ba
    from brush_amd import _ffi

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    ctx = ba.Context(dev)
    w, h, n_views = 1920, 1080, 8
    voxel = 2.0 / (size - 1)
    vol = ba.TsdfVolume((-1.0, -1.0, -1.0), voxel, (size, size, size), ctx=ctx)
    cams, depths, images = [], [], []
    ys, xs = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float64), torch.arange(w, device=dev, dtype=torch.float64), indexing="ij")
    for v in range(n_views):
        ang = 2.0 * math.pi * v / n_views
        pos = np.asarray([2.6 * math.cos(ang), 0.4 * math.sin(3.0 * ang), 2.6 * math.sin(ang)])
        fwd = -pos / np.linalg.norm(pos)
        right = np.cross([0.0, 1.0, 0.0], fwd)
        right /= np.linalg.norm(right)
        rwc = np.stack([right, np.cross(fwd, right), fwd])
        cam = _ffi.BhCamera()
        for c in range(3):
            for r in range(3):
                cam.vm[3 * c + r] = rwc[r, c]
        t = -rwc @ pos
        for r in range(3):
            cam.vm[9 + r], cam.cam_pos[r] = t[r], pos[r]
        cam.fx = cam.fy = 1500.0
        cam.cx, cam.cy, cam.img_w, cam.img_h, cam.model = 0.5 * w, 0.5 * h, w, h, _ffi.CAMERA_PINHOLE
        # z-depth of the sphere of radius 0.7 about the origin through every pixel centre
        d = torch.stack([(xs + 0.5 - cam.cx) / cam.fx, (ys + 0.5 - cam.cy) / cam.fy, torch.ones_like(xs)], dim=-1)
        c_cam = torch.tensor(t, device=dev)
        a, b, cc = (d * d).sum(-1), (d * c_cam).sum(-1), float(t @ t) - 0.49
        disc = b * b - a * cc
        depths.append(torch.where(disc > 0, (b - disc.clamp(min=0).sqrt()) / a, torch.zeros_like(a)).float().contiguous())
        img = torch.rand((h, w, 4), device=dev)
        img[..., 3] = 1.0
        images.append(img)
        cams.append(cam)

    def single():
        for v in range(n_views):
            vol.integrate([depths[v]], [cams[v]], [images[v]])

    def batched():
        vol.integrate(depths, cams, images)

    def timed(fn):
        vol.clear()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    touched_single = 0
    for v in range(n_views):
        vol.clear()
        vol.integrate([depths[v]], [cams[v]], [images[v]])
        touched_single += int((vol.tw[..., 1] > 0).sum())
    times = {"single_ms": [], "batched_ms": []}
    timed(single), timed(batched)
    for _ in range(rounds):
        times["single_ms"].append(timed(single))
        times["batched_ms"].append(timed(batched))
    touched = int((vol.tw[..., 1] > 0).sum())
    n = size ** 3
    res = dict(size=size, samples=n, views=n_views, w=w, h=h, touched=touched, touched_single=touched_single, hbm_tbs=hbm_tbs)
    res.update({k: round(float(np.median(t)), 4) for k, t in times.items()})
    res["single_tbs"] = round(touched_single * 40 / (res["single_ms"] * 1e-3) / 1e12, 3)
    res["batched_tbs"] = round(touched * 40 / (res["batched_ms"] * 1e-3) / 1e12, 3)
    res["single_swept_tbs"] = round((n_views * n + touched_single) * 20 / (res["single_ms"] * 1e-3) / 1e12, 3)
    res["batched_swept_tbs"] = round((n + touched) * 20 / (res["batched_ms"] * 1e-3) / 1e12, 3)
    vol.extract_mesh()   # (grows the scratch slot)
    ctx.profile(True)
    ctx.profile_fetch()
    for _ in range(3):
        v, c, t = vol.extract_mesh()
    stages = ctx.profile_fetch()
    ctx.profile(False)
    # (extract_mesh = a count call and an extract call: classify and scan run twice per mesh, emit once)
    for key, stage in (("classify_ms", "TsdfClassify"), ("scan_ms", "TsdfScan"), ("emit_ms", "TsdfEmit")):
        ms, calls = stages[stage]
        res[key] = round(ms / max(calls, 1), 4)
    res["vertices"], res["triangles"] = int(v.shape[0]), int(t.shape[0])
    print(json.dumps(res), flush=True)
    ctx.sync()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="the HBM rate the achieved rates are quoted against, TB/s")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        probe(args.child, args.rounds, args.hbm_tbs)
        return
    for size in args.sizes:   # a fresh process per size, each under its own time limit; nothing is started after a failure
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(size), "--rounds", str(args.rounds), "--hbm-tbs", str(args.hbm_tbs)],
                           timeout=args.step_timeout)
        if r.returncode != 0:
            sys.exit("mesh_probe: size %d ended with status %d" % (size, r.returncode))


if __name__ == "__main__":
    main()
