"""Developer tool (GPU box): what a sparse TSDF volume (include/brush_hip_sparse_mesh.h) costs next to the dense one of
the same tree.  The scene is scripts/mesh_probe.py's: eight 1920x1080 views of an analytic sphere of radius 0.7 in the box [-1, 1]^3,
with colour.  Per virtual size one JSON line:
  * blocks / block_share: allocated blocks and their share of the grid's; sparse_bytes (pool + keys + bits + rank) against dense_bytes
    (20 per sample);
  * mark_ms (eight views in one call), commit_ms (dilate 1, with its readback);
  * sparse_single_ms / sparse_batched_ms against dense_single_ms / dense_batched_ms: eight single-view integrate calls and one
    eight-view call on a cleared volume, the four alternated inside a round (device events, medians of `--rounds` rounds);
  * classify_ms / scan_ms / emit_ms of both extractions (the library's stage events), and the meshes' counts.
A size above 1290 has no dense volume: the dense figures are left out.  Each size runs in a child process of its own under
`--step-timeout` seconds; the first failure ends the run.
    python scripts/sparse_mesh_probe.py [--sizes 256 512 2048] [--rounds 5]
"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def probe(size, rounds):
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
    with_dense = size ** 3 <= 2 ** 31 - 1
    sparse = ba.SparseTsdfVolume((-1.0, -1.0, -1.0), voxel, (size, size, size), ctx=ctx)
    dense = ba.TsdfVolume((-1.0, -1.0, -1.0), voxel, (size, size, size), ctx=ctx) if with_dense else None
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
        d = torch.stack([(xs + 0.5 - cam.cx) / cam.fx, (ys + 0.5 - cam.cy) / cam.fy, torch.ones_like(xs)], dim=-1)
        c_cam = torch.tensor(t, device=dev)
        a, b, cc = (d * d).sum(-1), (d * c_cam).sum(-1), float(t @ t) - 0.49
        disc = b * b - a * cc
        depths.append(torch.where(disc > 0, (b - disc.clamp(min=0).sqrt()) / a, torch.zeros_like(a)).float().contiguous())
        img = torch.rand((h, w, 4), device=dev)
        img[..., 3] = 1.0
        images.append(img)
        cams.append(cam)

    def event_ms(fn, before=None):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    times = {"mark_ms": [], "commit_ms": []}
    blocks = 0
    for _ in range(rounds + 1):   # (the first round warms up)
        times["mark_ms"].append(event_ms(lambda: sparse.mark(depths, cams, images), sparse.mark_clear)[0])
        ms, blocks = event_ms(sparse.commit)
        times["commit_ms"].append(ms)
    times = {k: t[1:] for k, t in times.items()}

    def runs(vol):
        def single():
            for v in range(n_views):
                vol.integrate([depths[v]], [cams[v]], [images[v]])
        return single, lambda: vol.integrate(depths, cams, images)

    variants = {"sparse": (sparse,) + runs(sparse)}
    if with_dense:
        variants["dense"] = (dense,) + runs(dense)
    for name, (vol, single, batched) in variants.items():
        times[name + "_single_ms"], times[name + "_batched_ms"] = [], []
        event_ms(single, vol.clear), event_ms(batched, vol.clear)
    for _ in range(rounds):
        for name, (vol, single, batched) in variants.items():
            times[name + "_single_ms"].append(event_ms(single, vol.clear)[0])
            times[name + "_batched_ms"].append(event_ms(batched, vol.clear)[0])
    total_blocks = sparse.block_dims[0] * sparse.block_dims[1] * sparse.block_dims[2]
    res = dict(size=size, samples=size ** 3, views=n_views, w=w, h=h, blocks=blocks, block_share=round(blocks / total_blocks, 5),
               sparse_bytes=blocks * (512 * 20 + 4) + 8 * sparse.n_words, dense_bytes=20 * size ** 3,
               sparse_observed=int((sparse.tw[..., 1] > 0).sum()))
    if with_dense:
        res["dense_observed"] = int((dense.tw[..., 1] > 0).sum())
    res.update({k: round(float(np.median(t)), 4) for k, t in times.items()})
    for name, (vol, _, _) in variants.items():
        prefix = "SpTsdf" if name == "sparse" else "Tsdf"
        vol.extract_mesh()   # (grows the scratch slot)
        ctx.profile(True)
        ctx.profile_fetch()
        for _ in range(3):
            v, c, t = vol.extract_mesh()
        stages = ctx.profile_fetch()
        ctx.profile(False)
        # (extract_mesh = a count call and an extract call: classify and scan run twice per mesh, emit once)
        for key, stage in (("classify_ms", "Classify"), ("scan_ms", "Scan"), ("emit_ms", "Emit")):
            ms, calls = stages[prefix + stage]
            res[name + "_" + key] = round(ms / max(calls, 1), 4)
        res[name + "_vertices"], res[name + "_triangles"] = int(v.shape[0]), int(t.shape[0])
    print(json.dumps(res), flush=True)
    ctx.sync()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 2048])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        probe(args.child, args.rounds)
        return
    for size in args.sizes:   # a fresh process per size, each under its own time limit; nothing is started after a failure
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(size), "--rounds", str(args.rounds)], timeout=args.step_timeout)
        if r.returncode != 0:
            sys.exit("sparse_mesh_probe: size %d ended with status %d" % (size, r.returncode))


if __name__ == "__main__":
    main()
