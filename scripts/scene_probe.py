"""Developer tool (GPU box): what bh_splats_transform (include/brush_hip_scene.h) costs next to its yardstick, a
device-to-device copy of the same bytes — the kernel reads and writes every byte of transforms, SH and min_scale once, as the copy does.
Cases: 1 M and 6 M splats, SH degree 0 and 3, out of place and in place.  Prints one JSON line per case:
  * bytes: what is read (and written again): N * (40 + 12 C + 4);
  * transform_ms / transform_tbs: the call, and (read + written bytes) / time;
  * copy_ms / copy_tbs: three hipMemcpyAsync device-to-device of the same buffers (torch's copy_), the same measure;
  * ratio: transform_ms / copy_ms.
Device events, medians of `--rounds` rounds of `--reps` calls each; kernel and copy alternate inside each round, in the same process.
Each case runs in a child process of its own under `--step-timeout` seconds; the first failure ends the run.
    python scripts/scene_probe.py [--sizes 1000000 6000000] [--degrees 0 3] [--reps 10] [--rounds 7]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import brush_amd as ba   # noqa: E402


def timed(fn, reps):
    """mean device ms per call over `reps` back-to-back calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def probe(n, degree, in_place, reps, rounds):
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    ctx = ba.Context(dev)
    c = (degree + 1) ** 2
    gen = torch.Generator(device=dev).manual_seed(n + degree)
    # (buffers filled on the device: the values do not change the time, and 6 M x SH 3 rows would take a while from numpy)
    src = ba.Splats(torch.randn((n, 10), device=dev, generator=gen), torch.randn((n, c, 3), device=dev, generator=gen),
                    torch.randn((n,), device=dev, generator=gen), device=dev, min_scale=torch.rand((n,), device=dev, generator=gen))
    dst = src.clone()
    # a rotation by a small angle and a scale next to 1: 10 x rounds x reps in-place applications leave the values finite
    T = ba.SceneTransform.from_quat((1.0, 0.01, -0.02, 0.015), (0.01, -0.02, 0.03), 1.001)
    rec, lib, h = T.as_struct(), ctx.lib, ctx._h
    ins = (src.transforms, src.sh_coeffs, src.min_scale)
    outs = ins if in_place else (dst.transforms, dst.sh_coeffs, dst.min_scale)
    ptrs = [t.data_ptr() for t in ins + outs]

    def transform():
        ctx.check(lib.bh_splats_transform(h, rec, n, c, *ptrs))

    def copy():
        for a, b in zip((dst.transforms, dst.sh_coeffs, dst.min_scale), ins):
            a.copy_(b)

    for fn in (transform, copy):
        fn()
    torch.cuda.synchronize()
    t_ms, c_ms = [], []
    for _ in range(rounds):
        t_ms.append(timed(transform, reps))
        c_ms.append(timed(copy, reps))
    nbytes = n * (40 + 12 * c + 4)
    tm, cm = float(np.median(t_ms)), float(np.median(c_ms))
    print(json.dumps(dict(n=n, sh_degree=degree, in_place=bool(in_place), bytes=nbytes, transform_ms=round(tm, 4), transform_tbs=round(2 * nbytes / tm * 1e-9, 3),
                          copy_ms=round(cm, 4), copy_tbs=round(2 * nbytes / cm * 1e-9, 3), ratio=round(tm / cm, 3),
                          transform_rounds=[round(x, 4) for x in t_ms], copy_rounds=[round(x, 4) for x in c_ms])), flush=True)
    ctx.sync()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000000, 6000000])
    ap.add_argument("--degrees", type=int, nargs="+", default=[0, 3])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--child", type=int, nargs=3, default=None, help=argparse.SUPPRESS)   # n, degree, in place
    args = ap.parse_args()
    if args.child:
        probe(args.child[0], args.child[1], args.child[2], args.reps, args.rounds)
        return
    for n in args.sizes:
        for degree in args.degrees:
            for in_place in (0, 1):   # a fresh process per case, each under its own time limit; nothing is started after a failure
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(degree), str(in_place), "--reps", str(args.reps),
                                    "--rounds", str(args.rounds)], timeout=args.step_timeout)
                if r.returncode != 0:
                    sys.exit("scene_probe: n %d degree %d in_place %d ended with status %d" % (n, degree, in_place, r.returncode))


if __name__ == "__main__":
    main()
