"""Developer tool (GPU box): what bh_lift_accumulate (include/brush_hip_lift.h) costs on the 1 M-splat 1080p bench
scene with one saved forward, next to the only route the library had to the same sums — bh_render_backward_features_saved with
v_output = NULL and a one-hot v_map [H,W,L] — and to the bh_render_features forward at C = L, the floor of a pass over the same lists.
Cases: L = 1 without a label map, L = 2 and L = 16 with blocky maps (64 x 64-pixel blocks: one label per tile), each with and without
the two statistics, and L = 16 with (x + 3 y) mod L (sixteen labels in every tile: four passes over its lists).  Prints one JSON line per case:
  * lift_ms, backward_ms, forward_ms: device ms per call; ratio = lift_ms / backward_ms;
  * vote_atomics: 64-bit atomic adds one call issues = the (tile, splat) pairs with a non-zero sum, counted exactly by lifting once
    with a label map that gives every tile of a 16 x 16-tile neighbourhood its own label (L = 256) and counting the non-zero votes
    (no splat of this scene spans 256 pixels: checked against the pixel counts); stat_atomics: two 32-bit ones per such pair;
  * atomic_gbs: vote_atomics * 8 bytes / lift time — the rate this kernel sustains, not the chip's ceiling.
Device events, medians of `--rounds` rounds of `--reps` calls each; the lift and the backward alternate inside each round, in the same
process.  Each case runs in a child process of its own under `--step-timeout` seconds; the first failure ends the run.
    python scripts/lift_probe.py [--labels 1 2 16] [--reps 10] [--rounds 7]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
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


def blocky(w, h, L, block=64):
    yy, xx = np.mgrid[0:h, 0:w]
    side = int(np.ceil(np.sqrt(L)))
    return (((xx // block) % side + side * ((yy // block) % side)) % L).astype(np.uint8)


def interleaved(w, h, L):
    """(x + 3 y) mod L: every tile holds min(L, 16) labels — ceil(L / 4) passes over its lists"""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx + 3 * yy) % L).astype(np.uint8)


def probe(L, stats, count, reps, rounds, mixed=0):
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    ctx = ba.Context(dev)
    sc, w, h = synth.config_scene("1m_1080p")
    cp = synth.default_camera_params(w, h)
    cam = ba.Camera(position=cp["pos"], rotation=cp["rot_xyzw"], fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    n = spl.num_splats()
    node = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, retain=True)
    lab_np = None if L == 1 else (interleaved(w, h, L) if mixed else blocky(w, h, L))
    lab = None if lab_np is None else torch.from_numpy(lab_np).to(dev)
    acc = ba.LiftAccumulator(n, L, dev, stats=bool(stats), ctx=ctx)
    lib, hd, out = ctx.lib, ctx._h, C.byref(node.out)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def lift():
        ctx.check(lib.bh_lift_accumulate(hd, out, p(lab), L, p(acc.votes), p(acc.max_weight), p(acc.pixel_count)))

    # the parent's route: a feature-only backward with a one-hot cotangent; every output preallocated
    onehot = torch.zeros((h, w, L), device=dev)
    onehot.scatter_(2, (torch.zeros((h, w), dtype=torch.int64, device=dev) if lab is None else lab.long()).unsqueeze(-1), 1.0)
    feats = torch.zeros((n, L), device=dev)
    r_t, r_o = node._folded
    c = spl.sh_coeffs.shape[1]
    v_t, v_sh, v_op, v_rf, v_f = (torch.empty(s, device=dev) for s in ((n, 10), (n, c, 3), (n,), (n,), (n, L)))

    def backward():
        ctx.check(lib.bh_render_backward_features_saved(hd, out, None, p(feats), L, p(onehot), p(r_t), p(spl.sh_coeffs), p(r_o), p(v_t), p(v_sh), p(v_op),
                                                        p(v_rf), p(v_f)))

    fmap = torch.empty((h, w, L), device=dev)

    def forward():
        ctx.check(lib.bh_render_features(hd, out, p(feats), L, p(fmap)))

    for fn in (lift, backward, forward):
        fn()
    torch.cuda.synchronize()
    # the two routes agree (the tables were zero before the one warm-up call)
    got = acc.weights()
    err = float((got - v_f).abs().max()) / max(float(v_f.abs().max()), 1e-30)
    l_ms, b_ms, f_ms = [], [], []
    for _ in range(rounds):
        l_ms.append(timed(lift, reps))
        b_ms.append(timed(backward, reps))
        f_ms.append(timed(forward, reps))
    res = dict(labels=L, stats=bool(stats), label_map="none" if L == 1 else ("interleaved" if mixed else "blocks"), isect=int(node.out.num_intersections), listed=int(node.out.num_listed_splats),
               lift_ms=round(float(np.median(l_ms)), 4), backward_ms=round(float(np.median(b_ms)), 4), forward_ms=round(float(np.median(f_ms)), 4),
               rel_diff_of_the_routes=float("%.3e" % err), lift_rounds=[round(x, 4) for x in l_ms], backward_rounds=[round(x, 4) for x in b_ms])
    res["ratio"] = round(res["lift_ms"] / res["backward_ms"], 3)
    if count and not mixed:
        # every tile of a 16 x 16-tile neighbourhood gets its own label: a non-zero votes entry IS one (tile, splat) atomic
        yy, xx = np.mgrid[0:h, 0:w]
        tiles = torch.from_numpy((((xx // 16) % 16) + 16 * ((yy // 16) % 16)).astype(np.uint8)).to(dev)
        big = ba.LiftAccumulator(n, 256, dev, stats=True, ctx=ctx).add(node, tiles)
        pairs = int(torch.count_nonzero(big.votes))
        res["vote_atomics"] = pairs
        res["stat_atomics"] = 2 * pairs if stats else 0
        res["pixel_terms"] = int(big.pixel_count.sum(dtype=torch.int64))
        res["max_pixels_of_a_splat"] = int(big.pixel_count.max())   # (a footprint of 256 x 256 pixels would be 65536)
        res["atomic_gbs"] = round(pairs * 8 / (res["lift_ms"] * 1e-3) * 1e-9, 3)
    print(json.dumps(res), flush=True)
    node.release()
    ctx.sync()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--labels", type=int, nargs="*", default=[1, 2, 16])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=180)
    ap.add_argument("--interleaved", type=int, nargs="*", default=[16], help="label counts also timed with (x + 3 y) mod L: several labels per tile")
    ap.add_argument("--child", type=int, nargs=4, default=None, help=argparse.SUPPRESS)   # L, stats, count the atomics, interleaved map
    args = ap.parse_args()
    if args.child:
        probe(args.child[0], args.child[1], args.child[2], args.reps, args.rounds, args.child[3])
        return
    cases = [(L, stats, 0) for L in args.labels for stats in (0, 1)] + [(L, 0, 1) for L in args.interleaved if L > 1]
    for L, stats, mixed in cases:   # a fresh process per case, each under its own time limit; nothing is started after a failure
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(L), str(stats), "1", str(mixed), "--reps", str(args.reps),
                            "--rounds", str(args.rounds)], timeout=args.step_timeout)
        if r.returncode != 0:
            sys.exit("lift_probe: L %d stats %d interleaved %d ended with status %d" % (L, stats, mixed, r.returncode))


if __name__ == "__main__":
    main()
