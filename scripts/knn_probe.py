"""Developer tool (GPU box): what compute_knn_scales (brush-train/src/splat_init.rs:179-216) costs on the device, bh_knn_log_scales,
at 100 k, 1 M and 10 M points of three clouds (tests/knn_ref.py: uniform cube, surface-like = noisy planes + sphere shells, a dense
cluster + 1 % far outliers at 10^3 x its scale).  Per case it prints one JSON line:
  * ms: the call's device-event time (warmed, median of --reps >= 5 calls; the call blocks on its bounds readback, so this is
    the wall time of the whole kNN: rank sorts, Morton sort, bounds, tree, query);
  * pairs_per_point: distance evaluations / N (a brute force is N);
  * exact: d1 / d2 of --check sampled queries bit-identical to a GPU brute force (8 candidates per query by f32 squared distance,
    elementwise torch in chunks, then the f32 distances recomputed on the host in the reference's order), log-scales <= 2 ulp;
  * ckdtree_ms: scipy.spatial.cKDTree(points).query(points, k=3, workers=16) — a STAND-IN for the reference's host ball tree
    (ball-tree crate + rayon), which cannot be built here; tree build + query, best of 2 (one run at 10 M).
    python scripts/knn_probe.py [--sizes 100000,1000000,10000000] [--kinds uniform,surface,outliers] [--reps 7] [--no-ckdtree]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import brush_amd as ba   # noqa: E402
import knn_ref   # noqa: E402


def candidates(pos_dev, q_idx, k=8, chunk=32):
    out = []
    px, py, pz = pos_dev[:, 0], pos_dev[:, 1], pos_dev[:, 2]
    for a in range(0, len(q_idx), chunk):
        qi = torch.as_tensor(q_idx[a:a + chunk], device=pos_dev.device, dtype=torch.int64)
        q = pos_dev[qi]
        dx = q[:, 0:1] - px[None, :]
        dy = q[:, 1:2] - py[None, :]
        dz = q[:, 2:3] - pz[None, :]
        s = (dx * dx + dy * dy) + dz * dz
        s[torch.arange(qi.numel(), device=s.device), qi] = float("inf")
        out.append(torch.topk(s, k, dim=1, largest=False).indices.cpu().numpy())
        del dx, dy, dz, s
    return np.concatenate(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,10000000")
    ap.add_argument("--kinds", default="uniform,surface,outliers")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--check", type=int, default=4096)
    ap.add_argument("--no-ckdtree", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = ba.get_context()
    for n in [int(s) for s in args.sizes.split(",")]:
        for kind in args.kinds.split(","):
            pos = knn_ref.cloud(kind, n, seed=1)
            tr = torch.zeros((n, 10), dtype=torch.float32, device="cuda")
            tr[:, :3] = torch.from_numpy(pos).cuda()
            tr[:, 3] = 1.0
            sp = ba.Splats(tr, torch.zeros((n, 1, 3), device="cuda"), torch.zeros(n, device="cuda"))
            ls, nn, st = ba.knn_log_scales(sp, ctx, return_distances=True, return_stats=True)   # warm-up (arena, code objects)
            times = []
            for _ in range(max(args.reps, 5)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ba.knn_log_scales(sp, ctx)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            rng = np.random.default_rng(3)
            q = np.sort(rng.choice(n, min(args.check, n), replace=False))
            cand = candidates(torch.from_numpy(pos).cuda(), q)
            two = np.sort(knn_ref.sq_dist_f32(pos[q][:, None, :], pos[cand]), axis=1)[:, :2]
            want = np.sqrt(two).astype(np.float32)
            got = nn.cpu().numpy()[q]
            upper = np.float32(knn_ref.median_size(pos) * np.float32(0.1))
            want_ls = np.log(knn_ref.clamped_dist(want, upper).astype(np.float64)).astype(np.float32)
            exact = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32))) and int(knn_ref.ulp_diff(ls[:, 0].cpu().numpy()[q], want_ls).max()) <= 2
            row = {"n": n, "kind": kind, "ms": round(float(np.median(times)), 3), "ms_min": round(float(np.min(times)), 3),
                   "pairs_per_point": round(st["pairs_tested"] / n, 1), "exact": exact, "checked": int(q.size)}
            if not args.no_ckdtree:
                from scipy.spatial import cKDTree
                best = float("inf")
                for _ in range(2 if n <= 1_000_000 else 1):
                    t0 = time.perf_counter()
                    cKDTree(pos).query(pos, k=3, workers=16)
                    best = min(best, time.perf_counter() - t0)
                row["ckdtree_ms_standin"] = round(best * 1e3, 1)
            print(json.dumps(row), flush=True)
            del sp, tr, ls, nn
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
