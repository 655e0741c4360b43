#!/usr/bin/env python3
"""Developer tool (GPU): the fused loss pair's outputs from seeded inputs, to compare two builds bit for bit.
   BRUSH_HIP_LIB=<a build's libbrush_hip.so> python scripts/loss_fused_bits.py save a.npz
   python scripts/loss_fused_bits.py save b.npz             (the in-tree build)
   python scripts/loss_fused_bits.py compare a.npz b.npz    (no GPU needed; exit status 1 if anything differs)
Shapes: the three of tests/test_gpu_loss_fused_edges.py and 1080 x 1920, each with that test's three
(background, mask, alpha weight) combinations."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [(33, 18), (32, 256), (70, 260), (1080, 1920)]
COMBOS = [(None, False, 0.0), ((0.3, 0.5, 0.2), False, 0.1), (None, True, 0.0)]


def save(path):
    import torch
    import brush_amd as ba
    dev = torch.device("cuda:0")
    out = {}
    for h, w in SHAPES:
        rng = np.random.default_rng(h * 7 + w)
        rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint32)
        gt = (rgba[..., 0] | (rgba[..., 1] << 8) | (rgba[..., 2] << 16) | (rgba[..., 3] << 24)).astype(np.uint32)
        img = rng.uniform(-0.1, 1.1, (h, w, 4)).astype(np.float32)
        gt_t = torch.from_numpy(gt.view(np.int32)).to(dev)
        img_t = torch.from_numpy(img).to(dev)
        for n, (bg, mask, alpha_w) in enumerate(COMBOS):
            loss, v_out = ba.image_loss_value_and_grad(img_t, gt_t, 0.8, -0.2, composite_bg=bg, mask=mask, alpha_weight=alpha_w)
            out["%dx%d_%d_loss" % (h, w, n)] = loss.detach().cpu().numpy().reshape(1).copy()
            out["%dx%d_%d_v_output" % (h, w, n)] = v_out.detach().cpu().numpy().copy()
    np.savez(path, **out)
    print("saved %d arrays to %s (library: %s)" % (len(out), path, os.environ.get("BRUSH_HIP_LIB", "in-tree")))


def compare(a, b):
    x, y = np.load(a), np.load(b)
    assert sorted(x.files) == sorted(y.files)
    bad = 0
    for k in sorted(x.files):
        u, v = x[k], y[k]
        same = u.shape == v.shape and u.tobytes() == v.tobytes()
        if not same:
            bad += 1
            d = np.abs(u.astype(np.float64) - v.astype(np.float64))
            print("%-28s DIFFERS: %d of %d words, max |diff| %.3g, max |value| %.3g" % (k, int((u.view(np.uint32) != v.view(np.uint32)).sum()), u.size, d.max(), np.abs(u).max()))
    print("%s vs %s: %d arrays, %s" % (a, b, len(x.files), "identical" if not bad else "%d differ" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "save":
        save(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
