"""tests/normal_loss_ref.py against itself (no GPU): its gradients are torch.autograd's in float64, a plane facing the camera with
N = A u gives l = A (1 - A) at every valid pixel, and borders and non-finite or <= 0 depths invalidate exactly the stencils that read
them."""
import numpy as np
import torch

import normal_loss_ref as nl

FX, FY, CX, CY = 31.0, 29.0, 13.2, 9.7


def _maps(seed=7, h=19, w=27):
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    depth = 4.0 + 0.05 * xs - 0.03 * ys + rng.uniform(-0.05, 0.05, (h, w))
    normal = rng.uniform(-1.0, 1.0, (h, w, 3))
    alpha = rng.uniform(0.0, 1.0, (h, w))
    return normal, depth, alpha


def test_gradients_are_autograds():
    normal, depth, alpha = _maps()
    depth[5, 8] = 0.0
    depth[11, 20] = np.nan
    depth[3, 3] = -1.0
    weight = 0.37
    r = nl.value_and_grad(normal, depth, alpha, FX, FY, CX, CY, weight)
    nt = torch.tensor(normal, requires_grad=True)
    dt = torch.tensor(depth, requires_grad=True)
    at = torch.tensor(alpha, requires_grad=True)
    loss, valid, _ = nl.loss_terms(nt, dt, at, FX, FY, CX, CY, weight)
    loss.backward()
    assert at.grad is None   # alpha is a constant of the term
    assert r["count"] == int(valid.sum()) and 0 < r["count"] < (depth.shape[0] - 2) * (depth.shape[1] - 2)
    assert abs(r["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    want_d = torch.nan_to_num(dt.grad).numpy()
    assert np.abs(want_d).max() > 0 and np.abs(nt.grad.numpy()).max() > 0
    assert np.abs(r["v_normal"] - nt.grad.numpy()).max() <= 1e-10 * np.abs(nt.grad.numpy()).max()
    assert np.abs(r["v_depth"] - want_d).max() <= 1e-10 * np.abs(want_d).max()
    # the holes take no gradient themselves: no valid stencil reads them
    for (y, x) in ((5, 8), (11, 20), (3, 3)):
        assert r["v_depth"][y, x] == 0.0


def test_a_plane_facing_the_camera():
    h, w = 9, 12
    depth = np.full((h, w), 3.0)
    rng = np.random.default_rng(1)
    alpha = rng.uniform(0.1, 1.0, (h, w))
    u = np.zeros((h, w, 3))
    u[..., 2] = -1.0   # c = gy x gx points at the camera
    r = nl.value_and_grad(alpha[..., None] * u, depth, alpha, FX, FY, CX, CY, 1.0)
    valid = np.zeros((h, w), bool)
    valid[1:-1, 1:-1] = True
    assert np.array_equal(r["valid"], valid) and r["count"] == (h - 2) * (w - 2)
    assert np.abs(r["u"][valid] - u[valid]).max() <= 1e-12
    want = nl.constant(1.0, h * w) * float((alpha * (1.0 - alpha))[valid].sum())
    assert abs(r["loss"] - want) <= 1e-12 * want
    assert not r["v_normal"][~valid].any()


def test_borders_and_bad_depths_invalidate_the_stencils_that_read_them():
    normal, depth, alpha = _maps(9, 11, 14)
    h, w = depth.shape
    bad = {(4, 5): np.nan, (7, 9): np.inf, (2, 10): 0.0, (8, 3): -2.0}
    for (y, x), v in bad.items():
        depth[y, x] = v
    want = np.ones((h, w), bool)
    want[0, :] = want[-1, :] = want[:, 0] = want[:, -1] = False
    for (y, x) in bad:
        for (dy, dx) in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
            want[y + dy, x + dx] = False
    r = nl.value_and_grad(normal, depth, alpha, FX, FY, CX, CY, 0.5)
    assert np.array_equal(r["valid"], want) and r["count"] == int(want.sum())
    assert np.isfinite(r["v_depth"]).all() and np.isfinite(r["v_normal"]).all() and np.isfinite(r["loss"])
    assert not r["v_normal"][~want].any()
    # a diagonal neighbour of a hole keeps its stencil
    assert r["valid"][5, 6] and r["valid"][3, 4]
    # too small for any stencil, and no term at all
    tiny = nl.value_and_grad(normal[:2, :7], np.ones((2, 7)), alpha[:2, :7], FX, FY, CX, CY, 1.0)
    assert tiny["count"] == 0 and tiny["loss"] == 0.0 and not tiny["v_depth"].any() and not tiny["v_normal"].any()
    for weight in (0.0, -1.0, float("nan")):
        off = nl.value_and_grad(normal, depth, alpha, FX, FY, CX, CY, weight)
        assert off["count"] == 0 and off["loss"] == 0.0 and not off["v_depth"].any() and not off["v_normal"].any()
