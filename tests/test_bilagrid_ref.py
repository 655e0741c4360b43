"""tests/bilagrid_ref.py against torch: with float64 coordinates the restatement is gsplat's slice — grid_sample(mode="bilinear",
align_corners=True, padding_mode="border") at the pixel centres and the luminance, through the layout mapping grids[k, l, j, i] =
g[j][i][l][k] — and its autograd, to 1e-11 of each entry's L1 mass; the float32 coordinates move it only by their rounding; TV is
the literal loop of gsplat's total_variation_loss and its gradient autograd's; and the masses bound what they are meant to bound."""
import numpy as np
import pytest
import torch

import bilagrid_ref as br

GRIDS = [(16, 16, 8), (3, 4, 2), (5, 6, 1), (1, 1, 3)]   # (Hg, Wg, L)
W, H = 37, 23


def _inputs(shape, seed=11):
    x, v, g = br.case_inputs(W, H, shape, seed)
    return x.astype(np.float64), v.astype(np.float64), g.astype(np.float64)


def _torch_slice(g, x):
    """gsplat's slice in float64: -> (y [H,W,4], the grid tensor in gsplat's layout, the image tensor)."""
    grids = torch.from_numpy(br.to_gsplat(g))[None].requires_grad_(True)   # [1,12,L,Hg,Wg]
    xt = torch.from_numpy(x).requires_grad_(True)
    h, w = x.shape[:2]
    gx = ((torch.arange(w, dtype=torch.float64) + 0.5) / w)[None, :].expand(h, w)
    gy = ((torch.arange(h, dtype=torch.float64) + 0.5) / h)[:, None].expand(h, w)
    rgb = xt[..., :3]
    gz = rgb[..., 0] * 0.299 + rgb[..., 1] * 0.587 + rgb[..., 2] * 0.114
    xyz = (torch.stack([gx, gy, gz], -1) - 0.5) * 2.0
    mats = torch.nn.functional.grid_sample(grids, xyz[None, None], mode="bilinear", align_corners=True, padding_mode="border")
    mats = mats[0, :, 0].permute(1, 2, 0).reshape(h, w, 3, 4)
    y_rgb = (mats[..., :3] * rgb[:, :, None, :]).sum(-1) + mats[..., 3]
    return torch.cat([y_rgb, xt[..., 3:]], -1), grids, xt


@pytest.mark.parametrize("shape", GRIDS)
def test_float64_restatement_is_grid_sample_and_its_autograd(shape):
    x, v, g = _inputs(shape)
    assert (x[..., :3] @ np.array(br.LUM) < 0).any() and (x[..., :3] @ np.array(br.LUM) > 1).any()   # the border rule is exercised
    y_t, grids, xt = _torch_slice(g, x)
    (y_t * torch.from_numpy(v)).sum().backward()
    fwd, bwd = br.slice_grid(g, x, np.float64), br.backward(g, x, v, np.float64)
    assert (np.abs(fwd["y"][..., :3] - y_t.detach().numpy()[..., :3]) <= 1e-11 * fwd["mass_y"]).all()
    assert np.array_equal(fwd["y"][..., 3], x[..., 3])
    assert (np.abs(bwd["v_img"][..., :3] - xt.grad.numpy()[..., :3]) <= 1e-11 * bwd["mass_v"]).all()
    assert np.array_equal(bwd["v_img"][..., 3], v[..., 3])
    vg_t = br.from_gsplat(grids.grad[0].numpy())
    assert vg_t.shape == g.shape and (np.abs(bwd["v_g"] - vg_t) <= 1e-11 * bwd["S"] + 1e-300).all()
    assert np.abs(bwd["v_g"]).max() > 0 and (bwd["S"][~bwd["reached"]] == 0).all()
    if shape[2] > 1:   # the guidance gradient is part of v_img
        assert np.abs(bwd["v_img"][..., :3] - np.einsum("hwrc,hwr->hwc", fwd["A"].reshape(H, W, 3, 4)[..., :3], v[..., :3])).max() > 1e-3


@pytest.mark.parametrize("shape", GRIDS)
def test_float32_coordinates_move_the_result_by_their_rounding_only(shape):
    x, v, g = _inputs(shape)
    a, b = br.slice_grid(g, x, np.float32), br.slice_grid(g, x, np.float64)
    # a coordinate is off by a few 2^-24 of its size (<= 16): the weights move by that much, the matrices by that times their spread
    assert (np.abs(a["y"][..., :3] - b["y"][..., :3]) <= 64 * 2.0 ** -24 * 16 * a["mass_y"]).all()
    c32, c64 = br.coordinates(g.shape, x.astype(np.float32), np.float32), br.coordinates(g.shape, x, np.float64)
    assert c32["tx"].dtype == np.float64 and np.abs(c32["tx"] + c32["i0"] - c64["tx"] - c64["i0"]).max() <= 16 * 2.0 ** -23


def test_identity_grid_returns_its_input():
    x, v, _ = _inputs((16, 16, 8))
    g = br.identity_grid(16, 16, 8)
    assert np.abs(br.slice_grid(g, x)["y"] - x).max() <= 1e-15
    b = br.backward(g, x, v)
    assert np.abs(b["v_img"] - v).max() <= 1e-15   # every level holds the same matrix: dA/dfz = 0


def _tv_literal(grids):
    """gsplat's total_variation_loss on [B,12,L,Hg,Wg], with an axis of one vertex skipped (its count is zero)."""
    tv = 0.0
    for i in range(2, grids.dim()):
        n = grids.shape[i]
        if n < 2:
            continue
        x1 = grids.index_select(i, torch.arange(1, n))
        x2 = grids.index_select(i, torch.arange(0, n - 1))
        count = 1
        for s in x1.shape[1:]:
            count *= s
        tv = tv + torch.pow(x1 - x2, 2).sum() / count
    return tv / grids.shape[0]


@pytest.mark.parametrize("shape", GRIDS)
def test_total_variation_is_gsplats_and_its_gradient_autograds(shape):
    _, _, g = _inputs(shape, seed=5)
    grids = torch.from_numpy(br.to_gsplat(g))[None].requires_grad_(True)
    tv_t = _tv_literal(grids)
    tv_t.backward()
    tv, grad = br.total_variation(g)
    assert tv > 0 and abs(tv - float(tv_t.detach())) <= 1e-12 * tv
    want = br.from_gsplat(grads := grids.grad[0].numpy())
    assert grads.shape == (12, shape[2], shape[0], shape[1])
    assert np.abs(grad - want).max() <= 1e-12 * np.abs(want).max()
    assert br.total_variation(br.identity_grid(*shape))[0] == 0.0


def test_adam_step_is_plain_adam():
    rng = np.random.default_rng(3)
    p, g = rng.normal(size=24), rng.normal(size=24)
    q, m1, m2, t = br.adam_step(p, np.zeros(24), np.zeros(24), 0, g, 2e-3)
    assert t == 1 and np.allclose(q, p - 2e-3 * np.sign(g), rtol=0, atol=1e-12)
    assert np.allclose(m1, 0.1 * g) and np.allclose(m2, 0.001 * g * g)
    q0, _, _, _ = br.adam_step(p, np.zeros(24), np.zeros(24), 0, np.zeros(24), 2e-3)
    assert np.array_equal(q0, p)   # a vertex no pixel reaches stays where it is
