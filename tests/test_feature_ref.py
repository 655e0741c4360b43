"""tests/feature_ref.py pinned without a GPU: its RGBA is oracle/autograd_ref.render's exactly (pinhole, a fisheye model, Mip), a
feature map of ones is the image's alpha and one of the splats' colours its rgb, the two ways to its gradient (through the map,
through the per-splat weights) agree with each other and with central finite differences, and the two loss restatements' gradients
agree with central finite differences of their values."""
import numpy as np
import pytest
import torch

from oracle import autograd_ref
import depth_ref
import feature_ref
import util

CASES = [("pinhole", False), ("kb4", False), ("pinhole", True)]


def _case(model, seed=3, n=6):
    sc = util.random_scene(seed, n)
    camp = dict(util.random_camera(seed))
    if model != "pinhole":
        camp["model"], camp["dist"] = util.REF_LENSES[model]
    return sc, camp


def _tensors(sc):
    return [torch.tensor(np.asarray(sc[k], np.float64), requires_grad=True) for k in ("transforms", "sh", "raw_opac")]


def _features(n, c, seed=1):
    return torch.tensor(np.random.default_rng(seed).normal(0.0, 1.0, (n, c)), requires_grad=True)


@pytest.mark.parametrize("model,mip", CASES)
def test_rgba_is_autograd_refs_exactly(model, mip):
    w = h = 40
    for seed in (3, 7):
        sc, camp = _case(model, seed, 2 + seed % 7)
        intr = depth_ref.intrinsics(camp, w, h)
        tr, sh, op = _tensors(sc)
        bg = (0.1, 0.3, 0.2)
        a = autograd_ref.render(tr, sh, op, camp, w, h, bg, intr, mip)
        out = feature_ref.render(tr, sh, op, _features(tr.shape[0], 5), camp, w, h, bg, intr, mip)
        assert torch.equal(a, out["img"])
        assert torch.equal(out["alpha"], a[..., 3])
        # the tie margins are depth_ref's: its tie mask applies
        d = depth_ref.render(tr, sh, op, camp, w, h, bg, intr, mip)
        assert torch.equal(depth_ref.tie_mask(out, "accumulated"), depth_ref.tie_mask(d, "accumulated"))
    sc, camp = util.base_scene(), util.STD_CAM
    tr, sh, op = _tensors(sc)
    assert torch.equal(autograd_ref.render(tr, sh, op, camp, 32, 32), feature_ref.render(tr, sh, op, _features(tr.shape[0], 2), camp, 32, 32)["img"])


@pytest.mark.parametrize("model,mip", CASES)
def test_the_map_is_the_blend_of_the_rows(model, mip):
    """Channels are independent blends with the image's weights: ones give alpha, z gives depth_ref's accumulated depth, a negative
    row is not clamped, and the weights add up to the map."""
    w = h = 40
    sc, camp = _case(model)
    tr, sh, op = _tensors(sc)
    intr = depth_ref.intrinsics(camp, w, h)
    d = depth_ref.render(tr, sh, op, camp, w, h, intrinsics=intr, mip=mip)
    rows = torch.stack([torch.ones_like(d["z"]), d["z"].detach(), -2.0 * torch.ones_like(d["z"])], -1)
    out = feature_ref.render(tr, sh, op, rows, camp, w, h, intrinsics=intr, mip=mip)
    f = out["feat"].detach()
    assert float(out["alpha"].detach().max()) > 0.1
    assert float((f[..., 0] - out["alpha"].detach()).abs().max()) <= 1e-12
    assert torch.equal(f[..., 1], d["acc"].detach())
    assert float((f[..., 2] + 2.0 * f[..., 0]).abs().max()) <= 1e-12 and float(f[..., 2].min()) < -0.2
    again = feature_ref.render(tr, sh, op, rows, camp, w, h, intrinsics=intr, mip=mip, map_grad=False)
    assert torch.equal(again["feat"], f) and not again["feat"].requires_grad
    assert float((torch.einsum("nhw,nc->hwc", out["vis"].detach(), rows) - f).abs().max()) <= 1e-12


@pytest.mark.parametrize("model,mip", CASES)
def test_autograd_gradient_agrees_with_central_differences(model, mip):
    """Smooth cut-off (the reference's finite-difference pass), comp_is_constant=False in Mip mode: the true derivative of the
    forward, which is what a finite difference measures.  And the gradient through the per-splat weights (gradients(): what the
    GPU tests compare against) is the one through the map."""
    w = h = 24
    c = 5
    sc, camp = _case(model, 5, 4)
    intr = depth_ref.intrinsics(camp, w, h)
    rng = np.random.default_rng(11)
    v = rng.uniform(-1.0, 1.0, (h, w, c)) / (h * w)
    ft = _features(4, c)

    def value(tr, sh, op, ft):
        return (feature_ref.render(tr, sh, op, ft, camp, w, h, intrinsics=intr, mip=mip, smooth=True, comp_is_constant=False)["feat"] * torch.tensor(v)).sum()
    tr, sh, op = _tensors(sc)
    value(tr, sh, op, ft).backward()
    eps = 1e-6
    for name, t, g, picks in (("tr", tr, tr.grad, [(0, 0), (0, 2), (1, 1), (2, 4), (1, 8), (3, 2)]), ("op", op, op.grad, [(0,), (2,)]),
                              ("ft", ft, ft.grad, [(0, 0), (1, 4), (3, 2)])):
        for idx in picks:
            def pert(d):
                x = t.detach().clone()
                x[idx] += d
                x.requires_grad_(True)
                args = {"tr": (x, sh, op, ft), "op": (tr, sh, x, ft), "ft": (tr, sh, op, x)}[name]
                return float(value(*args).detach())
            num = (pert(eps) - pert(-eps)) / (2 * eps)
            an = float(g[idx])
            assert abs(num - an) <= 1e-6 * max(abs(num), abs(an)) + 1e-9, (name, idx, num, an)
    assert float(tr.grad[:, :3].abs().max()) > 0 and float(ft.grad.abs().max()) > 0
    # the two routes, on the forward the GPU tests use (hard cut-off, comp constant)
    tr, sh, op = _tensors(sc)
    ft2 = ft.detach().clone().requires_grad_(True)
    (feature_ref.render(tr, sh, op, ft2, camp, w, h, intrinsics=intr, mip=mip)["feat"] * torch.tensor(v)).sum().backward()
    _, g_tr, g_sh, g_op, g_ft = feature_ref.gradients(sc, ft.detach().numpy(), camp, w, h, v, intrinsics=intr, mip=mip)
    for a, b in ((tr.grad.numpy(), g_tr), (op.grad.numpy(), g_op), (ft2.grad.numpy(), g_ft)):
        assert np.abs(a - b).max() <= 1e-12 * max(np.abs(a).max(), 1e-30)
    assert not g_sh.any()


def _fd(value, x, idx, eps):
    a, b = x.copy(), x.copy()
    a[idx] += eps
    b[idx] -= eps
    return (value(a) - value(b)) / (2 * eps)


def test_l1_restatement():
    rng = np.random.default_rng(5)
    h, w, c = 6, 7, 4
    f = rng.normal(0, 1, (h, w, c)).astype(np.float32)
    t = rng.normal(0, 1, (h, w, c)).astype(np.float32)
    t[1, 2, 3] = np.nan
    t[4, 0, 0] = np.inf
    t[2, 2] = f[2, 2]   # exact ties: sign(0) = 0
    loss, count, v = feature_ref.l1_loss(f, t, 0.7)
    assert count == h * w - 2 and not v[1, 2].any() and not v[4, 0].any() and not v[2, 2].any()
    assert abs(loss - 0.7 * np.abs(np.where(np.isfinite(t).all(-1, keepdims=True), f.astype(np.float64) - t, 0)).sum() / (h * w * c)) <= 1e-7 * loss
    for idx in [(0, 0, 0), (3, 4, 2), (5, 6, 3), (1, 2, 0)]:
        num = _fd(lambda x: feature_ref.l1_loss(x, t, 0.7)[0], f, idx, np.float32(1e-2))
        assert abs(num - v[idx]) <= 1e-4 * (0.7 / (h * w * c)), (idx, num, v[idx])


def test_cross_entropy_restatement():
    rng = np.random.default_rng(6)
    h, w, c = 5, 6, 7
    f = rng.normal(0, 3, (h, w, c)).astype(np.float32)
    f[0, 0] = [80, -80, 0, 79, -3, 2, 1]   # no overflow: the maximum is subtracted
    lab = rng.integers(0, c, (h, w)).astype(np.uint8)
    lab[1, 1], lab[2, 3] = 255, c
    loss, count, v = feature_ref.cross_entropy_loss(f, lab, 1.3)
    assert count == h * w - 2 and np.isfinite(loss) and np.isfinite(v).all() and not v[1, 1].any() and not v[2, 3].any()
    # against torch's own cross entropy (sum over the valid pixels / (H W))
    tl = torch.nn.functional.cross_entropy(torch.tensor(f, dtype=torch.float64).reshape(-1, c), torch.tensor(np.where(lab < c, lab.astype(np.int64), -100)).reshape(-1),
                                           ignore_index=-100, reduction="sum")
    assert abs(loss - 1.3 * float(tl) / (h * w)) <= 1e-12 * abs(loss)
    assert np.abs(v.sum(-1)).max() <= 1e-15   # softmax - onehot sums to 0
    for idx in [(0, 0, 0), (0, 0, 3), (3, 4, 2), (4, 5, 6)]:
        num = _fd(lambda x: feature_ref.cross_entropy_loss(x, lab, 1.3)[0], f, idx, np.float32(2.0 ** -7))
        assert abs(num - v[idx]) <= 1e-3 * (1.3 / (h * w)), (idx, num, v[idx])
