"""tests/depth_ref.py pinned without a GPU: its RGBA is oracle/autograd_ref.render's exactly (pinhole, a fisheye model, Mip), the
accumulated depth lies between z_min A and z_max A, and its autograd gradient of <v, D> agrees with central finite differences."""
import numpy as np
import pytest
import torch

from oracle import autograd_ref
import depth_ref
import util

CASES = [("pinhole", False), ("kb4", False), ("pinhole", True)]


def _case(model, seed=3, n=6):
    sc = util.random_scene(seed, n)
    camp = dict(util.random_camera(seed))
    if model != "pinhole":
        camp["model"], camp["dist"] = util.REF_LENSES[model]
    return sc, camp


def _tensors(sc):
    # (leaves that require grad: the lens models take their Jacobian by autograd)
    return [torch.tensor(np.asarray(sc[k], np.float64), requires_grad=True) for k in ("transforms", "sh", "raw_opac")]


@pytest.mark.parametrize("model,mip", CASES)
def test_rgba_is_autograd_refs_exactly(model, mip):
    w = h = 40
    for seed in (3, 7):
        sc, camp = _case(model, seed, 2 + seed % 7)
        intr = depth_ref.intrinsics(camp, w, h)
        tr, sh, op = _tensors(sc)
        bg = (0.1, 0.3, 0.2)
        a = autograd_ref.render(tr, sh, op, camp, w, h, bg, intr, mip)
        out = depth_ref.render(tr, sh, op, camp, w, h, bg, intr, mip)
        assert torch.equal(a, out["img"])
        assert torch.equal(out["alpha"], a[..., 3])
    sc, camp = util.base_scene(), util.STD_CAM
    tr, sh, op = _tensors(sc)
    assert torch.equal(autograd_ref.render(tr, sh, op, camp, 32, 32), depth_ref.render(tr, sh, op, camp, 32, 32)["img"])


@pytest.mark.parametrize("model,mip", CASES)
def test_depth_is_bounded_by_the_splats_it_blends(model, mip):
    w = h = 40
    sc, camp = _case(model)
    tr, sh, op = _tensors(sc)
    out = depth_ref.render(tr, sh, op, camp, w, h, intrinsics=depth_ref.intrinsics(camp, w, h), mip=mip)
    out = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}
    z = out["z"][out["keep"]]
    zmin, zmax = float(z.min()), float(z.max())
    A, D = out["alpha"], out["acc"]
    assert float(A.max()) > 0.1
    eps = 1e-12
    assert bool(((D >= zmin * A - eps) & (D <= zmax * A + eps)).all())
    E = out["expected"]
    seen = A > 0
    assert bool(((E[seen] >= zmin - 1e-9) & (E[seen] <= zmax + 1e-9)).all()) and bool((E[~seen] == 0).all())
    med = out["median"]
    found = med != 0
    assert bool(found.any()) and bool(((med[found] >= zmin) & (med[found] <= zmax)).all())
    assert bool((A[found] >= 0.5).all()) and bool((med[A < 0.5] == 0).all())


@pytest.mark.parametrize("mode", ["accumulated", "expected"])
@pytest.mark.parametrize("model,mip", CASES)
def test_autograd_gradient_agrees_with_central_differences(model, mip, mode):
    """Smooth cut-off (the reference's finite-difference pass), comp_is_constant=False in Mip mode: the true derivative of the
    forward, which is what a finite difference measures."""
    w = h = 24
    sc, camp = _case(model, 5, 4)
    intr = depth_ref.intrinsics(camp, w, h)
    rng = np.random.default_rng(11)
    v = rng.uniform(-1.0, 1.0, (h, w)) / (h * w)
    key = "acc" if mode == "accumulated" else "expected"

    def value(tr, sh, op):
        return (depth_ref.render(tr, sh, op, camp, w, h, intrinsics=intr, mip=mip, smooth=True, comp_is_constant=False)[key] * torch.tensor(v)).sum()
    tr, sh, op = _tensors(sc)
    value(tr, sh, op).backward()
    eps = 1e-6
    for name, t, g, picks in (("tr", tr, tr.grad, [(0, 0), (0, 2), (1, 1), (2, 4), (1, 8), (3, 2)]), ("op", op, op.grad, [(0,), (2,)])):
        for idx in picks:
            def pert(d):
                x = t.detach().clone()
                x[idx] += d
                x.requires_grad_(True)
                return float(value(*((x, sh, op) if name == "tr" else (tr, sh, x))).detach())
            num = (pert(eps) - pert(-eps)) / (2 * eps)
            an = float(g[idx])
            assert abs(num - an) <= 1e-6 * max(abs(num), abs(an)) + 1e-9, (name, idx, num, an)
    assert float(tr.grad[:, :3].abs().max()) > 0
