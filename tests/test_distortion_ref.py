"""tests/distortion_ref.py pinned without a GPU: its RGBA, depth and tie margins are depth_ref.render's exactly (pinhole, a fisheye
model, Mip, the smooth cut-off), its normals are normal_ref.render's, dist = A M2 - M1^2 equals the literal double sum over pairs for
both kinds, is invariant under a shift of the depths, vanishes for one splat, and its autograd gradient is what central differences
say."""
import numpy as np
import pytest
import torch

import depth_ref
import distortion_ref
import normal_ref
import util

CASES = [("pinhole", False, False), ("kb4", False, False), ("pinhole", True, False), ("pinhole", False, True)]


def _case(model, seed=3, n=6):
    sc = util.random_scene(seed, n)
    camp = dict(util.random_camera(seed))
    if model != "pinhole":
        camp["model"], camp["dist"] = util.REF_LENSES[model]
    return sc, camp


def _tensors(sc):
    # (leaves that require grad: the lens models take their Jacobian by autograd)
    return [torch.tensor(np.asarray(sc[k], np.float64), requires_grad=True) for k in ("transforms", "sh", "raw_opac")]


@pytest.mark.parametrize("model,mip,smooth", CASES)
def test_rgba_depth_and_margins_are_depth_refs_exactly(model, mip, smooth):
    w = h = 40
    for seed in (3, 7):
        sc, camp = _case(model, seed, 2 + seed % 7)
        intr = distortion_ref.intrinsics(camp, w, h)
        tr, sh, op = _tensors(sc)
        bg = (0.1, 0.3, 0.2)
        a = depth_ref.render(tr, sh, op, camp, w, h, bg, intr, mip, smooth)
        n = normal_ref.render(tr, sh, op, camp, w, h, bg, intr, mip, smooth)
        out = distortion_ref.render(tr, sh, op, camp, w, h, bg, intr, mip, smooth)
        for k in ("img", "acc", "alpha", "expected", "tie_alpha", "tie_t", "tie_median", "n_terms"):
            assert torch.equal(a[k], out[k]), k
        assert torch.equal(n["normal"], out["normal"])
        assert torch.equal(out["A"], out["img"][..., 3])
        # kind "z": M1 is the accumulated depth
        assert torch.equal(out["M1"], out["acc"])


@pytest.mark.parametrize("kind", ["z", "ndc"])
@pytest.mark.parametrize("model,mip,smooth", CASES)
def test_dist_is_the_literal_sum_over_pairs(model, mip, smooth, kind):
    w = h = 40
    sc, camp = _case(model, 7, 9)
    intr = distortion_ref.intrinsics(camp, w, h)
    tr, sh, op = _tensors(sc)
    with torch.enable_grad():
        out = distortion_ref.render(tr, sh, op, camp, w, h, intrinsics=intr, mip=mip, smooth=smooth, kind=kind, near=0.1, far=50.0, keep_terms=True)
    weights, m = out["terms"]
    want = distortion_ref.pair_sum(weights, m)
    got = out["dist"].detach()
    assert int(out["n_terms"].max()) >= 3 and float(want.max()) > 0.0
    assert float((got - want).abs().max()) <= 1e-12 * max(float(want.max()), float((out["A"] * out["M2"]).detach().max()))
    assert bool((want >= 0).all())
    # the sum of the weights is the image's alpha, and a pixel with fewer than two terms has no distortion
    assert float((weights.sum(0) - out["A"].detach()).abs().max()) <= 1e-14
    assert float(got[out["n_terms"] < 2].abs().max()) <= 1e-15
    if kind == "ndc":   # m is 2DGS's mapping: 0 at near, 1 at far, monotone
        z = out["z"].detach()
        assert float(distortion_ref.splat_depth(torch.tensor(0.1, dtype=torch.float64), "ndc", 0.1, 50.0)) == 0.0
        assert abs(float(distortion_ref.splat_depth(torch.tensor(50.0, dtype=torch.float64), "ndc", 0.1, 50.0)) - 1.0) <= 1e-15
        order = torch.argsort(z)
        assert bool((out["m"].detach()[order].diff() >= 0).all())


def test_dist_does_not_change_under_a_shift_of_the_depths():
    """The property the kernels' per-pixel reference rests on: with the weights fixed, m -> m - r leaves A M2 - M1^2 unchanged."""
    w = h = 32
    sc, camp = _case("pinhole", 7, 9)
    tr, sh, op = _tensors(sc)
    out = distortion_ref.render(tr, sh, op, camp, w, h, keep_terms=True)
    weights, m = out["terms"]
    a = weights.sum(0)
    for r in (0.0, float(m[0]), 123.0):
        d = m - r
        m1 = (weights * d[:, None, None]).sum(0)
        m2 = (weights * (d * d)[:, None, None]).sum(0)
        assert float((a * m2 - m1 * m1 - out["dist"].detach()).abs().max()) <= 1e-9 * (1.0 + r * r)


def test_one_splat_has_no_distortion():
    sc = util.random_scene(3, 1)
    camp = util.random_camera(3)
    tr, sh, op = _tensors(sc)
    out = distortion_ref.render(tr, sh, op, camp, 24, 24)
    assert float(out["A"].detach().max()) > 0.0
    assert float(out["dist"].detach().abs().max()) <= 1e-15


@pytest.mark.parametrize("kind", ["z", "ndc"])
def test_autograd_agrees_with_central_differences(kind):
    w = h = 20
    sc, camp = _case("pinhole", 5, 5)
    rng = np.random.default_rng(4)
    v = rng.uniform(0.2, 1.0, (h, w))
    vt = torch.tensor(v)
    kw = dict(kind=kind, near=0.1, far=50.0)
    _, g_tr, g_sh, g_op = distortion_ref.gradients(sc, camp, w, h, v, **kw)
    assert float(np.abs(g_sh).max()) == 0.0 and float(np.abs(g_tr[:, :3]).max()) > 0.0 and float(np.abs(g_op).max()) > 0.0

    def value(tr, op):
        sh = torch.tensor(np.asarray(sc["sh"], np.float64))
        return float((distortion_ref.render(tr, sh, op, camp, w, h, **kw)["dist"] * vt).sum())
    tr0 = torch.tensor(np.asarray(sc["transforms"], np.float64))
    op0 = torch.tensor(np.asarray(sc["raw_opac"], np.float64))
    eps = 1e-6
    scale = float(np.abs(g_tr).max())
    for i in range(tr0.shape[0]):
        for c in range(10):
            def pert(d):
                x = tr0.clone()
                x[i, c] += d
                return value(x, op0)
            num = (pert(eps) - pert(-eps)) / (2 * eps)
            assert abs(num - g_tr[i, c]) <= 1e-5 * scale + 1e-9, (i, c, num, g_tr[i, c])
        def pert_o(d):
            x = op0.clone()
            x[i] += d
            return value(tr0, x)
        num = (pert_o(eps) - pert_o(-eps)) / (2 * eps)
        assert abs(num - g_op[i]) <= 1e-5 * float(np.abs(g_op).max()) + 1e-9, (i, num, g_op[i])
