"""Pins tests/intrinsics_ref.py, the float64 reference of the intrinsics gradient (include/brush_hip_intrinsics.h),
without a GPU: (a) its image is oracle/autograd_ref.py::render's for the four lens models, Mip on and off, (b) its v_intrinsics
agrees with central finite differences of its own smooth-cut-off loss (step and tolerances of tests/test_pose_ref.py), (c) the
header's per-splat formula, evaluated in f64 on the reference's v_xy / v_conic, is autograd's per-splat gradient: this pins the
convention of the off-diagonal entry G01."""
import numpy as np
import pytest
import torch

from oracle import autograd_ref
import intrinsics_ref
from test_pose_ref import ABS_TOL, EPS, REL_TOL, _fd_camera, scene_and_camera
import util

MODELS = ["pinhole", "kb4", "rt8", "tpf"]


@pytest.mark.parametrize("mip", [False, True])
@pytest.mark.parametrize("model", MODELS)
def test_image_is_the_pinned_renderers(model, mip):
    w, h = 32, 32
    sc, cp = scene_and_camera(40, w, h, 0xA1, 2, model)
    intr = intrinsics_ref.intrinsics(cp, w, h)
    tr, sh, op = [torch.tensor(np.asarray(sc[k], np.float64), requires_grad=True) for k in ("transforms", "sh", "raw_opac")]
    a = autograd_ref.render(tr, sh, op, cp, w, h, (0.1, 0.2, 0.3), intr, mip, model == "kb4").detach()
    b = intrinsics_ref.render(tr, sh, op, cp, w, h, (0.1, 0.2, 0.3), intr, mip, model == "kb4")["img"].detach()
    assert float(a.abs().max()) > 0.1
    assert float((a - b).abs().max()) <= 1e-12


@pytest.mark.parametrize("model", MODELS)
def test_v_intrinsics_matches_finite_differences(model):
    """On the finite-difference suite's own scenes and cameras, with the step and tolerances tests/test_pose_ref.py uses for the
    pose.  Without Mip: there the gradient is by contract not the forward's derivative."""
    w, h = 32, 32
    seed, cp = _fd_camera(model)
    sc = util.random_scene(seed, 6)
    intr = intrinsics_ref.intrinsics(cp, w, h)
    v = np.random.default_rng(5).uniform(0.0, 1.0, (h, w, 4)) / 16.0
    res = intrinsics_ref.intrinsics_gradients(sc, cp, w, h, v, intrinsics=intr, smooth=True)
    assert np.allclose(res["v_intrinsics"], res["v_intrinsics_leaf"], rtol=1e-10, atol=1e-13)   # the per-splat copies sum to the leaf's gradient
    tr, sh, op = [torch.tensor(np.asarray(sc[k], np.float64), requires_grad=(model != "pinhole")) for k in ("transforms", "sh", "raw_opac")]
    vt = torch.tensor(v)

    def loss(k):
        with torch.set_grad_enabled(model != "pinhole"):   # (the lens models take their Jacobian by autograd)
            img = intrinsics_ref.render(tr, sh, op, cp, w, h, intrinsics=intr, smooth=True, k=torch.tensor(k))["img"]
        return float((img.detach() * vt).sum())

    assert np.abs(res["v_intrinsics"]).max() > 1e-4
    for j in range(4):
        e = np.zeros(4)
        e[j] = EPS
        num = (loss(res["k"] + e) - loss(res["k"] - e)) / (2 * EPS)
        an = res["v_intrinsics"][j]
        print("%s entry %d: numeric %.6e analytic %.6e" % (model, j, num, an))
        assert abs(num - an) <= ABS_TOL + REL_TOL * max(abs(num), abs(an), 1e-8), (j, num, an)


@pytest.mark.parametrize("mip", [False, True])
@pytest.mark.parametrize("model", MODELS)
def test_header_formula_is_autograds_per_splat_gradient(model, mip):
    w, h = 32, 32
    sc, cp = scene_and_camera(40, w, h, 0xA2, 1, model)
    intr = intrinsics_ref.intrinsics(cp, w, h)
    v = np.random.default_rng(11).uniform(-1.0, 1.0, (h, w, 4)) / (h * w)
    res = intrinsics_ref.intrinsics_gradients(sc, cp, w, h, v, intrinsics=intr, mip=mip, smooth=False)
    want = res["per_splat"]
    got = intrinsics_ref.header_formula(res["k"], res["v_xy"], res["v_conic"], res["conic"], res["cov_raw"], res["d"])
    assert np.abs(want[:, 0]).max() > 1e-6 and np.abs(res["cov_raw"][:, 0, 1]).max() > 1e-3   # the off-diagonal term is exercised
    scale = np.abs(want).max(0)
    err = np.abs(got - want).max(0) / scale
    print("%s mip=%d: max |formula - autograd| / max |autograd| per entry = %s" % (model, mip, err))
    assert (err <= 1e-9).all(), err
    # ... and the other convention (G01 counted once) is not within the bound: the check can tell them apart
    G = intrinsics_ref.inverse2x2_vjp(res["conic"], np.stack([res["v_conic"][:, 0], 0.5 * res["v_conic"][:, 1], res["v_conic"][:, 2]], -1))
    other = got[:, 0] - G[:, 1] * res["cov_raw"][:, 0, 1] / res["k"][0]
    assert np.abs(other - want[:, 0]).max() / scale[0] > 1e-4
