"""Pins tests/pose_ref.py, the float64 reference of the pose gradient (include/brush_hip_pose.h), without a GPU:
(a) its image is oracle/autograd_ref.py::render's, (b) its v_viewmat agrees with central finite differences of its own
smooth-cut-off render (step and tolerances of tests/test_oracle_finite_diff.py), (c) the rigid-invariance identities hold."""
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
from oracle import autograd_ref
import pose_ref
import util

EPS, REL_TOL, ABS_TOL = 3e-4, 0.02, 2e-4   # tests/test_oracle_finite_diff.py


def scene_and_camera(n, w, h, seed, sh_degree, model="pinhole", turned=True):
    cp = synth.default_camera_params(w, h)
    tans = (math.tan(cp["fov_x"] / 2.0), math.tan(cp["fov_y"] / 2.0))
    sc = synth.make_scene(n, seed, sh_degree=sh_degree, log_scale_range=(math.log(0.05), math.log(0.4)), z_range=(2.0, 9.0), tan_half_fov=tans)
    cp = {k: v for k, v in cp.items() if k not in ("img_w", "img_h")}
    if turned:
        cp["pos"] = (0.15, -0.1, -0.4)
        cp["rot_xyzw"] = util.quat_from_axis_angle((0.3, 1.0, 0.1), 0.08)
    if model != "pinhole":
        cp["model"], cp["dist"] = util.REF_LENSES[model]
    return sc, cp


def _weights(h, w, seed=17):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (h, w, 4)) / (h * w)


CASES = [("pinhole", 0, False, False), ("pinhole", 3, True, True), ("kb4", 3, False, True), ("rt8", 0, True, False), ("tpf", 3, False, False)]


@pytest.mark.parametrize("model,deg,mip,smooth", CASES)
def test_image_is_the_pinned_renderers(model, deg, mip, smooth):
    w, h = 32, 32
    sc, cp = scene_and_camera(40, w, h, 0xA1, deg, model)
    intr = pose_ref.intrinsics(cp, w, h)
    # (leaves that require a gradient: the lens models take their Jacobian by autograd)
    tr, sh, op = [torch.tensor(np.asarray(sc[k], np.float64), requires_grad=True) for k in ("transforms", "sh", "raw_opac")]
    a = autograd_ref.render(tr, sh, op, cp, w, h, (0.1, 0.2, 0.3), intr, mip, smooth).detach()
    b = pose_ref.render(tr, sh, op, cp, w, h, (0.1, 0.2, 0.3), intr, mip, smooth)["img"].detach()
    assert float(a.abs().max()) > 0.1
    assert float((a - b).abs().max()) <= 1e-12


def _fd_camera(model):
    """The first camera of tests/util.py::random_camera_with_model (the finite-difference suite's cameras) with this lens."""
    for seed in range(1, 64):
        cp = util.random_camera_with_model(seed)
        if cp["model"] == model:
            return seed, cp
    raise AssertionError(model)


@pytest.mark.parametrize("model", ["pinhole", "kb4", "rt8", "tpf"])
def test_v_viewmat_matches_finite_differences(model):
    """On the finite-difference suite's own scenes (tests/test_oracle_finite_diff.py: means in [-1, 1]^3, its cameras), with its step
    and tolerances.  Without Mip: there the gradient is by contract not the forward's derivative (comp_is_constant)."""
    w, h = 32, 32
    seed, cp = _fd_camera(model)
    sc = util.random_scene(seed, 6)
    intr = pose_ref.intrinsics(cp, w, h)
    v = np.random.default_rng(5).uniform(0.0, 1.0, (h, w, 4)) / 16.0
    res = pose_ref.pose_gradients(sc, cp, w, h, v, intrinsics=intr, smooth=True)
    assert np.allclose(res["v_viewmat"], res["v_viewmat_leaf"], rtol=1e-10, atol=1e-13)   # the per-splat copies sum to the leaf's gradient
    tr, sh, op = [torch.tensor(np.asarray(sc[k], np.float64), requires_grad=True) for k in ("transforms", "sh", "raw_opac")]
    vt = torch.tensor(v)

    def loss(vm):
        wm, t = pose_ref.unpack(vm)
        img = pose_ref.render(tr, sh, op, cp, w, h, intrinsics=intr, smooth=True, pose=(torch.tensor(wm), torch.tensor(t)))["img"]
        return float((img.detach() * vt).sum())

    assert np.abs(res["v_viewmat"]).max() > 1e-2
    for k in range(12):
        e = np.zeros(12)
        e[k] = EPS
        num = (loss(res["vm"] + e) - loss(res["vm"] - e)) / (2 * EPS)
        an = res["v_viewmat"][k]
        assert abs(num - an) <= ABS_TOL + REL_TOL * max(abs(num), abs(an), 1e-8), (k, num, an)


def _rot(axis, angle):
    return torch.linalg.matrix_exp(torch.tensor(pose_ref._hat(np.asarray(axis, np.float64) * angle))).numpy()


@pytest.mark.parametrize("model,deg", [("pinhole", 0), ("kb4", 0), ("pinhole", 2)])
def test_rigid_invariance(model, deg):
    w, h = 32, 32
    sc, cp = scene_and_camera(40, w, h, 0xA3, deg, model)
    intr = pose_ref.intrinsics(cp, w, h)
    pose = pose_ref.pose_of(cp, w, h)
    v = _weights(h, w)
    base = pose_ref.pose_gradients(sc, cp, w, h, v, intrinsics=intr, smooth=True)
    scale = float(np.abs(base["img"]).max())
    # the image does not move under a world translation (any degree) nor, at degree 0, under a world rotation
    g_rot = _rot((0.2, -0.5, 0.8), 0.3) if deg == 0 else np.eye(3)
    sc2, pose2 = pose_ref.rigid_map(sc, pose, g_rot, np.array([0.3, -0.2, 0.5]))
    moved = pose_ref.pose_gradients(sc2, cp, w, h, v, intrinsics=intr, smooth=True, pose=pose2)
    assert float(np.abs(moved["img"] - base["img"]).max()) <= 1e-9 * scale
    # at G = I: v_t = W sum_i v_mean_i
    w_mat, t = pose
    v_t = base["v_viewmat"][9:]
    want = w_mat @ base["v_transforms"][:, 0:3].sum(0)
    ref_scale = float(np.abs(base["per_splat"][:, 9:]).sum())
    assert float(np.abs(v_t - want).max()) <= 1e-9 * ref_scale
    if deg == 0:
        om = pose_ref.twist(base["vm"], base["v_viewmat"])[:3]
        want = pose_ref.omega_from_splat_grads(base["vm"], sc["transforms"], base["v_transforms"])
        mass = pose_ref.omega_mass_from_splat_grads(base["vm"], sc["transforms"], base["v_transforms"])
        assert float(np.abs(om).max()) > 1e-6
        assert float(np.abs(om - want).max()) <= 1e-9 * float(mass.max()), (om, want)


def test_hard_cutoff_ties_stay_rare():
    """The tie band of every hard cut-off case of the GPU parity suite (tests/test_gpu_pose.py PARITY), on the reference alone: at
    most 1 % of the frame's pixels.  The band depends on alpha and T only, so the colours are left at SH degree 0 here."""
    import test_gpu_pose as g
    hard = [c for c in g.PARITY if not c[4]]
    assert len(hard) == 5
    for size, model, _deg, mip, smooth in hard:
        n, w, h, seed = size
        sc, cp = g._scene(n, w, h, seed, 0, model)
        tr, sh, op = [torch.tensor(np.asarray(sc[k], np.float64), requires_grad=(model != "pinhole")) for k in ("transforms", "sh", "raw_opac")]
        with torch.set_grad_enabled(model != "pinhole"):   # (the lens models take their Jacobian by autograd)
            out = pose_ref.render(tr, sh, op, cp, w, h, intrinsics=pose_ref.intrinsics(cp, w, h), mip=mip, smooth=False)
        ties = pose_ref.tie_mask(out, False)
        print("%s n=%d mip=%d: %d tie pixels of %d" % (model, n, mip, int(ties.sum()), w * h))
        assert float(ties.float().mean()) <= 0.01, (model, n, int(ties.sum()))
