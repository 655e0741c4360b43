"""Camera pose gradients on the GPU (include/brush_hip_pose.h): v_viewmat against the float64 reference
tests/pose_ref.py, the rigid-invariance identities on the device's own output, the splat outputs bit for bit, run-to-run and list
policy, the empty view, and the recovery of a perturbed camera by PoseOptimizer.

Bound of every comparison: |delta_k| <= 1e-4 S_k, S_k = the L1 mass sum_i |contribution of splat i to entry k| — the project's
1e-4 per-element gradient figure applied to each summand (the sum cancels, so the bound is on the mass, not on the result)."""
import functools
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import pose_ref
import util

pytestmark = pytest.mark.gpu
TOL = 1e-4
BIG, SMALL = (3000, 123, 82, 0xB1), (40, 32, 32, 0xA1)


def _scene(n, w, h, seed, deg, model):
    cp = synth.default_camera_params(w, h)
    tans = (math.tan(cp["fov_x"] / 2.0), math.tan(cp["fov_y"] / 2.0))
    scales = (0.01, 0.1) if n > 1000 else (0.05, 0.4)
    sc = synth.make_scene(n, seed, sh_degree=deg, log_scale_range=(math.log(scales[0]), math.log(scales[1])), z_range=(2.0, 9.0), tan_half_fov=tans)
    cp = {k: v for k, v in cp.items() if k not in ("img_w", "img_h")}
    cp["pos"] = (0.15, -0.1, -0.4)
    cp["rot_xyzw"] = util.quat_from_axis_angle((0.3, 1.0, 0.1), 0.08)
    if model != "pinhole":
        cp["model"], cp["dist"] = util.REF_LENSES[model]
    return sc, cp


def _v_output(h, w, seed):
    return (np.random.default_rng(seed).uniform(-1, 1, (h, w, 4)) / (h * w)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(size, model, deg, mip, smooth):
    """Computed once per case and shared; never modified."""
    n, w, h, seed = size
    sc, cp = _scene(n, w, h, seed, deg, model)
    with torch.enable_grad():
        res = pose_ref.pose_gradients(sc, cp, w, h, _v_output(h, w, deg + 7), intrinsics=pose_ref.intrinsics(cp, w, h), mip=mip, smooth=smooth,
                                      skip_ties=True)
    return sc, cp, res


def _node(ba, ctx, dev, sc, cp, w, h, mip, smooth, **kw):
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], render_mip=mip, device=dev)
    pass_ = ba.RasterPass.BackwardSmoothCutoff if smooth else ba.RasterPass.Backward
    return ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), pass_=pass_, ctx=ctx, **kw)


def _check(tag, got, want, mass):
    got, want, mass = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(mass, np.float64)
    assert np.isfinite(got).all(), tag
    ratio = np.abs(got - want) / np.maximum(mass, 1e-300)
    print("%s: max |delta_k| / S_k = %.3e" % (tag, float(ratio.max())))
    assert (np.abs(got - want) <= TOL * mass).all(), (tag, ratio)


# every lens, Mip on and off, SH degree 0 and 3, both cut-offs; the large scene (several blocks, a ragged last one) once per cut-off
PARITY = [(SMALL, "pinhole", 0, False, False), (SMALL, "pinhole", 3, True, True), (SMALL, "kb4", 3, True, False), (SMALL, "kb4", 0, False, True),
          (SMALL, "rt8", 0, True, True), (SMALL, "rt8", 3, False, False), (SMALL, "tpf", 3, False, True), (SMALL, "tpf", 0, True, False),
          (BIG, "pinhole", 3, False, False), (BIG, "tpf", 0, True, True)]


@pytest.mark.parametrize("size,model,deg,mip,smooth", PARITY)
def test_v_viewmat_matches_the_float64_reference(dev, size, model, deg, mip, smooth):
    import brush_amd as ba
    n, w, h, _ = size
    sc, cp, ref = _reference(size, model, deg, mip, smooth)
    assert ref["ties"].mean() <= 0.01, int(ref["ties"].sum())   # pixels left out: within the tie band of the float64 run
    assert np.abs(ref["v_viewmat"]).max() > 1e-4
    ctx = ba.Context(dev)
    try:
        node = _node(ba, ctx, dev, sc, cp, w, h, mip, smooth)
        g = node.backward(torch.from_numpy(ref["v_output"].astype(np.float32)).to(dev), pose=True)
        vm = np.array(list(util.hip_camera(ba, cp).uniforms((w, h)).vm), np.float64)
        assert np.abs(vm - ref["vm"]).max() <= 1e-6
        _check("%s n=%d deg=%d mip=%d smooth=%d" % (model, n, deg, mip, smooth), g["v_viewmat"].cpu().numpy(), ref["v_viewmat"], ref["S"])
    finally:
        ctx.close()


@pytest.mark.parametrize("size,model,deg,mip", [(BIG, "pinhole", 0, False), (BIG, "kb4", 0, True), (SMALL, "rt8", 0, False), (BIG, "pinhole", 3, False),
                                                (SMALL, "tpf", 3, True)])
def test_device_output_satisfies_the_rigid_identities(dev, size, model, deg, mip):
    """On the values ONE call returned: v_t = W sum v_mean (any degree) and, at degree 0, v_omega from v_viewmat = the identity
    evaluated in f64 on v_transforms.  The masses are those of the device's own per-splat rows."""
    import brush_amd as ba
    n, w, h, seed = size
    sc, cp = _scene(n, w, h, seed, deg, model)
    ctx = ba.Context(dev)
    try:
        node = _node(ba, ctx, dev, sc, cp, w, h, mip, True)
        g = node.backward(torch.from_numpy(_v_output(h, w, 3)).to(dev), pose=True)
        vv = g["v_viewmat"].cpu().numpy().astype(np.float64)
        vt = g["v_transforms"].cpu().numpy().astype(np.float64)
        vm = np.array(list(util.hip_camera(ba, cp).uniforms((w, h)).vm), np.float64)
        w_mat, t = pose_ref.unpack(vm)
        assert np.abs(vv).max() > 1e-5
        _check("v_t", vv[9:], w_mat @ vt[:, 0:3].sum(0), np.abs(vt[:, 0:3] @ w_mat.T).sum(0))
        if deg == 0:
            om = pose_ref.twist(vm, vv)[:3]
            _check("v_omega", om, pose_ref.omega_from_splat_grads(vm, sc["transforms"], vt), pose_ref.omega_mass_from_splat_grads(vm, sc["transforms"], vt))
    finally:
        ctx.close()


def test_splat_outputs_are_those_of_the_plain_backward(dev):
    """A retained forward rendered twice: the four splat outputs of the pose backward are bit-equal to bh_render_backward_saved's
    (v_output confined to one tile: every splat gets one addition, so the backward repeats itself)."""
    import brush_amd as ba
    n, w, h, seed = BIG
    sc, cp = _scene(n, w, h, seed, 3, "pinhole")
    v = np.zeros((h, w, 4), np.float32)
    v[16:32, 32:48] = _v_output(16, 16, 1)
    vt = torch.from_numpy(v).to(dev)
    ctx = ba.Context(dev)
    try:
        a = _node(ba, ctx, dev, sc, cp, w, h, False, False, retain=True)
        b = _node(ba, ctx, dev, sc, cp, w, h, False, False, retain=True)
        plain = a.backward(vt)
        posed = b.backward(vt, pose=True)
        again = b.backward(vt, pose=True)
        assert float(plain["v_transforms"].abs().max()) > 0
        for k in plain:
            assert torch.equal(plain[k].view(torch.int32), posed[k].view(torch.int32)), k
        # ... and two calls on the same retained forward give the same twelve, to the bit
        assert float(posed["v_viewmat"].abs().max()) > 0
        assert torch.equal(posed["v_viewmat"].view(torch.int32), again["v_viewmat"].view(torch.int32))
        a.release()
        b.release()
    finally:
        ctx.close()


def test_run_to_run_and_list_policy(dev):
    import brush_amd as ba
    n, w, h = 60000, 320, 208
    cp0 = synth.default_camera_params(w, h)
    tans = (math.tan(cp0["fov_x"] / 2.0), math.tan(cp0["fov_y"] / 2.0))
    sc = synth.make_scene(n, 0x56, sh_degree=1, log_scale_range=(math.log(0.03), math.log(0.3)), tan_half_fov=tans)
    cp = {k: v for k, v in cp0.items() if k not in ("img_w", "img_h")}
    vt = torch.from_numpy(_v_output(h, w, 9)).to(dev)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    cam = util.hip_camera(ba, cp)
    ctx = ba.Context(dev)
    try:
        base = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, retain=True)
        g0 = base.backward(vt, pose=True)
        g1 = base.backward(vt, pose=True)
        base.release()
        v0 = g0["v_viewmat"].cpu().numpy().astype(np.float64)
        # The masses of all twelve entries, from below: W = I here, so the translation entries' S_k is sum |v_mean| of the device's
        # own rows; the nine W entries have no per-splat rows at this size (the float64 reference would walk 60000 splats for a
        # minute), and S_k >= |v_k| (the triangle inequality) stands in for them, entry by entry: a bound no wider than 1e-4 S_k.
        # The risk of the stand-in: the atomic-order noise of v_combined scales with S_k, not with |v_k|, so an entry whose sum
        # nearly cancelled could miss 1e-4 |v_k| while inside 1e-4 S_k.  On this scene (fixed seed) no entry cancels that far:
        # measured on the MI355X, the largest |delta_k| / |v_k| of two calls was 7.8e-6 and 1.6e-5 in two runs, of the cut
        # lists 2.3e-6 and 8.2e-6 — at least six times inside the bound.  Changing the scene means measuring that again.
        vtr = g0["v_transforms"].cpu().numpy().astype(np.float64)
        mass = np.concatenate([np.abs(v0[:9]), np.abs(vtr[:, 0:3]).sum(0)])
        assert (mass > 0).all()
        _check("run to run", g1["v_viewmat"].cpu().numpy(), v0, mass)
        ba.set_view_id(0xD0, ctx)
        ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
        cut = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
        assert cut.out.tile_offsets_far and cut.out.num_listed_splats < cut.out.num_visible, "not a cut frame"
        gc = cut.backward(vt, pose=True)
        _check("cut lists", gc["v_viewmat"].cpu().numpy(), v0, mass)
    finally:
        ctx.close()


def test_empty_view_writes_twelve_zeros(dev):
    import brush_amd as ba
    from brush_amd.host import _ptr
    import ctypes as C
    n, w, h, seed = SMALL
    sc, cp = _scene(n, w, h, seed, 0, "pinhole")
    cp["rot_xyzw"] = util.quat_from_axis_angle((0.0, 1.0, 0.0), math.pi)   # turned away from the scene
    ctx = ba.Context(dev)
    try:
        node = _node(ba, ctx, dev, sc, cp, w, h, False, False)
        assert node.out.num_visible == 0
        spl = node.splats
        r_t, r_o = node._folded
        outs = [torch.empty((n, 10), device=dev), torch.empty((n, 1, 3), device=dev), torch.empty((n,), device=dev), torch.empty((n,), device=dev)]
        vv = torch.full((12,), float("nan"), device=dev)
        vt = torch.from_numpy(_v_output(h, w, 2)).to(dev)
        ctx.check(ctx.lib.bh_render_backward_pose_saved(ctx._h, C.byref(node.out), _ptr(vt), _ptr(r_t), _ptr(spl.sh_coeffs), _ptr(r_o),
                                                        _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), _ptr(vv)))
        assert torch.equal(vv, torch.zeros(12, device=dev))
    finally:
        ctx.close()


# ---- recovery ---------------------------------------------------------------------------------------------------------------
RECOVERY = dict(lr_rotation=2e-3, lr_translation=1.5e-2, iters=40)   # chosen on the CPU with pose_ref


def test_pose_optimizer_recovers_a_perturbed_camera(dev):
    """Frozen splats, the target rendered from the true camera, the student turned by 2 degrees and shifted by 5 % of the scene
    depth; PoseOptimizer alone through RenderNode.backward(pose=True).  Both errors at most half their initial value."""
    import brush_amd as ba
    w, h = 64, 48
    cp0 = synth.default_camera_params(w, h)
    tans = (math.tan(cp0["fov_x"] / 2.0), math.tan(cp0["fov_y"] / 2.0))
    cp = {k: v for k, v in cp0.items() if k not in ("img_w", "img_h")}
    sc = synth.make_scene(400, 0xC7, sh_degree=0, log_scale_range=(math.log(0.05), math.log(0.3)), z_range=(3.0, 8.0), tan_half_fov=tans)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    true_cam = util.hip_camera(ba, cp)
    ax_r, ax_t = np.array([0.3, 1.0, -0.2]), np.array([0.2, -0.1, 0.15])
    tw0 = np.concatenate([ax_r / np.linalg.norm(ax_r) * math.radians(2.0), ax_t / np.linalg.norm(ax_t) * 0.05 * 5.5])
    student = ba.host._uniforms_apply_twist(true_cam.uniforms((w, h)), tw0)
    w0, t0 = pose_ref.unpack(np.array(list(true_cam.uniforms((w, h)).vm), np.float64))

    def errs(cam):
        wm, t = pose_ref.unpack(np.array(list(cam.vm), np.float64))
        r = wm @ w0.T
        return math.acos(max(-1.0, min(1.0, (np.trace(r) - 1.0) / 2.0))), float(np.linalg.norm(wm.T @ t - w0.T @ t0))

    ctx = ba.Context(dev)
    try:
        smooth = ba.RasterPass.BackwardSmoothCutoff
        target = ba.render_splats_diff(spl, true_cam, (w, h), pass_=smooth, ctx=ctx).img.clone()
        po = ba.PoseOptimizer(lr_rotation=RECOVERY["lr_rotation"], lr_translation=RECOVERY["lr_translation"])
        e0 = errs(student)
        tables = []
        for _ in range(RECOVERY["iters"]):
            cam = po.bind(ctx, 1, student)
            node = ba.render_splats_diff(spl, cam, (w, h), pass_=smooth, ctx=ctx)
            v = (node.img - target) * (2.0 / (h * w * 4))
            g = node.backward(v, pose=True)
            po.step(1, list(cam.vm), g["v_viewmat"], ctx)
            tables.append(ctx.view_table_count())
        e1 = errs(po.camera(1, student))
        print("rotation %.4f -> %.4f rad, translation %.4f -> %.4f" % (e0[0], e1[0], e0[1], e1[1]))
        assert tables[-1] == tables[1] <= 1, tables   # the moving camera is one view: no table per step
        assert e1[0] <= 0.5 * e0[0] and e1[1] <= 0.5 * e0[1], (e0, e1)
    finally:
        ctx.close()
