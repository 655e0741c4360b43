"""Camera intrinsics gradients on the GPU (include/brush_hip_intrinsics.h): v_intrinsics against the float64
reference tests/intrinsics_ref.py on the scenes of tests/test_gpu_pose.py, the splat outputs and the pose gradient bit for bit, run
to run and list policy, the empty view, and the combination with a depth cotangent.

Bound of every comparison, as tests/test_gpu_pose.py: |delta_k| <= 1e-4 S_k, S_k = the L1 mass sum_i |contribution of splat i to
entry k| — the project's 1e-4 per-element gradient figure applied to each summand."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import intrinsics_ref
import test_gpu_pose as gp
import util

pytestmark = pytest.mark.gpu
TOL = 1e-4
# one 16x16 tile (every splat has at most one (splat, tile) pair: the backward repeats itself), and six tiles of a 48x32 frame
ONE, SIX = (2000, 16, 16, 0xB1), (600, 48, 32, 0xA1)
DEG = 1


def _v_depth(h, w, seed):
    return (np.random.default_rng(seed).uniform(-1, 1, (h, w)) / (h * w)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(size, model, mip, smooth, depth=False):
    """Computed once per case and shared; never modified."""
    n, w, h, seed = size
    sc, cp = gp._scene(n, w, h, seed, DEG, model)
    with torch.enable_grad():
        res = intrinsics_ref.intrinsics_gradients(sc, cp, w, h, gp._v_output(h, w, 5), intrinsics=intrinsics_ref.intrinsics(cp, w, h), mip=mip,
                                                  smooth=smooth, skip_ties=True, v_depth=_v_depth(h, w, 6) if depth else None)
    return sc, cp, res


def _check(tag, got, want, mass):
    got, want, mass = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(mass, np.float64)
    assert np.isfinite(got).all(), tag
    ratio = np.abs(got - want) / np.maximum(mass, 1e-300)
    print("%s: max |delta_k| / S_k = %.3e  (got %s)" % (tag, float(ratio.max()), got))
    assert (np.abs(got - want) <= TOL * mass).all(), (tag, ratio)


# the four lenses with the distortion values of tests/test_gpu_camera_models.py (util.REF_LENSES), Mip on and off, both cut-offs, on
# the six-tile frame; the one-tile scene (eight blocks of the pass, a ragged last one) for the pinhole and two lenses
PARITY = [(SIX, m, mip, mip) for m in ("pinhole", "kb4", "rt8", "tpf") for mip in (False, True)] + \
         [(ONE, "pinhole", False, False), (ONE, "pinhole", True, True), (ONE, "kb4", True, False), (ONE, "rt8", False, True)]


@pytest.mark.parametrize("size,model,mip,smooth", PARITY)
def test_v_intrinsics_matches_the_float64_reference(dev, size, model, mip, smooth):
    import brush_amd as ba
    n, w, h, _ = size
    sc, cp, ref = _reference(size, model, mip, smooth)
    # pixels left out: within the tie band of the float64 run (the one-tile frame stacks 2000 splats on 256 pixels: T passes 1e-4 in
    # small steps there, and up to 16 pixels may meet the band)
    assert ref["ties"].mean() <= (0.01 if size == SIX else 1.0 / 16.0), int(ref["ties"].sum())
    assert np.abs(ref["v_intrinsics"]).max() > 1e-6
    ctx = ba.Context(dev)
    try:
        node = gp._node(ba, ctx, dev, sc, cp, w, h, mip, smooth)
        g = node.backward(torch.from_numpy(ref["v_output"].astype(np.float32)).to(dev), intrinsics=True)
        u = util.hip_camera(ba, cp).uniforms((w, h))
        assert np.abs(np.array([u.fx, u.fy, u.cx, u.cy]) - ref["k"]).max() <= 1e-5 * ref["k"].max()
        assert set(g) == {"v_transforms", "v_sh_coeffs", "v_raw_opacities", "v_refine_weight", "v_intrinsics"}
        _check("%s n=%d mip=%d smooth=%d" % (model, n, mip, smooth), g["v_intrinsics"].cpu().numpy(), ref["v_intrinsics"], ref["S"])
    finally:
        ctx.close()


def test_splat_outputs_and_the_pose_gradient_are_bit_for_bit(dev):
    """Retained forwards of the one-tile scene: the four splat outputs of the intrinsics backward are bit-equal to
    bh_render_backward_saved's, pose=True with intrinsics=True returns the v_viewmat pose=True alone returns, the four of
    v_intrinsics do not depend on the pose pass, and two calls give the same four, to the bit."""
    import brush_amd as ba
    n, w, h, seed = ONE
    sc, cp = gp._scene(n, w, h, seed, DEG, "pinhole")
    vt = torch.from_numpy(gp._v_output(h, w, 1)).to(dev)
    ctx = ba.Context(dev)
    try:
        nodes = [gp._node(ba, ctx, dev, sc, cp, w, h, False, False, retain=True) for _ in range(4)]
        plain = nodes[0].backward(vt)
        intr = nodes[1].backward(vt, intrinsics=True)
        posed = nodes[2].backward(vt, pose=True)
        both = nodes[3].backward(vt, pose=True, intrinsics=True)
        again = nodes[3].backward(vt, pose=True, intrinsics=True)
        assert float(plain["v_transforms"].abs().max()) > 0
        for k in plain:
            for other in (intr, both):
                assert torch.equal(plain[k].view(torch.int32), other[k].view(torch.int32)), k
        assert float(posed["v_viewmat"].abs().max()) > 0 and float(intr["v_intrinsics"].abs().min()) > 0
        assert torch.equal(posed["v_viewmat"].view(torch.int32), both["v_viewmat"].view(torch.int32))
        assert torch.equal(intr["v_intrinsics"].view(torch.int32), both["v_intrinsics"].view(torch.int32))
        assert torch.equal(both["v_intrinsics"].view(torch.int32), again["v_intrinsics"].view(torch.int32))
        for nd in nodes:
            nd.release()
    finally:
        ctx.close()


def _device_masses(ba, ctx, node, cam, dev, blur):
    """The L1 masses of the four entries from the device's OWN rows, in f64: the header's per-splat formula on v_combined (the
    RasterizeGrads rows the pass read) and the projected rows (xy, conic), with A = conic^-1 - blur I and d = (xy - c) / f.  (A mass
    only sets the scale of a bound: the f32 inversion of the conic is accurate enough for that.)"""
    from brush_amd.host import _view
    nl = node.out.num_listed_splats
    vc = _view(ctx.lib.bh_last_v_combined(ctx._h), (nl, 10), torch.float32, dev).cpu().numpy().astype(np.float64)
    pr = _view(node.out.projected, (nl, 9), torch.float32, dev).cpu().numpy().astype(np.float64)
    conic = pr[:, 2:5]
    det = conic[:, 0] * conic[:, 2] - conic[:, 1] ** 2
    cov = np.stack([conic[:, 2] / det, -conic[:, 1] / det, conic[:, 0] / det], -1)
    cov_raw = np.zeros((nl, 2, 2))
    cov_raw[:, 0, 0], cov_raw[:, 0, 1], cov_raw[:, 1, 1] = cov[:, 0] - blur, cov[:, 1], cov[:, 2] - blur
    k = np.array([cam.fx, cam.fy, cam.cx, cam.cy], np.float64)
    d = (pr[:, 0:2] - k[2:4]) / k[0:2]
    per = intrinsics_ref.header_formula(k, vc[:, 0:2], vc[:, 2:5], conic, cov_raw, d)
    return np.abs(per).sum(0), per.sum(0)


def test_run_to_run_and_list_policy(dev):
    """tests/test_gpu_pose.py's frame (60000 splats, 320x208: atomics in K17, cut lists on the second frame of a named view)."""
    import brush_amd as ba
    n, w, h = 60000, 320, 208
    cp0 = synth.default_camera_params(w, h)
    tans = (math.tan(cp0["fov_x"] / 2.0), math.tan(cp0["fov_y"] / 2.0))
    sc = synth.make_scene(n, 0x56, sh_degree=1, log_scale_range=(math.log(0.03), math.log(0.3)), tan_half_fov=tans)
    cp = {k: v for k, v in cp0.items() if k not in ("img_w", "img_h")}
    vt = torch.from_numpy(gp._v_output(h, w, 9)).to(dev)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    cam = util.hip_camera(ba, cp)
    ctx = ba.Context(dev)
    try:
        base = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, retain=True)
        g0 = base.backward(vt, intrinsics=True)
        mass, own = _device_masses(ba, ctx, base, cam.uniforms((w, h)), dev, 0.3)
        g1 = base.backward(vt, intrinsics=True)
        base.release()
        v0 = g0["v_intrinsics"].cpu().numpy().astype(np.float64)
        assert (mass > 0).all()
        print("f64 formula on the device's rows: %s, the pass: %s, masses %s" % (own, v0, mass))
        _check("run to run", g1["v_intrinsics"].cpu().numpy(), v0, mass)
        ba.set_view_id(0xD0, ctx)
        ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
        cut = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
        assert cut.out.tile_offsets_far and cut.out.num_listed_splats < cut.out.num_visible, "not a cut frame"
        gc = cut.backward(vt, intrinsics=True)
        _check("cut lists", gc["v_intrinsics"].cpu().numpy(), v0, mass)
    finally:
        ctx.close()


def test_empty_view_writes_four_zeros(dev):
    import brush_amd as ba
    from brush_amd.host import _ptr
    n, w, h, seed = gp.SMALL
    sc, cp = gp._scene(n, w, h, seed, 0, "pinhole")
    cp["rot_xyzw"] = util.quat_from_axis_angle((0.0, 1.0, 0.0), math.pi)   # turned away from the scene
    ctx = ba.Context(dev)
    try:
        node = gp._node(ba, ctx, dev, sc, cp, w, h, False, False)
        assert node.out.num_visible == 0
        spl = node.splats
        r_t, r_o = node._folded
        outs = [torch.empty((n, 10), device=dev), torch.empty((n, 1, 3), device=dev), torch.empty((n,), device=dev), torch.empty((n,), device=dev)]
        vv = torch.full((12,), float("nan"), device=dev)
        vi = torch.full((4,), float("nan"), device=dev)
        vt = torch.from_numpy(gp._v_output(h, w, 2)).to(dev)
        ctx.check(ctx.lib.bh_render_backward_intrinsics_saved(ctx._h, C.byref(node.out), _ptr(vt), _ptr(r_t), _ptr(spl.sh_coeffs), _ptr(r_o),
                                                              _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), _ptr(vv), _ptr(vi)))
        assert torch.equal(vi, torch.zeros(4, device=dev)) and torch.equal(vv, torch.zeros(12, device=dev))
        vi.fill_(float("nan"))
        ctx.check(ctx.lib.bh_render_backward_intrinsics_saved(ctx._h, C.byref(node.out), _ptr(vt), _ptr(r_t), _ptr(spl.sh_coeffs), _ptr(r_o),
                                                              _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), None, _ptr(vi)))
        assert torch.equal(vi, torch.zeros(4, device=dev))
    finally:
        ctx.close()


@pytest.mark.parametrize("model,mip", [("pinhole", False), ("tpf", True)])
def test_with_a_depth_cotangent_matches_the_reference_extended_by_the_depth_term(dev, model, mip):
    """<v_output, image> + <v_depth, expected depth> through bh_render_backward_camera_saved, against tests/intrinsics_ref.py with
    the depth term added in f64 (tests/depth_ref.py's expected depth; n = 600 walks in about a second, so the reference is used and
    not finite differences of the device's forward).  The four splat outputs are bh_render_backward_depth_saved's; the depth
    cotangent moves the result by more than the bound, so the check sees the term."""
    import brush_amd as ba
    n, w, h, _ = SIX
    sc, cp, ref = _reference(SIX, model, mip, True, True)
    _, _, colour = _reference(SIX, model, mip, True)
    assert (np.abs(ref["v_intrinsics"] - colour["v_intrinsics"]) > 10 * TOL * ref["S"]).any()
    ctx = ba.Context(dev)
    try:
        node = gp._node(ba, ctx, dev, sc, cp, w, h, mip, True, retain=True)
        vo = torch.from_numpy(ref["v_output"].astype(np.float32)).to(dev)
        vd = torch.from_numpy(ref["v_depth"].astype(np.float32)).to(dev)
        g = node.backward(vo, v_depth=vd, depth_mode="expected", intrinsics=True)
        _check("%s mip=%d colour + depth" % (model, mip), g["v_intrinsics"].cpu().numpy(), ref["v_intrinsics"], ref["S"])
        g_d = node.backward(None, v_depth=vd, depth_mode="expected", intrinsics=True)   # the depth term alone: no K17
        _check("%s mip=%d depth alone" % (model, mip), g_d["v_intrinsics"].cpu().numpy(), ref["v_intrinsics"] - colour["v_intrinsics"],
               ref["S"] + colour["S"])
        with pytest.raises(ba.BrushHipError):
            node.backward(vo, v_depth=vd, pose=True, intrinsics=True)   # the pose gradient is the colour term's alone
        node.release()
    finally:
        ctx.close()
