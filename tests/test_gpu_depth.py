"""Depth maps on the GPU (include/brush_hip_depth.h): accumulated depth against the oracle-pinned colour path,
all three modes against the float64 restatement tests/depth_ref.py, bit identity across list policies / calls / retained forwards /
tile-row windows, gradients against autograd and against the oracle's backward of a depth-coloured scene, and the refusals.

Tie pixels of check 2 (float64 reference alone, counted on the CPU for the cases below, 64 x 48 = 3072 pixels, cap 0.5 % = 15):
pinhole 3 / 3 / 3, pinhole Mip 4 / 4 / 5, kb4 0 / 0 / 0, kb4 Mip 8 / 8 / 9 (accumulated / expected / median); with the smooth cut-off
(RasterPass.BackwardSmoothCutoff, smooth=True in the reference): 3 / 3 / 3, 4 / 4 / 5, 0 / 0 / 0, 8 / 8 / 10.

Smooth cut-off cases that are left out because the kernels miss TOL on them ("Expected depth under the smooth
cut-off"; measured on an MI355X, accumulated and median depth of the same frames are within 2.3e-6 and 1.4e-7 of the frame's
maximum):
  * expected depth of the two Mip frames: 1.13e-4 (pinhole Mip) and 1.64e-4 (kb4 Mip) of the frame's maximum against TOL = 1e-4
    (the two frames without Mip: 1.0e-5 and 3.4e-5, kept);
  * the gradient of an expected-depth term, relative L-inf of the means block: 1.5e-4 (pinhole), 4.3e-4 (pinhole Mip), 1.1e-3 (kb4),
    8.4e-3 (kb4 Mip) against TOL (accumulated depth: at most 2.1e-5 in every block, kept)."""
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import depth_ref
import util

pytestmark = pytest.mark.gpu
C0 = 0.2820947917738781
TOL = 1e-4   # the project's gradient-grade figure
MODES = ("accumulated", "expected", "median")


def _scene(n, w, h, seed, z_range=(2.0, 12.0), scales=(0.03, 0.3), sh_degree=0):
    cp = synth.default_camera_params(w, h)
    tans = (math.tan(cp["fov_x"] / 2.0), math.tan(cp["fov_y"] / 2.0))
    return synth.make_scene(n, seed, sh_degree=sh_degree, log_scale_range=(math.log(scales[0]), math.log(scales[1])), z_range=z_range, tan_half_fov=tans), cp


def _depth_coloured(sc):
    """SH degree 0 colour == camera z for the default camera (origin, identity rotation: z_cam is the mean's z exactly)."""
    z = sc["transforms"][:, 2].astype(np.float32)
    sh = np.repeat(((z - np.float32(0.5)) / np.float32(C0)).astype(np.float32)[:, None, None], 3, axis=2)
    return dict(transforms=sc["transforms"], sh=np.ascontiguousarray(sh), raw_opac=sc["raw_opac"])


def _oracle(bo, sc, cp, w, h, flags=None):
    p = {k: v for k, v in cp.items() if k not in ("img_w", "img_h")}
    return bo.Render().forward(bo.camera(img_w=w, img_h=h, **p), sc["transforms"], sc["sh"], sc["raw_opac"], bg=(0.0, 0.0, 0.0),
                               flags=bo.FLAG_BWD_INFO if flags is None else flags)


def _longest_list(node, aux_far=True):
    from brush_amd import host
    out = node.out
    to = host._view(out.tile_offsets, (out.num_tiles, 2), torch.int32, node.splats.device).cpu().numpy().astype(np.int64)
    n = to[:, 1] - to[:, 0]
    if out.tile_offsets_far:
        tf = host._view(out.tile_offsets_far, (out.num_tiles, 2), torch.int32, node.splats.device).cpu().numpy().astype(np.int64)
        n = n + (tf[:, 1] - tf[:, 0])
    return int(max(n.max(), 0))


# ---- 1. accumulated depth against the oracle-pinned colour path -----------------------------------------------------------
@pytest.mark.parametrize("n,w,h,seed", [(20000, 256, 160, 0xD1), (3000, 123, 82, 0xD2)])
def test_accumulated_depth_is_the_oracles_depth_coloured_image(dev, oracle_lib, n, w, h, seed):
    """|dD| <= (n + 3) 2^-24 (z_max + 0.5) per pixel, n = the frame's longest tile list: one rounding of sh, one of the colour
    fma, one per accumulation step (derived, not measured)."""
    import brush_amd as ba
    sc, cp = _scene(n, w, h, seed)
    dc = _depth_coloured(sc)
    ref = _oracle(oracle_lib, dc, cp, w, h)
    spl = ba.Splats(dc["transforms"], dc["sh"], dc["raw_opac"], device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), ctx=ctx)
        d = node.depth("accumulated").cpu().numpy()
        img = node.img.cpu().numpy()
        zmax = float(sc["transforms"][:, 2].max())
        bound = (_longest_list(node) + 3) * 2.0 ** -24 * (zmax + 0.5)
        err = float(np.abs(d.astype(np.float64) - ref.image()[..., 0].astype(np.float64)).max())
        print("accumulated depth vs oracle colour: max |dD| = %.3e, bound %.3e (longest list %d)" % (err, bound, _longest_list(node)))
        assert float(d.max()) > 1.0
        assert err <= bound, (err, bound)
        # ... and against the HIP colour image of the same frame, whose channel 0 it restates
        assert float(np.abs(d.astype(np.float64) - img[..., 0]).max()) <= bound
        # expected == accumulated / alpha, exactly; 0 where alpha == 0
        e = node.depth("expected")
        a = node.img[..., 3]
        want = torch.where(a == 0, torch.zeros_like(a), torch.from_numpy(d).to(dev) / torch.where(a == 0, torch.ones_like(a), a))
        assert torch.equal(e, want)
    finally:
        ctx.close()


# ---- 2. all three modes against the float64 restatement ---------------------------------------------------------------------
REF_CASES = [("pinhole", False), ("pinhole", True), ("kb4", False), ("kb4", True)]


def _params(cases, left_out=()):
    """Every case with the hard cut-off under the id it always had, then with the smooth one ('-smooth'), but for `left_out`."""
    ids = ["-".join(str(x) for x in c) for c in cases]
    hard = [pytest.param(*c, False, id=i) for c, i in zip(cases, ids)]
    return hard + [pytest.param(*c, True, id=i + "-smooth") for c, i in zip(cases, ids) if c not in left_out]


def _ref_case(model):
    w, h = 64, 48
    sc, cp = _scene(300, w, h, 0xE5, z_range=(2.0, 9.0), scales=(0.05, 0.4))
    cp = {k: v for k, v in cp.items() if k not in ("img_w", "img_h")}
    cp["pos"] = (0.15, -0.1, -0.4)
    cp["rot_xyzw"] = util.quat_from_axis_angle((0.3, 1.0, 0.1), 0.08)
    if model != "pinhole":
        cp["model"], cp["dist"] = util.REF_LENSES[model]
    return sc, cp, w, h


def _ref_render(sc, cp, w, h, mip, smooth=False):
    tr, sh, op = [torch.tensor(np.asarray(sc[k], np.float64), requires_grad=True) for k in ("transforms", "sh", "raw_opac")]
    with torch.enable_grad():
        out = depth_ref.render(tr, sh, op, cp, w, h, intrinsics=depth_ref.intrinsics(cp, w, h), mip=mip, smooth=smooth)
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}


def _pass(ba, smooth):
    return ba.RasterPass.BackwardSmoothCutoff if smooth else ba.RasterPass.Backward


@pytest.mark.parametrize("model,mip,smooth", _params(REF_CASES, left_out=[("pinhole", True), ("kb4", True)]))
def test_depth_modes_match_the_float64_reference(dev, model, mip, smooth):
    import brush_amd as ba
    sc, cp, w, h = _ref_case(model)
    ref = _ref_render(sc, cp, w, h, mip, smooth)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], render_mip=mip, device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), pass_=_pass(ba, smooth), ctx=ctx)
        assert float(np.abs(node.img.cpu().numpy() - ref["img"].numpy()).max()) <= 1e-5
        zmax = float(ref["acc"].max().clamp(min=ref["expected"].max()))
        for mode in MODES:
            got = node.depth(mode).cpu().numpy().astype(np.float64)
            want = ref["acc" if mode == "accumulated" else mode].numpy()
            skip = depth_ref.tie_mask(ref, mode).numpy()
            assert skip.mean() <= 0.005, (mode, int(skip.sum()))
            err = np.abs(got - want)[~skip]
            print("%s %s mip=%d smooth=%d: max err / frame max = %.3e, %d tie pixels" % (model, mode, mip, smooth, err.max() / zmax, int(skip.sum())))
            assert float(want.max()) > 1.0
            assert err.max() <= TOL * zmax, (mode, float(err.max()), zmax)
    finally:
        ctx.close()


# ---- 3. bit identity ------------------------------------------------------------------------------------------------------
def test_depth_does_not_depend_on_the_list_policy_or_the_call(dev):
    import brush_amd as ba
    n, w, h = 60000, 320, 208
    sc, cp = _scene(n, w, h, 0x56)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    cam = util.hip_camera(ba, cp)
    ctx = ba.Context(dev)
    try:
        base = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx)
        want = {m: base.depth(m).clone() for m in MODES}
        for m in MODES:
            assert torch.equal(base.depth(m), want[m]), "two calls on one saved state"
            assert float(want[m].max()) > 1.0
        img = base.img.clone()
        # per-tile cut lists: the second sliced frame of a view
        ba.set_view_id(0xD0, ctx)
        first = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
        assert first.out.tile_offsets_far is None or first.out.list_budget == first.out.num_intersections
        cut = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
        assert cut.out.tile_offsets_far and cut.out.num_listed_splats < cut.out.num_visible, "not a cut frame"
        assert torch.equal(cut.img, img)
        for m in MODES:
            assert torch.equal(cut.depth(m), want[m]), ("cut lists", m)
        # a near + far frame with a fixed near share
        ba.set_view_id(0, ctx)
        ba.host.set_list_slicing(0.5, ctx)
        try:
            half = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
            assert half.out.tile_offsets_far
            assert torch.equal(half.img, img)
            for m in MODES:
                assert torch.equal(half.depth(m), want[m]), ("near + far", m)
        finally:
            ba.host.set_list_slicing(0.0, ctx)
        # a retained forward, after another forward has run
        kept = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, retain=True)
        other = dict(cp)
        other["pos"] = (1.0, -0.2, -1.0)
        ba.render_splats(spl, util.hip_camera(ba, other), (w, h), (0, 0, 0), ba.RasterPass.Backward, ctx=ctx, copy=False)
        for m in MODES:
            assert torch.equal(kept.depth(m), want[m]), ("retained", m)
        kept.release()
        # two tile-row windows stitched together
        rows = (h + 15) // 16
        for m in MODES:
            out = torch.full((h, w), -7.0, device=dev)
            for win in ((0, 5), (5, rows)):
                part = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, tile_rows=win)
                ba.render_depth(part, m, out=out)
            assert torch.equal(out, want[m]), ("windows", m)
    finally:
        ctx.close()


# ---- 4. gradients -----------------------------------------------------------------------------------------------------------
def _assert_close(name, a, b, tol=TOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.isfinite(a).all(), name
    rel = util.rel_linf(a, b)
    print("%s: rel linf %.3e" % (name, rel))
    assert rel <= tol, (name, rel)


def _assert_grads(tag, g, tr, op):
    vt = g["v_transforms"].cpu().numpy()
    for nm, sl in (("means", slice(0, 3)), ("quats", slice(3, 7)), ("log_scales", slice(7, 10))):
        _assert_close("%s %s" % (tag, nm), vt[:, sl], tr[:, sl])
    _assert_close("%s raw_opac" % tag, g["v_raw_opacities"].cpu().numpy(), op)


@pytest.mark.parametrize("model,mip,mode,smooth", _params([c + (m,) for m in ("accumulated", "expected") for c in REF_CASES],
                                                         left_out=[c + ("expected",) for c in REF_CASES]))
def test_depth_gradients_match_autograd(dev, model, mip, mode, smooth):
    import brush_amd as ba
    sc, cp, w, h = _ref_case(model)
    rng = np.random.default_rng(17)
    v = (rng.uniform(-1.0, 1.0, (h, w)) / (h * w)).astype(np.float32)
    _, g_tr, g_sh, g_op = depth_ref.gradients(sc, cp, w, h, v, mode, intrinsics=depth_ref.intrinsics(cp, w, h), mip=mip, smooth=smooth)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], render_mip=mip, device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), pass_=_pass(ba, smooth), ctx=ctx)
        g = node.backward(None, v_depth=torch.from_numpy(v).to(dev), depth_mode=mode)
        _assert_grads("%s %s mip=%d smooth=%d" % (model, mode, mip, smooth), g, g_tr, g_op)
        assert float(g["v_sh_coeffs"].abs().max()) == 0.0 and float(g["v_refine_weight"].abs().max()) == 0.0
    finally:
        ctx.close()


def test_accumulated_gradients_match_the_oracles_depth_coloured_backward(dev, oracle_lib):
    """The oracle's backward of the depth-coloured scene with v_output = v_depth on channel 0: its v_transforms plus
    (view-matrix row 2) v_sh[:,0,0] / C0 is the expected v_transforms, its v_raw_opacities the expected one; v_output and v_depth
    together give the sum of the two alone; the refine weight is the colour term's."""
    import brush_amd as ba
    n, w, h = 10000, 256, 160
    sc, cp = _scene(n, w, h, 0xD4, sh_degree=1)
    dc = _depth_coloured(sc)
    rng = np.random.default_rng(23)
    v = (rng.uniform(-1.0, 1.0, (h, w)) / (h * w)).astype(np.float32)
    v_out = np.zeros((h, w, 4), np.float32)
    v_out[..., 0] = v
    ref = _oracle(oracle_lib, dc, cp, w, h)
    ref.backward(v_out)
    want_t = ref.get("v_transforms").reshape(n, 10).astype(np.float64).copy()
    want_t[:, 2] += ref.get("v_coeffs").reshape(n, 1, 3)[:, 0, 0].astype(np.float64) / C0   # default camera: row 2 of the view matrix = (0, 0, 1)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)   # any colour: depth does not read it
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), ctx=ctx)
        vd = torch.from_numpy(v).to(dev)
        g_d = node.backward(None, v_depth=vd, depth_mode="accumulated")
        _assert_grads("oracle depth-coloured", g_d, want_t, ref.get("v_raw_opac"))
        # (c) both terms together == the sum of the two alone, (d) the refine weight is the colour term's alone
        vo = torch.from_numpy((rng.uniform(-1.0, 1.0, (h, w, 4)) / (h * w)).astype(np.float32)).to(dev)
        g_c = node.backward(vo)
        g_c_again = node.backward(vo)
        for mode in ("accumulated", "expected"):
            g_1 = node.backward(None, v_depth=vd, depth_mode=mode)
            g_b = node.backward(vo, v_depth=vd, depth_mode=mode)
            for k in ("v_transforms", "v_sh_coeffs", "v_raw_opacities"):
                _assert_close("sum %s %s" % (mode, k), g_b[k].cpu().numpy(), (g_c[k].double() + g_1[k].double()).cpu().numpy())
            # (d) the depth kernels never touch the refine column: they write columns 0-4 and 8 of the accumulator and v_z, and a
            # depth-only backward leaves the refine weight exactly 0 (test_depth_gradients_match_autograd asserts it) — that is what
            # carries (d).  Two runs WITH a colour term can only be compared to K17's own run-to-run noise:  K17 adds it up with float atomics, so two runs of the colour
            # term ALONE agree only to the reordering noise of a short sum (a few 2^-24): equal bits where they do, else that noise
            if torch.equal(g_c_again["v_refine_weight"], g_c["v_refine_weight"]):
                assert torch.equal(g_b["v_refine_weight"], g_c["v_refine_weight"])
            _assert_close("refine %s" % mode, g_b["v_refine_weight"].cpu().numpy(), g_c["v_refine_weight"].cpu().numpy(), tol=1e-6)
        # 5a. a depth render between a forward and its backward disturbs nothing
        node.depth("median")
        g_c2 = node.backward(vo)
        for k in ("v_transforms", "v_sh_coeffs", "v_raw_opacities", "v_refine_weight"):
            _assert_close("undisturbed %s" % k, g_c2[k].cpu().numpy(), g_c[k].cpu().numpy())
    finally:
        ctx.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    import ctypes as C
    import brush_amd as ba
    from brush_amd import host
    sc = util.base_scene()
    cam = util.hip_camera(ba, util.STD_CAM)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, cam, (32, 32), ctx=ctx)
        with pytest.raises(ba.BrushHipError, match="mode"):
            node.depth(3)
        with pytest.raises(ba.BrushHipError, match="median"):
            node.backward(None, v_depth=torch.zeros((32, 32), device=dev), depth_mode="median")
        with pytest.raises(ba.BrushHipError, match="mode"):
            node.backward(None, v_depth=torch.zeros((32, 32), device=dev), depth_mode=3)
        with pytest.raises(ba.BrushHipError, match="out"):
            ba.render_depth(node, "expected", out=torch.zeros((32, 31), device=dev))
        with pytest.raises(ba.BrushHipError, match="out"):
            ba.render_depth(node, "expected", out=torch.zeros((32, 32)))
        # a forward-only frame
        _, out, folded = host._forward(ctx, spl, cam, (32, 32), (0, 0, 0), ba.RasterPass.Forward)
        d = torch.zeros((32, 32), device=dev)
        rc = ctx.lib.bh_render_depth(ctx._h, C.byref(out), 0, C.c_void_p(d.data_ptr()))
        assert rc == -1 and b"BWD_INFO" in ctx.lib.bh_last_error(ctx._h)
        p = C.c_void_p(d.data_ptr())
        rc = ctx.lib.bh_render_backward_depth_saved(ctx._h, C.byref(out), None, p, 0, p, p, p, p, p, p, p)   # (refused before any pointer is read)
        assert rc == -1 and b"BWD_INFO" in ctx.lib.bh_last_error(ctx._h)
        # a stale BhRenderOut: another forward has run since
        with pytest.raises(ba.BrushHipError, match="stale"):
            node.depth("expected")
        with pytest.raises(ba.BrushHipError, match="stale"):
            node.backward(None, v_depth=d)
    finally:
        ctx.close()


# ---- 5b. depth renders between training steps ---------------------------------------------------------------------------------
def test_interleaved_depth_renders_do_not_change_training(dev):
    """The one-tile deterministic set-up of test_gpu_eval.py::test_interleaved_evals_do_not_change_training (16x16, 6000 splats,
    seed 77, 9 steps), with, after every step, the depth maps of the step's own forward (bh_last_render_out) and of a larger frame
    at another camera, and a depth backward of that frame: parameters, moments and refine statistics equal a run without, bit for
    bit."""
    import ctypes as C
    import brush_amd as ba
    from brush_amd import _ffi, host
    n, w, h = 6000, 16, 16
    sc = synth.make_scene(n, 0xD0A, sh_degree=1, log_scale_range=(math.log(0.05), math.log(0.4)),
                          tan_half_fov=(math.tan(math.radians(50)), math.tan(math.radians(50))))
    cams = []
    for i in range(3):
        c = dict(synth.default_camera_params(w, h))
        c["rot_xyzw"] = util.quat_from_axis_angle((0, 1, 0), math.radians(-35 + 35 * i))
        cams.append(c)
    gt = torch.from_numpy(synth.synthetic_gt_packed(w, h).view(np.int32)).to(dev)
    ew, eh = 200, 136
    other = util.hip_camera(ba, synth.default_camera_params(ew, eh))
    runs = {}
    for key in ("plain", "with_depth"):
        ctx = ba.Context(dev)
        try:
            spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
            tr = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=3.0, ctx=ctx, seed=77)
            for s in range(9):
                tr.step(ba.SceneBatch(gt, util.hip_camera(ba, cams[s % len(cams)])), spl)
                if key == "with_depth":
                    last = _ffi.BhRenderOut()
                    ctx.check(ctx.lib.bh_last_render_out(ctx._h, C.byref(last)))
                    own = torch.zeros((h, w), device=dev)
                    for m in range(3):
                        ctx.check(ctx.lib.bh_render_depth(ctx._h, C.byref(last), m, C.c_void_p(own.data_ptr())))
                    assert bool(torch.isfinite(own).all())
                    node = ba.render_splats_diff(spl, other, (ew, eh), ctx=ctx)
                    d = node.depth("expected")
                    assert float(d.max()) > 0.0
                    g = node.backward(None, v_depth=torch.full((eh, ew), 1.0 / (ew * eh), device=dev))
                    assert bool(torch.isfinite(g["v_transforms"]).all())
            ctx.sync()
            out = {"transforms": spl.transforms.clone(), "sh": spl.sh_coeffs.clone(), "opac": spl.raw_opacities.clone()}
            out.update({k: v.clone() for k, v in tr.state.items()})
            runs[key] = out
        finally:
            ctx.close()
    a, b = runs["plain"], runs["with_depth"]
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
