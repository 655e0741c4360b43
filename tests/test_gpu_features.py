"""Feature maps on the GPU (include/brush_hip_features.h): bit identity with the colour image whose blend they
restate and with the accumulated normal map (the map skeleton's other three-channel traits struct), the map and its gradients against the float64 restatement tests/feature_ref.py, the feature-only backward against the
oracle-pinned colour backward, bit identity across list policies / calls / retained forwards / tile-row windows, the two fused
losses against their numpy restatements, and the edges.

Channel counts of every forward / backward check: {1, 3, CH - 1, CH, CH + 1, 2 CH + 3} for each instantiated chunk width CH (4, 8,
16), and 256.  One float64 reference per case is rendered with 256 channels and shared: channels are independent blends, so the
reference of C channels is its first C columns, and its gradient goes through the per-splat weights (feature_ref.gradients).

Tie pixels (depth_ref.tie_mask(ref, "accumulated"): the decisions are the colour blend's, so the counts are those recorded in
tests/test_gpu_depth.py for accumulated depth): 3 / 4 / 0 / 8 of 3072 for pinhole / pinhole Mip / kb4 / kb4 Mip, hard and smooth
cut-off; cap 0.5 % = 15.

Loss bounds (eps = 2^-24, one f32 rounding; c = f32(weight / count); brush_hip_features.h states the arithmetic):
  v_map, L1             sign(d) c with d the f32 difference the restatement forms too: no rounding at all        -> bit-exact
  loss[0], L1           per-channel f32 |d| as the restatement's; the f64 sum of N C terms (N C 2^-52 relative); the rounding of c
                        and the final rounding to f32                                                            -> 3 eps |loss|
  v_map, cross-entropy  e_c / s - [c == label] in f64 from f64 exp of exact differences: each exp within 1 ulp (2^-52 relative),
                        the sum of C of them C 2^-52, so the bracket is off by at most (C + 8) 2^-52 ABSOLUTE (it cancels to
                        p - 1 at the label); then one rounding to f32, the rounding of c and one f32 product: 3 eps |v|; a result
                        below the smallest normal f32 may lose everything: 2^-126 more
                        -> |delta| <= 3 eps (1 + 2 eps) |v| + c (C + 8) 2^-52 + 2^-126   (the three roundings compounded)
  loss[0], cross-entropy  per pixel log(s) + (m - F_label) in f64: (C + 8) 2^-52 (1 + |m| + |F_label|) absolute; the rounding of c
                        and the final rounding                     -> 3 eps |loss| + c N (C + 8) 2^-52 (1 + 2 max|F|)
  the valid count       exact
Measured on an MI355X: maps within 2.7e-6 of max|F|, gradient blocks within 1.2e-5, |loss - restatement| at most 0.21
of its bound, the cross-entropy gradient at most 0.75 of its."""
import functools
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import depth_ref
import feature_ref
import util

pytestmark = pytest.mark.gpu
C0 = 0.2820947917738781
TOL = 1e-4   # the project's gradient-grade figure
EPS = 2.0 ** -24
CHUNKS = (4, 8, 16)   # the instantiated chunk widths (features.hip)
CHANNELS = sorted({1, 3, 256} | {c for ch in CHUNKS for c in (ch - 1, ch, ch + 1, 2 * ch + 3)})
REF_CASES = [("pinhole", False), ("pinhole", True), ("kb4", False), ("kb4", True)]
CASE_PARAMS = [pytest.param(m, mip, s, id="%s-%s%s" % (m, mip, "-smooth" if s else "")) for s in (False, True) for m, mip in REF_CASES]


def _scene(n, w, h, seed, z_range=(2.0, 12.0), scales=(0.03, 0.3), sh_degree=0):
    cp = synth.default_camera_params(w, h)
    tans = (math.tan(cp["fov_x"] / 2.0), math.tan(cp["fov_y"] / 2.0))
    return synth.make_scene(n, seed, sh_degree=sh_degree, log_scale_range=(math.log(scales[0]), math.log(scales[1])), z_range=z_range, tan_half_fov=tans), cp


def _ref_case(model):
    """tests/test_gpu_depth.py::_ref_case: 300 splats, 64 x 48, lists longer than one 64-entry batch."""
    w, h = 64, 48
    sc, cp = _scene(300, w, h, 0xE5, z_range=(2.0, 9.0), scales=(0.05, 0.4))
    cp = {k: v for k, v in cp.items() if k not in ("img_w", "img_h")}
    cp["pos"] = (0.15, -0.1, -0.4)
    cp["rot_xyzw"] = util.quat_from_axis_angle((0.3, 1.0, 0.1), 0.08)
    if model != "pinhole":
        cp["model"], cp["dist"] = util.REF_LENSES[model]
    return sc, cp, w, h


def _pass(ba, smooth):
    return ba.RasterPass.BackwardSmoothCutoff if smooth else ba.RasterPass.Backward


@functools.lru_cache(maxsize=None)
def _reference(model, mip, smooth):
    """The float64 reference of a case with 256 channels drawn from N(0, 1), rendered once and never written: (scene, camera, w, h,
    features [N,256] f32, leaves (tr, sh, op), out) with out["vis"] and out["img"] carrying the graph."""
    sc, cp, w, h = _ref_case(model)
    feats = np.random.default_rng(0xFEA7).normal(0.0, 1.0, (sc["transforms"].shape[0], 256)).astype(np.float32)
    feats.setflags(write=False)
    leaves = [torch.tensor(np.asarray(sc[k], np.float64), requires_grad=True) for k in ("transforms", "sh", "raw_opac")]
    with torch.enable_grad():
        out = feature_ref.render(*leaves, torch.tensor(feats.astype(np.float64)), cp, w, h, intrinsics=depth_ref.intrinsics(cp, w, h), mip=mip, smooth=smooth,
                                 map_grad=False)
    return sc, cp, w, h, feats, leaves, out


def _listed(node):
    """(projected [Nl,9], global ids [Nl] int64) of the node's listed splats."""
    from brush_amd import host
    out, dev = node.out, node.splats.device
    nl = out.num_listed_splats
    proj = host._view(out.projected, (nl, 9), torch.float32, dev)
    gid = host._view(out.global_from_compact_gid, (nl,), torch.int32, dev).long()
    return proj, gid


def _colour_features(node, n, extra=0, seed=1):
    """features [N, 3 + extra]: the projected rgb at the listed splats' rows (anything else elsewhere), N(0, 1) in the other channels."""
    dev = node.splats.device
    g = torch.Generator(device="cpu").manual_seed(seed)
    f = torch.randn((n, 3 + extra), generator=g).to(dev)
    proj, gid = _listed(node)
    f[gid, :3] = proj[:, 6:9]
    return f.contiguous()


# ---- 1. bit identity with the colour image ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,w,h,seed", [(20000, 256, 160, 0xD1), (3000, 123, 82, 0xD2)])
def test_rgb_features_are_the_colour_image_bit_for_bit(dev, n, w, h, seed):
    """Degree 0, black background: features = the projected rgb give img[..., :3] with torch.equal, alone and as the first three
    of CH + 1 and 2 CH + 3 channels (chunk boundaries and padding), whatever chunk width is forced."""
    import brush_amd as ba
    sc, cp = _scene(n, w, h, seed)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), ctx=ctx)
        rgb = node.img[..., :3].clone()
        assert float(rgb.max()) > 0.1
        f3 = _colour_features(node, n)
        assert torch.equal(node.features(f3), rgb)
        for extra in sorted({ch + 1 - 3 for ch in CHUNKS} | {2 * ch + 3 - 3 for ch in CHUNKS}):
            f = _colour_features(node, n, extra)
            got = node.features(f)
            assert torch.equal(got[..., :3], rgb), ("padded to", 3 + extra)
            assert float(got[..., 3:].abs().max()) > 0.0
        f = _colour_features(node, n, 16)
        for width in CHUNKS:
            ctx.set_option("feature_chunk", width)
            assert torch.equal(node.features(f3), rgb), ("forced chunk", width)
            assert torch.equal(node.features(f)[..., :3], rgb), ("forced chunk, 19 channels", width)
        ctx.set_option("feature_chunk", 0)
    finally:
        ctx.close()


@pytest.mark.parametrize("extra", [0, 16], ids=["C3", "C19"])
@pytest.mark.parametrize("smooth", [False, True], ids=["hard", "smooth"])
def test_normal_features_are_the_normal_map_bit_for_bit(dev, smooth, extra):
    """Features whose first three columns are the dense splat normals give the accumulated normal map with torch.equal, at the
    default chunk width and at every forced one (C = 19: two chunks at width 16, five at width 4): FeatureMap and NormalMap are two
    traits structs of one skeleton, and this holds them to each other through the arithmetic they share."""
    import brush_amd as ba
    n, w, h = 3000, 123, 82
    sc, cp = _scene(n, w, h, 0xD2)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    cam = util.hip_camera(ba, cp)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, cam, (w, h), pass_=_pass(ba, smooth), ctx=ctx)
        want = ba.render_normal(node, "accumulated").clone()
        assert float(want.abs().max()) > 0.1
        f = torch.randn((n, 3 + extra), generator=torch.Generator().manual_seed(11)).to(dev)
        f[:, :3] = ba.splat_normals(spl, cam, ctx=ctx)
        f = f.contiguous()
        for width in (0,) + CHUNKS:
            ctx.set_option("feature_chunk", width)
            got = node.features(f)
            assert torch.equal(got[..., :3], want), ("chunk width", width)
            assert extra == 0 or float(got[..., 3:].abs().max()) > 0.0
        ctx.set_option("feature_chunk", 0)
    finally:
        ctx.close()


# ---- 2. against the float64 restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,mip,smooth", CASE_PARAMS)
def test_feature_maps_match_the_float64_reference(dev, model, mip, smooth):
    import brush_amd as ba
    sc, cp, w, h, feats, _, ref = _reference(model, mip, smooth)
    skip = depth_ref.tie_mask(ref, "accumulated").numpy()
    assert skip.mean() <= 0.005, int(skip.sum())
    want_all = ref["feat"].numpy()
    assert float(want_all.min()) < -0.5 and float(want_all.max()) > 0.5   # negative features are not clamped
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], render_mip=mip, device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), pass_=_pass(ba, smooth), ctx=ctx)
        assert float(np.abs(node.img.cpu().numpy() - ref["img"].detach().numpy()).max()) <= 1e-5
        worst = 0.0
        for c in CHANNELS:
            got = node.features(torch.from_numpy(feats[:, :c].copy()).to(dev)).cpu().numpy().astype(np.float64)
            want = want_all[..., :c]
            fmax = float(np.abs(want).max())
            err = float(np.abs(got - want)[~skip].max())
            worst = max(worst, err / fmax)
            assert err <= TOL * fmax, (c, err, fmax)
        print("%s mip=%d smooth=%d: worst max err / max|F| = %.3e over %d channel counts, %d tie pixels" % (model, mip, smooth, worst, len(CHANNELS), int(skip.sum())))
    finally:
        ctx.close()


# ---- 3. bit identity across calls and policies -----------------------------------------------------------------------------------
def test_features_do_not_depend_on_the_list_policy_or_the_call(dev):
    import brush_amd as ba
    n, w, h, c = 60000, 320, 208, 19
    sc, cp = _scene(n, w, h, 0x56)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    cam = util.hip_camera(ba, cp)
    f = torch.randn((n, c), generator=torch.Generator().manual_seed(3)).to(dev)
    ctx = ba.Context(dev)
    try:
        base = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx)
        want = base.features(f).clone()
        assert torch.equal(base.features(f), want), "two calls on one saved state"
        assert float(want.abs().max()) > 0.5
        img = base.img.clone()
        # per-tile cut lists: the second sliced frame of a view
        ba.set_view_id(0xFE, ctx)
        first = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
        assert first.out.tile_offsets_far is None or first.out.list_budget == first.out.num_intersections
        cut = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
        assert cut.out.tile_offsets_far and cut.out.num_listed_splats < cut.out.num_visible, "not a cut frame"
        assert torch.equal(cut.img, img)
        assert torch.equal(cut.features(f), want), "cut lists"
        # a near + far frame with a fixed near share
        ba.set_view_id(0, ctx)
        ba.host.set_list_slicing(0.5, ctx)
        try:
            half = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
            assert half.out.tile_offsets_far
            assert torch.equal(half.features(f), want), "near + far"
        finally:
            ba.host.set_list_slicing(0.0, ctx)
        # a retained forward, after another forward has run
        kept = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, retain=True)
        other = dict(cp)
        other["pos"] = (1.0, -0.2, -1.0)
        ba.render_splats(spl, util.hip_camera(ba, other), (w, h), (0, 0, 0), ba.RasterPass.Backward, ctx=ctx, copy=False)
        assert torch.equal(kept.features(f), want), "retained"
        kept.release()
        # two tile-row windows stitched together: each writes its rows only
        rows = (h + 15) // 16
        out = torch.full((h, w, c), -7.0, device=dev)
        for win in ((0, 5), (5, rows)):
            part = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, tile_rows=win)
            ba.render_features(part, f, out=out)
            if win == (0, 5):
                assert bool((out[80:] == -7.0).all()) and torch.equal(out[:80], want[:80])
        assert torch.equal(out, want), "windows"
    finally:
        ctx.close()


# ---- 4. gradients against autograd -----------------------------------------------------------------------------------------------
def _assert_close(name, a, b, tol=TOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.isfinite(a).all(), name
    rel = util.rel_linf(a, b)
    assert rel <= tol, (name, rel)
    return rel


def _assert_grads(tag, g, tr, op, sh=None, vf=None):
    vt = g["v_transforms"].cpu().numpy()
    rels = [_assert_close("%s %s" % (tag, nm), vt[:, sl], tr[:, sl]) for nm, sl in (("means", slice(0, 3)), ("quats", slice(3, 7)), ("log_scales", slice(7, 10)))]
    rels.append(_assert_close("%s raw_opac" % tag, g["v_raw_opacities"].cpu().numpy(), op))
    if sh is not None:
        rels.append(_assert_close("%s sh" % tag, g["v_sh_coeffs"].cpu().numpy(), sh))
    if vf is not None:
        rels.append(_assert_close("%s v_features" % tag, g["v_features"].cpu().numpy(), vf))
    return max(rels)


@pytest.mark.parametrize("model,mip,smooth", CASE_PARAMS)
def test_feature_gradients_match_autograd(dev, model, mip, smooth):
    """<v_map, F> alone and together with <v_output, img>, every block within TOL relative L-inf."""
    import brush_amd as ba
    sc, cp, w, h, feats, (tr, sh, op), ref = _reference(model, mip, smooth)
    rng = np.random.default_rng(29)
    v_all = (rng.uniform(-1.0, 1.0, (h, w, 256)) / (h * w)).astype(np.float32)
    v_out = (rng.uniform(-1.0, 1.0, (h, w, 4)) / (h * w)).astype(np.float32)
    vis = ref["vis"]
    gi = torch.autograd.grad((ref["img"] * torch.tensor(v_out.astype(np.float64))).sum(), (tr, sh, op), retain_graph=True)
    gi_tr, gi_sh, gi_op = (x.numpy() for x in gi)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], render_mip=mip, device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), pass_=_pass(ba, smooth), ctx=ctx)
        vo = torch.from_numpy(v_out).to(dev)
        worst = 0.0
        for c in CHANNELS:
            f64, v64 = torch.tensor(feats[:, :c].astype(np.float64)), torch.tensor(v_all[..., :c].astype(np.float64))
            g_tr, g_op = torch.autograd.grad((vis * torch.einsum("hwc,nc->nhw", v64, f64)).sum(), (tr, op), retain_graph=True)
            g_tr, g_op = g_tr.numpy(), g_op.numpy()
            g_f = torch.einsum("nhw,hwc->nc", vis.detach(), v64).numpy()
            f = torch.from_numpy(feats[:, :c].copy()).to(dev)
            v = torch.from_numpy(np.ascontiguousarray(v_all[..., :c])).to(dev)
            tag = "%s mip=%d smooth=%d C=%d" % (model, mip, smooth, c)
            g = node.backward(None, v_features=v, features=f)
            worst = max(worst, _assert_grads(tag, g, g_tr, g_op, vf=g_f))
            assert float(g["v_sh_coeffs"].abs().max()) == 0.0 and float(g["v_refine_weight"].abs().max()) == 0.0
            g = node.backward(vo, v_features=v, features=f)
            worst = max(worst, _assert_grads(tag + " + colour", g, g_tr + gi_tr, g_op + gi_op, sh=gi_sh, vf=g_f))
        print("%s mip=%d smooth=%d: worst block rel linf %.3e over %d channel counts" % (model, mip, smooth, worst, len(CHANNELS)))
    finally:
        ctx.close()


# ---- 5. against the oracle-pinned colour backward ----------------------------------------------------------------------------------
def test_rgb_feature_backward_is_the_colour_backward(dev):
    """Degree 0, features = the projected rgb, v_map = v_output[..., :3], v_output[..., 3] = 0: the feature-only backward's
    v_transforms and v_raw_opacities are the colour-only backward's, and C0 v_features[gid] is v_sh_coeffs[gid, 0] where the colour is
    above its clamp at 0.  Each side is held to TOL against a reference elsewhere, hence 2 TOL."""
    import brush_amd as ba
    n, w, h = 10000, 256, 160
    sc, cp = _scene(n, w, h, 0xD4)
    rng = np.random.default_rng(31)
    v_out = np.zeros((h, w, 4), np.float32)
    v_out[..., :3] = rng.uniform(-1.0, 1.0, (h, w, 3)) / (h * w)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), ctx=ctx)
        vo = torch.from_numpy(v_out).to(dev)
        g_c = node.backward(vo)
        f3 = _colour_features(node, n)
        g_f = node.backward(None, v_features=vo[..., :3].contiguous(), features=f3)
        rel = _assert_grads("rgb features vs colour", g_f, g_c["v_transforms"].cpu().numpy(), g_c["v_raw_opacities"].cpu().numpy())
        proj, gid = _listed(node)
        lit = (proj[:, 6:9] > 0.0)
        assert float(lit.float().mean()) > 0.5
        a = (C0 * g_f["v_features"][gid].double() * lit).cpu().numpy()
        b = (g_c["v_sh_coeffs"][gid, 0].double() * lit).cpu().numpy()
        rel_sh = _assert_close("C0 v_features vs v_sh", a, b, tol=2 * TOL)
        print("rgb feature backward vs colour backward: geometry rel linf %.3e, C0 v_features vs v_sh %.3e" % (rel, rel_sh))
        assert rel <= 2 * TOL
    finally:
        ctx.close()


# ---- 6. losses -----------------------------------------------------------------------------------------------------------------------
LOSS_HW = (48, 64)


def _loss_inputs(c, kind):
    h, w = LOSS_HW
    rng = np.random.default_rng(100 + c)
    f = rng.normal(0.0, 1.5, (h, w, c)).astype(np.float32)
    if kind == "l1":
        t = rng.normal(0.0, 1.5, (h, w, c)).astype(np.float32)
        t[3, 5:9, 0] = [np.nan, np.inf, -np.inf, np.nan]
        t[7, 2, c - 1] = np.nan
        t[10:12, 10:20] = f[10:12, 10:20]   # exact ties: sign(0) = 0
        return f, t
    f[5, 5, :] = 0.0
    f[5, 5, 0] = 80.0
    f[5, 6, :] = -80.0
    f[5, 7, :] = 80.0
    f[5, 8, 0], f[5, 8, c - 1] = -80.0, 80.0
    lab = rng.integers(0, c, (h, w)).astype(np.uint8)
    lab[0, 0:4] = [255, c, min(c + 7, 254), 255]
    lab[5, 5:9] = [c - 1, 0, c - 1, 0]
    return f, lab


@pytest.mark.parametrize("c", [1, 3, 19])
@pytest.mark.parametrize("kind", ["l1", "cross_entropy"])
def test_losses_against_the_restatement(dev, kind, c):
    import brush_amd as ba
    h, w = LOSS_HW
    f, t = _loss_inputs(c, kind)
    weight = float(np.float32(0.7))   # (the entry takes an f32: the restatement gets the same number)
    fd, td = torch.from_numpy(f).to(dev), torch.from_numpy(t).to(dev)
    loss, v = ba.feature_loss_value_and_grad(fd, td, kind, weight)
    loss2, v2 = ba.feature_loss_value_and_grad(fd, td, kind, weight)
    only, none = ba.feature_loss_value_and_grad(fd, td, kind, weight, want_grad=False)
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2) and torch.equal(v, v2) and torch.equal(loss, only) and none is None, "two calls give the same bits"
    loss, v = loss.cpu().numpy(), v.cpu().numpy()
    if kind == "l1":
        want, count, vr = feature_ref.l1_loss(f, t, weight)
        cw = np.float32(weight / (h * w * c))
        assert 0 < count < h * w and loss[1] == count
        assert np.array_equal(v.view(np.int32), (cw * np.sign(vr).astype(np.float32)).astype(np.float32).view(np.int32))
        assert not v[10:12, 10:20].any() and not np.signbit(v[~np.isfinite(t).all(-1)]).any()
        bound = 3 * EPS * abs(want)
    else:
        want, count, vr = feature_ref.cross_entropy_loss(f, t, weight)
        cw = weight / (h * w)
        assert 0 < count < h * w and loss[1] == count
        assert np.isfinite(v).all() and not v[t >= c].any() and not np.signbit(v[t >= c]).any()
        slack = cw * (c + 8) * 2.0 ** -52
        d = np.abs(v.astype(np.float64) - vr)
        lim = 3 * EPS * (1 + 2 * EPS) * np.abs(vr) + slack + 2.0 ** -126   # ((1 + eps)^3 - 1 <= 3 eps (1 + 2 eps): three roundings compounded)
        print("cross-entropy C=%d: worst |dv| / bound = %.3f" % (c, float((d / lim).max())))
        assert (d <= lim).all(), float((d / lim).max())
        bound = 3 * EPS * abs(want) + count * slack * (1.0 + 2.0 * float(np.abs(f).max()))
    print("%s C=%d: loss %.9g, restatement %.9g, |d| / bound = %.3f" % (kind, c, loss[0], want, abs(float(loss[0]) - want) / bound))
    assert abs(float(loss[0]) - want) <= bound
    # weight <= 0 or NaN: all +0, the count too
    for wgt in (0.0, -1.0, float("nan")):
        l0, v0 = ba.feature_loss_value_and_grad(fd, td, kind, wgt)
        assert not l0.cpu().numpy().view(np.int32).any() and not v0.cpu().numpy().view(np.int32).any()


# ---- 7. edges ------------------------------------------------------------------------------------------------------------------------
def test_a_frame_that_lists_nothing_and_unlisted_splats(dev):
    import brush_amd as ba
    n, w, h, c = 3000, 123, 82, 9
    sc, cp = _scene(n, w, h, 0xD2)
    tr = sc["transforms"].copy()
    tr[-50:, 2] = -tr[-50:, 2]   # behind the camera: never listed
    spl = ba.Splats(tr, sc["sh"], sc["raw_opac"], device=dev)
    f = torch.randn((n, c), generator=torch.Generator().manual_seed(5)).to(dev)
    v = torch.randn((h, w, c), generator=torch.Generator().manual_seed(6)).to(dev) / (h * w)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), ctx=ctx)
        _, gid = _listed(node)
        unlisted = torch.ones(n, dtype=torch.bool, device=dev)
        unlisted[gid] = False
        assert bool(unlisted[-50:].all()) and int((~unlisted).sum()) > 100
        g = node.backward(None, v_features=v, features=f)
        vf = g["v_features"]
        assert float(vf[~unlisted].abs().max()) > 0.0
        assert not bool(vf[unlisted].view(torch.int32).any()), "rows of unlisted splats are +0"
        # a camera that looks away: nothing is listed
        away = dict(cp)
        away["rot_xyzw"] = util.quat_from_axis_angle((0.0, 1.0, 0.0), math.pi)
        empty = ba.render_splats_diff(spl, util.hip_camera(ba, away), (w, h), ctx=ctx)
        if empty.out.num_intersections:   # (the 50 flipped splats are in front of this camera: drop them)
            spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
            empty = ba.render_splats_diff(spl, util.hip_camera(ba, away), (w, h), ctx=ctx)
        assert empty.out.num_intersections == 0
        out = torch.full((h, w, c), -7.0, device=dev)
        ba.render_features(empty, f, out=out)
        assert not bool(out.view(torch.int32).any())
        g = empty.backward(None, v_features=v, features=f)
        for k in ("v_features", "v_transforms", "v_raw_opacities"):
            assert not bool(g[k].view(torch.int32).any()), k
    finally:
        ctx.close()


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
        f = torch.zeros((4, 3), device=dev)
        big = torch.zeros((4, 257), device=dev)
        m = torch.zeros((32, 32, 257), device=dev)
        p = C.c_void_p(m.data_ptr())
        err = lambda: ctx.lib.bh_last_error(ctx._h)
        # null arguments, C = 0, C = 257: BH_ERR_INVALID_ARG
        assert ctx.lib.bh_render_features(ctx._h, C.byref(node.out), None, 3, p) == -1 and b"null" in err()
        assert ctx.lib.bh_render_features(ctx._h, C.byref(node.out), p, 3, None) == -1 and b"null" in err()
        assert ctx.lib.bh_render_features(ctx._h, None, p, 3, p) == -1 and b"null" in err()
        assert ctx.lib.bh_render_features(ctx._h, C.byref(node.out), p, 0, p) == -1 and b"channels" in err()
        assert ctx.lib.bh_render_features(ctx._h, C.byref(node.out), p, 257, p) == -1 and b"channels" in err()
        tail = [p] * 8
        assert ctx.lib.bh_render_backward_features_saved(ctx._h, C.byref(node.out), None, p, 3, None, *tail) == -1 and b"null" in err()
        assert ctx.lib.bh_render_backward_features_saved(ctx._h, C.byref(node.out), None, None, 3, p, *tail) == -1 and b"null" in err()
        assert ctx.lib.bh_render_backward_features_saved(ctx._h, C.byref(node.out), None, p, 3, p, *([p] * 7), None) == -1 and b"null" in err()
        assert ctx.lib.bh_render_backward_features_saved(ctx._h, C.byref(node.out), None, p, 0, p, *tail) == -1 and b"channels" in err()
        assert ctx.lib.bh_render_backward_features_saved(ctx._h, C.byref(node.out), None, p, 257, p, *tail) == -1 and b"channels" in err()
        with pytest.raises(ba.BrushHipError, match="channels"):
            node.features(big)
        with pytest.raises(ba.BrushHipError, match="features must be"):
            node.features(torch.zeros((5, 3), device=dev))
        with pytest.raises(ba.BrushHipError, match="out"):
            ba.render_features(node, f, out=torch.zeros((32, 32, 4), device=dev))
        with pytest.raises(ba.BrushHipError, match="does not combine"):
            node.backward(None, v_depth=torch.zeros((32, 32), device=dev), v_features=m[..., :3].contiguous(), features=f)
        with pytest.raises(ba.BrushHipError, match="does not combine"):
            node.backward(torch.zeros((32, 32, 4), device=dev), pose=True, v_features=m[..., :3].contiguous(), features=f)
        with pytest.raises(ba.BrushHipError, match="go together"):
            node.backward(None, features=f)
        # the loss: null, zero size, C = 0 / 257, unknown kind
        t = ba._ffi.BhFeatureTarget()
        t.target, t.h, t.w, t.channels, t.kind, t.weight = m.data_ptr(), 32, 32, 3, 0, 1.0
        assert ctx.lib.bh_feature_loss_value_and_grad(ctx._h, None, C.byref(t), p, p) == -1 and b"null" in err()
        for field, bad, text in (("channels", 0, b"channels"), ("channels", 257, b"channels"), ("kind", 2, b"kind"), ("h", 0, b"zero size")):
            keep = getattr(t, field)
            setattr(t, field, bad)
            assert ctx.lib.bh_feature_loss_value_and_grad(ctx._h, p, C.byref(t), p, p) == -1 and text in err(), field
            setattr(t, field, keep)
        # a forward-only frame: BH_ERR_INVALID_ARG, as the depth entries'
        _, out, folded = host._forward(ctx, spl, cam, (32, 32), (0, 0, 0), ba.RasterPass.Forward)
        assert ctx.lib.bh_render_features(ctx._h, C.byref(out), p, 3, p) == -1 and b"BWD_INFO" in err()
        assert ctx.lib.bh_render_backward_features_saved(ctx._h, C.byref(out), None, p, 3, p, *tail) == -1 and b"BWD_INFO" in err()
        # a stale BhRenderOut: another forward has run since (BH_ERR_STATE)
        assert ctx.lib.bh_render_features(ctx._h, C.byref(node.out), p, 3, p) == -4 and b"stale" in err()
        with pytest.raises(ba.BrushHipError, match="stale"):
            node.features(f)
        with pytest.raises(ba.BrushHipError, match="stale"):
            node.backward(None, v_features=m[..., :3].contiguous(), features=f)
    finally:
        ctx.close()


def test_interleaved_feature_renders_do_not_change_training(dev):
    """The one-tile deterministic set-up of tests/test_gpu_depth.py::test_interleaved_depth_renders_do_not_change_training (16x16,
    6000 splats, seed 77, 9 steps), with, after every step, the feature map of the step's own forward (bh_last_render_out) and of a
    larger frame at another camera, a feature backward of that frame and a loss: parameters, moments and refine statistics equal a
    run without, bit for bit."""
    import ctypes as C
    import brush_amd as ba
    from brush_amd import _ffi
    n, w, h, c = 6000, 16, 16, 5
    sc = synth.make_scene(n, 0xD0A, sh_degree=1, log_scale_range=(math.log(0.05), math.log(0.4)),
                          tan_half_fov=(math.tan(math.radians(50)), math.tan(math.radians(50))))
    cams = []
    for i in range(3):
        cc = dict(synth.default_camera_params(w, h))
        cc["rot_xyzw"] = util.quat_from_axis_angle((0, 1, 0), math.radians(-35 + 35 * i))
        cams.append(cc)
    gt = torch.from_numpy(synth.synthetic_gt_packed(w, h).view(np.int32)).to(dev)
    ew, eh = 200, 136
    other = util.hip_camera(ba, synth.default_camera_params(ew, eh))
    f = torch.randn((n, c), generator=torch.Generator().manual_seed(9)).to(dev)
    labels = torch.randint(0, c, (eh, ew), generator=torch.Generator().manual_seed(10)).to(torch.uint8).to(dev)
    runs = {}
    for key in ("plain", "with_features"):
        ctx = ba.Context(dev)
        try:
            spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
            tr = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=3.0, ctx=ctx, seed=77)
            for s in range(9):
                tr.step(ba.SceneBatch(gt, util.hip_camera(ba, cams[s % len(cams)])), spl)
                if key == "with_features":
                    last = _ffi.BhRenderOut()
                    ctx.check(ctx.lib.bh_last_render_out(ctx._h, C.byref(last)))
                    own = torch.zeros((h, w, c), device=dev)
                    ctx.check(ctx.lib.bh_render_features(ctx._h, C.byref(last), C.c_void_p(f.data_ptr()), c, C.c_void_p(own.data_ptr())))
                    assert bool(torch.isfinite(own).all())
                    node = ba.render_splats_diff(spl, other, (ew, eh), ctx=ctx)
                    m = node.features(f)
                    assert float(m.abs().max()) > 0.0
                    _, v = ba.feature_loss_value_and_grad(m, labels, "cross_entropy", ctx=ctx)
                    g = node.backward(None, v_features=v, features=f)
                    assert bool(torch.isfinite(g["v_transforms"]).all()) and bool(torch.isfinite(g["v_features"]).all())
            ctx.sync()
            out = {"transforms": spl.transforms.clone(), "sh": spl.sh_coeffs.clone(), "opac": spl.raw_opacities.clone()}
            out.update({k: v.clone() for k, v in tr.state.items()})
            runs[key] = out
        finally:
            ctx.close()
    a, b = runs["plain"], runs["with_features"]
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
