"""Distortion maps on the GPU (include/brush_hip_distortion.h): both kinds against the float64 restatement
tests/distortion_ref.py, the slab case that unshifted float32 sums miss, bit identity across list policies / calls / retained forwards
/ tile-row windows, the empty frame, gradients against autograd (the term alone, with colour, with colour + expected depth +
accumulated normals), the loss operator and the refusals.

Reference case (tests/test_gpu_depth.py's: 300 splats, 64 x 48, seed 0xE5): outside depth_ref.tie_mask, at most 15 of 3072 pixels
skipped (the count is asserted before anything is compared).  Slab case: 300 splats, seed 0x53, z in [50, 52], scales 1.0 to 6.0,
default camera: about 23 terms per pixel, depth 25 times the spread; the naive float32 sums A M2 - M1^2 evaluated in numpy on the
reference's own weights must miss TOL by at least ten times before the kernel's map is held to TOL.

Tolerances: TOL = 1e-4 of the map's maximum and GRAD_TOL = 1e-4 of each gradient block's largest entry, the project's figures.
BH_DISTORTION_NDC is tested with near / far that bracket the case's depths (0.5 / 20, slab 10 / 100).

Measured on an MI355X: the 16 reference maps within 1.4e-6 to 2.1e-6 of their maximum and the slab's within 8.3e-7 (z) and 1.8e-6
(ndc), where the naive sums miss by 5.2e-3; 0 to 8 tie pixels; gradients at most 1.1e-5 of a block's largest entry on the reference
cases, 1.6e-5 on the slab with all four terms, 2.9e-6 on the big frame.  No case is left out."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import depth_ref
import distortion_ref
import util

pytestmark = pytest.mark.gpu
TOL = 1e-4        # of the map's maximum
GRAD_TOL = 1e-4   # of each block's largest entry
MAX_SKIPPED = 15  # of 3072 pixels
KINDS = ("z", "ndc")
REF_CASES = [("pinhole", False), ("pinhole", True), ("kb4", False), ("kb4", True)]
NDC = {"ref": (0.5, 20.0), "slab": (10.0, 100.0), "big": (0.5, 20.0)}


def _params(cases):
    """Every case with the hard cut-off, then with the smooth one ('-smooth')."""
    ids = ["-".join(str(x) for x in c) for c in cases]
    return [pytest.param(*c, False, id=i) for c, i in zip(cases, ids)] + [pytest.param(*c, True, id=i + "-smooth") for c, i in zip(cases, ids)]


def _scene(n, w, h, seed, z_range=(2.0, 12.0), scales=(0.03, 0.3), sh_degree=0):
    cp = synth.default_camera_params(w, h)
    tans = (math.tan(cp["fov_x"] / 2.0), math.tan(cp["fov_y"] / 2.0))
    return synth.make_scene(n, seed, sh_degree=sh_degree, log_scale_range=(math.log(scales[0]), math.log(scales[1])), z_range=z_range, tan_half_fov=tans), cp


def _strip(cp):
    return {k: v for k, v in cp.items() if k not in ("img_w", "img_h")}


def _ref_case(model):
    w, h = 64, 48
    sc, cp = _scene(300, w, h, 0xE5, z_range=(2.0, 9.0), scales=(0.05, 0.4))
    cp = _strip(cp)
    cp["pos"] = (0.15, -0.1, -0.4)
    cp["rot_xyzw"] = util.quat_from_axis_angle((0.3, 1.0, 0.1), 0.08)
    if model != "pinhole":
        cp["model"], cp["dist"] = util.REF_LENSES[model]
    return sc, cp, w, h


def _slab_case():
    w, h = 64, 48
    sc, cp = _scene(300, w, h, 0x53, z_range=(50.0, 52.0), scales=(1.0, 6.0))
    return sc, _strip(cp), w, h


def _big_case():
    w, h = 123, 82
    sc, cp = _scene(3000, w, h, 0xD2)
    return sc, _strip(cp), w, h


BIG_WINDOW = (96, 60, 123, 82)   # the ragged corner of the big frame: its last tile column (11 pixels) and tile row (2 pixels)


def _case(which, model="pinhole"):
    return _ref_case(model) if which == "ref" else (_slab_case() if which == "slab" else _big_case())


def _pass(ba, smooth):
    return ba.RasterPass.BackwardSmoothCutoff if smooth else ba.RasterPass.Backward


@functools.lru_cache(maxsize=None)
def _ref_render(which, model, mip, smooth, kind):
    """The float64 reference of a case, computed once and shared (read-only)."""
    sc, cp, w, h = _case(which, model)
    near, far = NDC[which]
    tr, sh, op = [torch.tensor(np.asarray(sc[k], np.float64), requires_grad=True) for k in ("transforms", "sh", "raw_opac")]
    with torch.enable_grad():
        out = distortion_ref.render(tr, sh, op, cp, w, h, intrinsics=distortion_ref.intrinsics(cp, w, h), mip=mip, smooth=smooth, kind=kind, near=near,
                                    far=far, keep_terms=which == "slab")
    return {k: (tuple(x.detach() for x in v) if isinstance(v, tuple) else (v.detach() if torch.is_tensor(v) else v)) for k, v in out.items()}


def _compare_map(tag, got, ref):
    want = ref["dist"].numpy()
    skip = depth_ref.tie_mask(ref, "accumulated").numpy()
    print("%s: %d tie pixels, %d uncovered, at most %d terms, mean %.1f" % (tag, int(skip.sum()), int((ref["n_terms"] == 0).sum()), int(ref["n_terms"].max()),
                                                                        float(ref["n_terms"].double().mean())))
    assert int(skip.sum()) <= MAX_SKIPPED, (tag, int(skip.sum()))
    top = float(want.max())
    assert top > 0.0
    err = float(np.abs(got.astype(np.float64) - want)[~skip].max())
    print("%s: max err / map max = %.3e (map max %.4e)" % (tag, err / top, top))
    assert err <= TOL * top, (tag, err / top)


# ---- 1. the maps against the float64 reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("model,mip,smooth", _params(REF_CASES))
def test_distortion_maps_match_the_float64_reference(dev, model, mip, smooth, kind):
    import brush_amd as ba
    sc, cp, w, h = _ref_case(model)
    near, far = NDC["ref"]
    ref = _ref_render("ref", model, mip, smooth, kind)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], render_mip=mip, device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), pass_=_pass(ba, smooth), ctx=ctx)
        assert float(np.abs(node.img.cpu().numpy() - ref["img"].numpy()).max()) <= 1e-5
        got = node.distortion(kind, near, far)
        _compare_map("%s mip=%d smooth=%d %s" % (model, mip, smooth, kind), got.cpu().numpy(), ref)
        # the moment map restates the value map: A is the image's alpha, dist = fma(A, M2', -(M1' M1')), bit for bit
        mo = ba.render_distortion(node, kind, near, far, moments=True)
        assert torch.equal(mo[..., 0], node.img[..., 3])
        d = (mo[..., 0].double() * mo[..., 2].double() - mo[..., 1].double() * mo[..., 1].double())
        assert float((d - got.double()).abs().max()) <= 4 * 2.0 ** -24 * float((mo[..., 0] * mo[..., 2]).abs().max()) + 1e-30
        assert bool((mo[..., 2] >= 0).all())
    finally:
        ctx.close()


# ---- 2. the slab: depth 25 times the spread ----------------------------------------------------------------------------------------
def _naive_f32(weights, m):
    """A M2 - M1^2 from unshifted float32 sums, folded in the blend's order with one fma per term: what a kernel without the per-pixel
    reference computes (the weights are the float64 reference's, rounded once)."""
    f = np.float32
    a = np.zeros(weights.shape[1:], f)
    m1, m2 = a.copy(), a.copy()
    for i in range(weights.shape[0]):
        wi, mi = weights[i].astype(f), f(m[i])
        a = a + wi
        m1 = (wi.astype(np.float64) * np.float64(mi) + m1).astype(f)          # (an fma: one rounding)
        m2 = (wi.astype(np.float64) * np.float64(mi) * np.float64(mi) + m2).astype(f)
    return (a.astype(np.float64) * m2 - m1.astype(np.float64) * m1).astype(f)


@pytest.mark.parametrize("kind", KINDS)
def test_slab_case_needs_the_shifted_sums_and_the_kernel_has_them(dev, kind):
    import brush_amd as ba
    sc, cp, w, h = _slab_case()
    near, far = NDC["slab"]
    ref = _ref_render("slab", "pinhole", False, False, kind)
    want = ref["dist"].numpy()
    top = float(want.max())
    assert int((ref["n_terms"] == 0).sum()) == 0 and float(ref["n_terms"].double().mean()) > 15.0
    if kind == "z":   # teeth: the unshifted float32 sums miss TOL by at least ten times on this case
        weights, m = ref["terms"]
        naive = _naive_f32(weights.numpy(), m.numpy())
        naive_err = float(np.abs(naive.astype(np.float64) - want).max()) / top
        print("slab: naive float32 sums miss by %.3e of the map's maximum" % naive_err)
        assert naive_err >= 10 * TOL, naive_err
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), ctx=ctx)
        _compare_map("slab %s" % kind, node.distortion(kind, near, far).cpu().numpy(), ref)
    finally:
        ctx.close()


# ---- 3. bit identity ---------------------------------------------------------------------------------------------------------------
def test_distortion_does_not_depend_on_the_list_policy_or_the_call(dev):
    import brush_amd as ba
    n, w, h = 60000, 320, 208
    sc, cp = _scene(n, w, h, 0x56)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    cam = util.hip_camera(ba, cp)
    args = {"z": ("z", 0.2, 1000.0), "ndc": ("ndc", 0.5, 30.0)}
    ctx = ba.Context(dev)
    try:
        base = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx)
        want = {k: base.distortion(*args[k]).clone() for k in KINDS}
        want_mo = ba.render_distortion(base, "z", moments=True).clone()
        for k in KINDS:
            assert torch.equal(base.distortion(*args[k]), want[k]), "two calls on one saved state"
            assert float(want[k].max()) > 0.0
        assert torch.equal(ba.render_distortion(base, "z", moments=True), want_mo)
        img = base.img.clone()
        # per-tile cut lists: the second sliced frame of a view
        ba.set_view_id(0xD0, ctx)
        first = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
        assert first.out.tile_offsets_far is None or first.out.list_budget == first.out.num_intersections
        cut = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
        assert cut.out.tile_offsets_far and cut.out.num_listed_splats < cut.out.num_visible, "not a cut frame"
        assert torch.equal(cut.img, img)
        for k in KINDS:
            assert torch.equal(cut.distortion(*args[k]), want[k]), ("cut lists", k)
        # a near + far frame with a fixed near share
        ba.set_view_id(0, ctx)
        ba.host.set_list_slicing(0.5, ctx)
        try:
            half = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
            assert half.out.tile_offsets_far
            assert torch.equal(half.img, img)
            for k in KINDS:
                assert torch.equal(half.distortion(*args[k]), want[k]), ("near + far", k)
            assert torch.equal(ba.render_distortion(half, "z", moments=True), want_mo)
        finally:
            ba.host.set_list_slicing(0.0, ctx)
        # a retained forward, after another forward has run
        kept = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, retain=True)
        other = dict(cp)
        other["pos"] = (1.0, -0.2, -1.0)
        ba.render_splats(spl, util.hip_camera(ba, other), (w, h), (0, 0, 0), ba.RasterPass.Backward, ctx=ctx, copy=False)
        for k in KINDS:
            assert torch.equal(kept.distortion(*args[k]), want[k]), ("retained", k)
        kept.release()
        # two tile-row windows stitched into a pre-filled tensor
        rows = (h + 15) // 16
        for k in KINDS:
            out = torch.full((h, w), -7.0, device=dev)
            for win in ((0, 5), (5, rows)):
                part = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, tile_rows=win)
                ba.render_distortion(part, *args[k], out=out)
            assert torch.equal(out, want[k]), ("windows", k)
    finally:
        ctx.close()


# ---- 4. the empty frame ------------------------------------------------------------------------------------------------------------
def test_a_camera_facing_away_gives_a_zero_map_and_zero_gradients(dev):
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
        for k in KINDS:
            out = torch.full((h, w), 3.0, device=dev)
            ba.render_distortion(node, k, 0.5, 20.0, out=out)
            assert float(out.abs().max()) == 0.0
        mo = torch.full((h, w, 4), 3.0, device=dev)
        ba.render_distortion(node, "z", out=mo, moments=True)
        assert float(mo.abs().max()) == 0.0
        # a window of an empty frame clears its rows only
        part = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), ctx=ctx, tile_rows=(1, 2))
        out = torch.full((h, w), 3.0, device=dev)
        ba.render_distortion(part, "z", out=out)
        assert float(out[16:32].abs().max()) == 0.0 and bool((out[:16] == 3.0).all()) and bool((out[32:] == 3.0).all())
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), ctx=ctx)
        for kw in (dict(), dict(v_depth=torch.ones((h, w), device=dev)), dict(distortion="ndc", distortion_near=0.5, distortion_far=20.0)):
            g = node.backward(None, v_distortion=torch.ones((h, w), device=dev), **kw)
            for k in ("v_transforms", "v_sh_coeffs", "v_raw_opacities", "v_refine_weight"):
                assert float(g[k].abs().max()) == 0.0, k
    finally:
        ctx.close()


# ---- 5. gradients ------------------------------------------------------------------------------------------------------------------
def _assert_close(name, a, b, tol=GRAD_TOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.isfinite(a).all(), name
    rel = util.rel_linf(a, b)
    print("%s: rel linf %.3e (block max %.3e)" % (name, rel, float(np.abs(b).max())))
    assert rel <= tol, (name, rel)


def _assert_grads(tag, g, tr, op, sh=None):
    vt = g["v_transforms"].cpu().numpy()
    for nm, sl in (("means", slice(0, 3)), ("quats", slice(3, 7)), ("log_scales", slice(7, 10))):
        _assert_close("%s %s" % (tag, nm), vt[:, sl], tr[:, sl])
    _assert_close("%s raw_opac" % tag, g["v_raw_opacities"].cpu().numpy(), op)
    if sh is not None:
        _assert_close("%s sh" % tag, g["v_sh_coeffs"].cpu().numpy(), sh)


def _cotangents(which, h, w, terms, seed=37):
    """v_distortion, and for terms > 1 v_output, for terms > 2 v_depth and v_normal: uniform in [-1, 1] / (H W).  On the big frame they
    are zero outside BIG_WINDOW (the float64 reference is evaluated on the window alone)."""
    rng = np.random.default_rng(seed)
    x0, y0, x1, y1 = BIG_WINDOW if which == "big" else (0, 0, w, h)

    def draw(*tail):
        full = np.zeros((h, w) + tail, np.float32)
        full[y0:y1, x0:x1] = (rng.uniform(-1.0, 1.0, (y1 - y0, x1 - x0) + tail) / (h * w)).astype(np.float32)
        return full
    v = dict(v_distortion=draw())
    if terms > 1:
        v["v_output"] = draw(4)
    if terms > 2:
        v["v_depth"] = draw()
        v["v_normal"] = draw(3)
    return v


def _check_gradients(dev, which, model, mip, smooth, kind, terms):
    import brush_amd as ba
    sc, cp, w, h = _case(which, model)
    near, far = NDC[which]
    v = _cotangents(which, h, w, terms)
    window = BIG_WINDOW if which == "big" else None
    x0, y0, x1, y1 = window or (0, 0, w, h)
    cut = {k: x[y0:y1, x0:x1] for k, x in v.items()}
    ref, g_tr, g_sh, g_op = distortion_ref.gradients(sc, cp, w, h, cut["v_distortion"], kind, near, far, v_output=cut.get("v_output"), v_depth=cut.get("v_depth"),
                                                     depth_mode="expected", v_normal=cut.get("v_normal"), intrinsics=distortion_ref.intrinsics(cp, w, h),
                                                     mip=mip, smooth=smooth, window=window)
    assert float(np.abs(g_tr[:, :3]).max()) > 0.0 and float(np.abs(g_op).max()) > 0.0
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], render_mip=mip, device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), pass_=_pass(ba, smooth), ctx=ctx)
        if which == "big":
            from brush_amd import host
            to = host._view(node.out.tile_offsets, (node.out.num_tiles, 2), torch.int32, dev).cpu().numpy().astype(np.int64)
            assert int((to[:, 1] - to[:, 0]).max()) > 64, "no list longer than one batch"
        t = {k: torch.from_numpy(x).to(dev) for k, x in v.items()}
        g = node.backward(t.get("v_output"), v_depth=t.get("v_depth"), depth_mode="expected", v_normal=t.get("v_normal"), normal_mode="accumulated",
                          v_distortion=t["v_distortion"], distortion=kind, distortion_near=near, distortion_far=far)
        _assert_grads("%s %s mip=%d smooth=%d %s terms=%d" % (which, model, mip, smooth, kind, terms), g, g_tr, g_op, g_sh if terms > 1 else None)
        if terms == 1:
            assert float(g["v_sh_coeffs"].abs().max()) == 0.0 and float(g["v_refine_weight"].abs().max()) == 0.0
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("model,mip,smooth", _params(REF_CASES))
def test_distortion_gradients_match_autograd(dev, model, mip, smooth, kind):
    _check_gradients(dev, "ref", model, mip, smooth, kind, terms=1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("terms", [2, 3], ids=["colour", "colour-depth-normal"])
def test_one_backward_carries_the_distortion_term_with_the_others(dev, terms, kind):
    _check_gradients(dev, "ref", "pinhole", False, False, kind, terms)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("terms", [1, 3], ids=["alone", "colour-depth-normal"])
def test_slab_gradients_match_autograd(dev, terms, kind):
    _check_gradients(dev, "slab", "pinhole", False, False, kind, terms)


@pytest.mark.parametrize("kind,terms", [("z", 1), ("ndc", 3)], ids=["z-alone", "ndc-colour-depth-normal"])
def test_big_frame_gradients_match_autograd(dev, kind, terms):
    """123 x 82 with 3000 splats: a ragged tile edge and lists longer than one batch of 64; cotangents on the ragged corner."""
    _check_gradients(dev, "big", "pinhole", False, False, kind, terms)


# ---- 6. the loss operator ----------------------------------------------------------------------------------------------------------
def test_distortion_loss_is_the_float64_mean_and_repeats_bit_for_bit(dev):
    import brush_amd as ba
    sc, cp, w, h = _ref_case("pinhole")
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), ctx=ctx)
        dist = node.distortion("z")
        mo = ba.render_distortion(node, "z", moments=True)
        weight = 0.37
        want = weight * float(dist.double().sum()) / (h * w)
        a = ba.distortion_loss(dist, weight, ctx=ctx)
        b = ba.distortion_loss(dist, weight, ctx=ctx)
        c = ba.distortion_loss(mo, weight, ctx=ctx)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), "the moment map's loss is the value map's"
        got = a.cpu().numpy()
        print("distortion loss %.8e against %.8e" % (got[0], want))
        # one rounding of c = weight / (H W), one of the product, one of the result
        assert abs(float(got[0]) - want) <= 3 * 2.0 ** -24 * abs(want) and want > 0.0
        assert float(got[1]) == float(h * w)
        # a frame wider than one pass of the capped grid (1024 blocks of 256 pixels), of a size that is no multiple of the block
        big = torch.rand((523, 1031), device=dev)
        wb = float(big.double().sum()) / big.numel()
        lb = ba.distortion_loss(big, 1.0, ctx=ctx)
        assert torch.equal(lb.view(torch.int32), ba.distortion_loss(big, 1.0, ctx=ctx).view(torch.int32))
        assert abs(float(lb[0]) - wb) <= 3 * 2.0 ** -24 * wb and float(lb[1]) == float(big.numel())
        # no term
        for wt in (0.0, -1.0, float("nan")):
            z = ba.distortion_loss(dist, wt, ctx=ctx)
            assert float(z.abs().max()) == 0.0
    finally:
        ctx.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    import brush_amd as ba
    from brush_amd import _ffi, host
    sc = util.base_scene()
    cam = util.hip_camera(ba, util.STD_CAM)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, cam, (32, 32), ctx=ctx)
        vd = torch.zeros((32, 32), device=dev)
        with pytest.raises(ba.BrushHipError, match="kind"):
            node.distortion(2)
        with pytest.raises(ba.BrushHipError, match="kind"):
            node.backward(None, v_distortion=vd, distortion=2)
        for near, far in ((0.0, 10.0), (-1.0, 10.0), (2.0, 2.0), (3.0, 1.0), (float("nan"), 10.0), (1.0, float("nan"))):
            with pytest.raises(ba.BrushHipError, match="near"):
                node.distortion("ndc", near, far)
            with pytest.raises(ba.BrushHipError, match="near"):
                node.backward(None, v_distortion=vd, distortion="ndc", distortion_near=near, distortion_far=far)
        with pytest.raises(ba.BrushHipError, match="median"):
            node.backward(None, v_depth=vd, depth_mode="median", v_distortion=vd)
        with pytest.raises(ba.BrushHipError, match="mode"):
            node.backward(None, v_normal=torch.zeros((32, 32, 3), device=dev), normal_mode=2, v_distortion=vd)
        with pytest.raises(ba.BrushHipError, match="pose"):
            node.backward(torch.zeros((32, 32, 4), device=dev), v_distortion=vd, pose=True)
        with pytest.raises(ba.BrushHipError, match="out"):
            ba.render_distortion(node, "z", out=torch.zeros((32, 31), device=dev))
        with pytest.raises(ba.BrushHipError, match="out"):
            ba.render_distortion(node, "z", out=torch.zeros((32, 32), device=dev), moments=True)
        with pytest.raises(ValueError):
            ba.distortion_loss(torch.zeros((32, 32, 3), device=dev), ctx=ctx)
        # null pointers, and a null ctx before the device is touched
        p = C.c_void_p(vd.data_ptr())
        cfg = _ffi.BhDistortionConfig(kind=0)
        lib = ctx.lib
        assert lib.bh_render_distortion(None, C.byref(node.out), C.byref(cfg), p) == -1
        assert lib.bh_render_distortion_moments(None, C.byref(node.out), C.byref(cfg), p) == -1
        assert lib.bh_render_backward_distortion_saved(None, C.byref(node.out), None, None, 0, None, 0, p, C.byref(cfg), p, p, p, p, p, p, p) == -1
        assert lib.bh_distortion_loss(None, p, 32, 32, 1, 1.0, p) == -1
        assert lib.bh_train_set_distortion(None, None) == -1
        assert lib.bh_render_distortion(ctx._h, None, C.byref(cfg), p) == -1
        assert lib.bh_render_distortion(ctx._h, C.byref(node.out), None, p) == -1
        assert lib.bh_render_distortion(ctx._h, C.byref(node.out), C.byref(cfg), None) == -1
        assert lib.bh_render_backward_distortion_saved(ctx._h, C.byref(node.out), None, None, 0, None, 0, None, C.byref(cfg), p, p, p, p, p, p, p) == -1
        assert lib.bh_render_backward_distortion_saved(ctx._h, C.byref(node.out), None, None, 0, None, 0, p, None, p, p, p, p, p, p, p) == -1
        assert lib.bh_distortion_loss(ctx._h, None, 32, 32, 1, 1.0, p) == -1
        assert lib.bh_distortion_loss(ctx._h, p, 32, 32, 1, 1.0, None) == -1
        assert b"null" in lib.bh_last_error(ctx._h)
        assert lib.bh_distortion_loss(ctx._h, p, 0, 32, 1, 1.0, p) == -1
        assert lib.bh_distortion_loss(ctx._h, p, 32, 32, 3, 1.0, p) == -1 and b"channels" in lib.bh_last_error(ctx._h)
        # the train term: an unknown kind or bad near / far with a weight > 0 is refused; without a weight nothing is looked at
        assert lib.bh_train_set_distortion(ctx._h, C.byref(_ffi.BhDistortionTermConfig(weight=1.0, kind=2))) == -1 and b"kind" in lib.bh_last_error(ctx._h)
        assert lib.bh_train_set_distortion(ctx._h, C.byref(_ffi.BhDistortionTermConfig(weight=1.0, kind=1, near_z=2.0, far_z=1.0))) == -1
        assert lib.bh_train_set_distortion(ctx._h, C.byref(_ffi.BhDistortionTermConfig(weight=0.0, kind=2))) == 0
        assert lib.bh_train_set_distortion(ctx._h, C.byref(_ffi.BhDistortionTermConfig(weight=float("nan"), kind=2))) == 0
        assert lib.bh_train_set_distortion(ctx._h, None) == 0
        # a forward-only frame
        _, out, folded = host._forward(ctx, spl, cam, (32, 32), (0, 0, 0), ba.RasterPass.Forward)
        rc = lib.bh_render_distortion(ctx._h, C.byref(out), C.byref(cfg), p)
        assert rc == -1 and b"BWD_INFO" in lib.bh_last_error(ctx._h)
        rc = lib.bh_render_backward_distortion_saved(ctx._h, C.byref(out), None, None, 0, None, 0, p, C.byref(cfg), p, p, p, p, p, p, p)   # (refused before any pointer is read)
        assert rc == -1 and b"BWD_INFO" in lib.bh_last_error(ctx._h)
        # a stale BhRenderOut: another forward has run since
        with pytest.raises(ba.BrushHipError, match="stale"):
            node.distortion("z")
        with pytest.raises(ba.BrushHipError, match="stale"):
            node.backward(None, v_distortion=vd)
    finally:
        ctx.close()
