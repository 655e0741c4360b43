"""The fused normal-consistency operator on the GPU (include/brush_hip_normal_loss.h) against the float64 restatement
tests/normal_loss_ref.py: on the real accumulated normals, expected depth and image of tests/test_gpu_depth.py's reference case (300
splats, 64 x 48, pinhole, Mip off and on) and on crafted maps (67 x 5; 3 x 3 with one valid pixel; 2 x 7 with none; a depth map with a
NaN, a 0 and a negative pixel).  The valid count is the reference's exactly (validity does not depend on rounding).

Bounds, the project's own: |du| <= 16 * 2^-24 * max(fx, fy) per component is §6m's depth -> normal bound (tests/test_gpu_normal.py), so
|dv_normal| <= c * that (v_normal = -c A u, A <= 1) and |dloss[0]| <= weight * that; v_depth within 1e-4 of its largest entry (README,
"Correctness").  Accumulate is the map plus the overwrite result to the bit, two calls give the same bits, weight 0 / NaN give +0.

Measured on an MI355X (the maxima over all cases, as fractions of their bounds): see DESIGN.md §6n."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import normal_loss_ref as nl
import normal_ref
import util

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
GRAD_TOL = 1e-4


def _ref_case():
    """tests/test_gpu_normal.py::_ref_case("pinhole")."""
    w, h = 64, 48
    cp = synth.default_camera_params(w, h)
    tans = (math.tan(cp["fov_x"] / 2.0), math.tan(cp["fov_y"] / 2.0))
    sc = synth.make_scene(300, 0xE5, sh_degree=0, log_scale_range=(math.log(0.05), math.log(0.4)), z_range=(2.0, 9.0), tan_half_fov=tans)
    cp = {k: v for k, v in cp.items() if k not in ("img_w", "img_h")}
    cp["pos"] = (0.15, -0.1, -0.4)
    cp["rot_xyzw"] = util.quat_from_axis_angle((0.3, 1.0, 0.1), 0.08)
    return sc, cp, w, h


def _crafted(name):
    """-> (normal [h,w,3], depth [h,w], image [h,w,4]) f32 numpy, camera params."""
    w, h = {"67x5": (67, 5), "3x3": (3, 3), "2x7": (7, 2), "holes": (23, 17)}[name]
    rng = np.random.default_rng(0x6E + w)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    depth = (3.0 + 0.04 * xs - 0.06 * ys + rng.uniform(-0.03, 0.03, (h, w))).astype(np.float32)
    if name == "holes":
        depth[4, 6], depth[9, 15], depth[12, 3] = np.nan, 0.0, -1.5
    normal = rng.uniform(-0.6, 0.6, (h, w, 3)).astype(np.float32)
    image = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float32)
    cp = {k: v for k, v in synth.default_camera_params(w, h).items() if k not in ("img_w", "img_h")}
    return (normal, depth, image), cp, w, h


@functools.lru_cache(maxsize=None)
def _reference(key, weight):
    """The float64 reference of a case's f32 maps, computed once and shared (read-only).  key: ("real", mip) or ("crafted", name)."""
    maps, cp, w, h = _maps(key)
    intr = normal_ref.intrinsics(cp, w, h)
    return nl.value_and_grad(maps[0], maps[1], maps[2][..., 3], intr["fx"], intr["fy"], intr["cx"], intr["cy"], weight), intr


@functools.lru_cache(maxsize=None)
def _maps(key):
    if key[0] == "crafted":
        return _crafted(key[1])
    import brush_amd as ba
    sc, cp, w, h = _ref_case()
    dev = torch.device("cuda:0")
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], render_mip=key[1], device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), ctx=ctx)
        maps = (node.normal("accumulated").cpu().numpy(), node.depth("expected").cpu().numpy(), node.img.cpu().numpy().copy())
    finally:
        ctx.close()
    return maps, cp, w, h


def _run(ba, ctx, dev, maps, cp, weight, v_depth=None):
    n, d, i = [torch.from_numpy(np.ascontiguousarray(m)).to(dev) for m in maps]
    loss, vn, vd = ba.normal_consistency_value_and_grad(n, d, i, util.hip_camera(ba, cp), weight, v_depth=v_depth, ctx=ctx)
    ctx.sync()
    return loss.cpu().numpy(), vn.cpu().numpy(), vd.cpu().numpy()


CASES = [("real", False), ("real", True), ("crafted", "67x5"), ("crafted", "3x3"), ("crafted", "2x7"), ("crafted", "holes")]


@pytest.mark.parametrize("key", CASES, ids=lambda k: "%s-%s" % k)
def test_operator_matches_the_float64_reference(dev, key):
    import brush_amd as ba
    weight = 0.7
    maps, cp, w, h = _maps(key)
    ref, intr = _reference(key, weight)
    c = nl.constant(weight, w * h)
    bound_u = 16 * EPS * max(intr["fx"], intr["fy"])
    ctx = ba.Context(dev)
    try:
        loss, vn, vd = _run(ba, ctx, dev, maps, cp, weight)
        assert np.isfinite(loss).all() and np.isfinite(vn).all() and np.isfinite(vd).all()
        assert loss[1] == ref["count"], (loss[1], ref["count"])
        assert not vn[~ref["valid"]].any()   # an invalid pixel is exactly 0
        err_n = float(np.abs(vn.astype(np.float64) - ref["v_normal"]).max())
        err_l = abs(float(loss[0]) - ref["loss"])
        big = float(np.abs(ref["v_depth"]).max())
        err_d = float(np.abs(vd.astype(np.float64) - ref["v_depth"]).max())
        print("%s-%s: %d valid of %d; |dv_normal| %.3e (bound %.3e), |dloss| %.3e (bound %.3e), v_depth %.3e of its largest %.3e (bound %.0e)"
              % (key + (ref["count"], w * h, err_n, c * bound_u, err_l, weight * bound_u, err_d / big if big else 0.0, big, GRAD_TOL)))
        assert err_n <= c * bound_u, (err_n, c * bound_u)
        assert err_l <= weight * bound_u, (err_l, weight * bound_u)
        assert err_d <= GRAD_TOL * big, (err_d, big)
        if key == ("crafted", "3x3"):
            assert ref["count"] == 1 and vn[1, 1].any() and np.count_nonzero(vd) == 4 and vd[1, 1] == 0.0
        elif key == ("crafted", "2x7"):
            # no valid pixel: loss, count and both gradients are exactly 0
            assert ref["count"] == 0
            for t in (loss, vn, vd):
                assert not t.view(np.int32).any()
        else:
            assert ref["count"] > 0.25 * w * h and big > 0 and loss[0] > 0
        if key == ("crafted", "holes"):
            for (y, x) in ((4, 6), (9, 15), (12, 3)):
                assert vd[y, x] == 0.0 and not vn[y, x].any()
    finally:
        ctx.close()


@pytest.mark.parametrize("key", [("real", False), ("crafted", "67x5")], ids=lambda k: "%s-%s" % k)
def test_accumulate_and_two_calls(dev, key):
    import brush_amd as ba
    maps, cp, w, h = _maps(key)
    ctx = ba.Context(dev)
    try:
        loss, vn, vd = _run(ba, ctx, dev, maps, cp, 0.7)
        loss2, vn2, vd2 = _run(ba, ctx, dev, maps, cp, 0.7)
        for a, b in ((loss, loss2), (vn, vn2), (vd, vd2)):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), "two calls give different bits"
        base = np.random.default_rng(5).uniform(-1e-3, 1e-3, (h, w)).astype(np.float32)
        onto = torch.from_numpy(base.copy()).to(dev)
        loss3, vn3, vd3 = _run(ba, ctx, dev, maps, cp, 0.7, v_depth=onto)
        assert np.array_equal(vd3.view(np.int32), (base + vd).view(np.int32)), "accumulate is not the map plus the overwrite result"
        assert np.array_equal(loss3.view(np.int32), loss.view(np.int32)) and np.array_equal(vn3.view(np.int32), vn.view(np.int32))
        assert float(np.abs(vd).max()) > 0
    finally:
        ctx.close()


@pytest.mark.parametrize("weight", [0.0, float("nan"), -1.0])
def test_no_term_gives_all_plus_zero(dev, weight):
    import brush_amd as ba
    maps, cp, w, h = _maps(("crafted", "67x5"))
    ctx = ba.Context(dev)
    try:
        loss, vn, vd = _run(ba, ctx, dev, maps, cp, weight)
        for t in (loss, vn, vd):
            assert not t.view(np.int32).any()
        base = np.full((h, w), 0.25, np.float32)
        loss, vn, vd = _run(ba, ctx, dev, maps, cp, weight, v_depth=torch.from_numpy(base.copy()).to(dev))
        assert np.array_equal(vd, base) and not loss.view(np.int32).any() and not vn.view(np.int32).any()   # untouched under accumulate
    finally:
        ctx.close()


def test_refusals(dev):
    import brush_amd as ba
    maps, cp, w, h = _maps(("crafted", "67x5"))
    ctx = ba.Context(dev)
    try:
        n, d, i = [torch.from_numpy(np.ascontiguousarray(m)).to(dev) for m in maps]
        kb4 = dict(cp)
        kb4["model"], kb4["dist"] = util.REF_LENSES["kb4"]
        with pytest.raises(ba.BrushHipError, match="pinhole"):
            ba.normal_consistency_value_and_grad(n, d, i, util.hip_camera(ba, kb4), 1.0, ctx=ctx)
        cam = util.hip_camera(ba, cp).uniforms((w, h))
        loss, vn, vd = torch.zeros(2, device=dev), torch.zeros_like(n), torch.zeros_like(d)
        p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        fn = ctx.lib.bh_normal_consistency_value_and_grad
        good = [ctx._h, C.byref(cam), p(n), p(d), p(i), h, w, 1.0, 0, p(loss), p(vn), p(vd)]
        assert fn(*good) == 0
        for k in (1, 2, 3, 4, 9, 10, 11):   # every pointer in turn
            args = list(good)
            args[k] = None
            assert fn(*args) == -1 and b"null" in ctx.lib.bh_last_error(ctx._h), k
        for k, v in ((5, 0), (6, 0)):
            args = list(good)
            args[k] = v
            assert fn(*args) == -1 and b"zero size" in ctx.lib.bh_last_error(ctx._h)
        # an output on top of an input (or inside it), and the two outputs on top of each other
        for k, t in ((10, n), (11, d), (11, i), (10, i), (11, vn)):
            args = list(good)
            args[k] = p(t)
            assert fn(*args) == -1 and b"alias" in ctx.lib.bh_last_error(ctx._h), k
        args = list(good)
        args[11] = C.c_void_p(i.data_ptr() + 64)
        assert fn(*args) == -1 and b"alias" in ctx.lib.bh_last_error(ctx._h)
        ctx.sync()
    finally:
        ctx.close()
