"""The fused image loss pair (brush_amd/csrc/loss_fused.hip: pass A loss_fused_forward_kernel, pass B loss_fused_backward_kernel)
pinned where the suite did not reach: against float64 on the image families of tests/loss_cases.py, each term alone and exactly,
and the strip-wise launch (launch_image_loss_fused_window) through the test hook bh_debug_image_loss_window (api.hip).

(h, w):
  115 x 40    8 tile rows, the last one 3 px tall; 3 tile columns, row-major mapping; w % 4 == 0: pass B's wide-row path
  115 x 18    8 tile rows, 2 tile columns: the narrow-row path
  83 x 260    6 tile rows, 17 tile columns: banded mapping, bands 3 wide, a partial band and two empty ones
  1 x 1       degenerate
  16 x 16     a single tile

D1, the float64 yardstick: err_gpu <= max(3 x err_oracle, floor), both errors against oracle/autograd_loss_ref.py on the same case
and the same pixels; floor = the suite's 2e-6 x max(1, |loss|) and 2e-6 x max|g|.  The fused kernels keep the oracle's accumulation
order and differ from it by FMA contraction and two 1-ulp reciprocals, roundings of the size the oracle makes itself: their worst
pixel may differ from the oracle's by a small factor, not by an order.  The bound is never taken from the kernels' own output.

Measured err_gpu / err_oracle of the fused gradient on an MI355X, the worst over both shapes, both weight pairs and the three modes
(region and case pairs where the floor rules, i.e. both errors are below 2e-6 x max|g|, are left out: "-"; 147 of the 504 are):

  family        border   seam   interior
  noise           -        -       -        (the floor rules everywhere; the worst error is 0.94 of it)
  flat_bright    1.04     0.99    1.17
  converged      1.59     1.08    1.32
  ramp           1.33     1.22    1.07
  black_bg       0.78     0.77    0.80
  inverted       1.01     1.02    1.41
  identical       -       1.34    2.54     (115 x 40, 0.8 / -0.2, masked: 6.8e-9 against 2.7e-9, with max|g| 1.4e-3)

The fused scalar loss: at most 1.73 x the oracle's error (ramp 83 x 260, SSIM alone: 2.3e-6 against 1.3e-6).  The stand-alone pair of
loss.hip, compiled without contraction: 1.00 in every region of every case, map and gradient.  Nothing came near an order.

D2 and D3 are exact.  What D3 needs to mean anything: the context's scratch outlives a call, so a window that did not compute a row
of partials it reads would find the right values there from the whole-image call before it (the first version of this test let
"pass A skips the tile row above the strip" through); window() poisons the scratch first.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import loss_cases as lc

gpu = pytest.mark.gpu
FILL = 0x7FC00BAD   # a quiet NaN nobody computes
WINDOWS = [(0, 1), (0, 2), (1, 2), (1, 4), (2, 3), (3, 8), (7, 8), (0, 8)]
PARTITIONS = [[(0, 3), (3, 4), (4, 8)], [(0, 1), (1, 8)]]


@pytest.fixture(scope="module")
def ctx(dev):
    import brush_amd as ba
    from brush_amd import _ffi
    c = ba.Context(dev, lib=_ffi.load_test_hooks())
    yield c
    c.close()


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _gt_dev(gt, dev):
    return torch.tensor(np.ascontiguousarray(gt).view(np.int32)).to(dev)


def _img_dev(img, dev):
    return torch.tensor(np.ascontiguousarray(img, np.float32)).to(dev)   # (a copy: the cases are read-only arrays)


def fused(ctx, dev, img, gt, weights, bg, mask, alpha_w):
    import brush_amd as ba
    loss, v = ba.image_loss_value_and_grad(_img_dev(img, dev), _gt_dev(gt, dev), weights[0], weights[1], composite_bg=bg, mask=mask,
                                           alpha_weight=alpha_w, ctx=ctx)
    return loss.cpu().numpy()[0], v.cpu().numpy()


def window(ctx, img_t, gt_t, h, w, weights, bg, mask, alpha_w, y0, y1):
    """One bh_debug_image_loss_window into NaN-filled outputs -> (return code, loss float32, v_output [H,W,4] float32).
    The context's scratch — pass A's nine partial planes and its per-tile loss sums — still holds what the last call on an image of
    this size left, for the same image the very values a window should have computed itself: a whole-image call on an all-NaN
    render turns every word of both into NaN first, so a plane row or a tile sum the window reads without writing it shows."""
    from brush_amd import host
    fill = int(np.uint32(FILL).view(np.int32))
    loss = torch.full((1,), fill, dtype=torch.int32, device=img_t.device)
    v = torch.full((h, w, 4), fill, dtype=torch.int32, device=img_t.device)
    cfg = host._loss_cfg(weights[0], weights[1], bg, mask)
    nan_img = torch.full((h, w, 4), float("nan"), dtype=torch.float32, device=img_t.device)
    rc = ctx.lib.bh_debug_image_loss_window(ctx._h, _ptr(nan_img), _ptr(gt_t), h, w, C.byref(cfg), float(alpha_w), 0, (h + 15) // 16, _ptr(loss), _ptr(v))
    assert rc == 0 and torch.isnan(v.view(torch.float32)[..., :3]).all().item() and torch.isnan(loss.view(torch.float32)).all().item()
    loss.fill_(fill)
    v.fill_(fill)
    rc = ctx.lib.bh_debug_image_loss_window(ctx._h, _ptr(img_t), _ptr(gt_t), h, w, C.byref(cfg), float(alpha_w), y0, y1, _ptr(loss), _ptr(v))
    return rc, loss.cpu().numpy().view(np.float32)[0], v.cpu().numpy().view(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# D1: float64 yardstick
# ---------------------------------------------------------------------------------------------------------------------------
def _held(err_gpu, err_oracle, floor):
    return err_gpu <= max(3.0 * err_oracle, floor)


@gpu
@pytest.mark.parametrize("mode", list(lc.MODES))
@pytest.mark.parametrize("weights", lc.WEIGHTS[:2], ids=lambda t: "l1_%g_ssim_%g" % t)
@pytest.mark.parametrize("h,w", [(115, 40), (83, 260)])
@pytest.mark.parametrize("family", list(lc.FAMILIES))
def test_loss_pair_against_float64(dev, ctx, family, h, w, weights, mode):
    import brush_amd as ba
    img, gt = lc.case(family, h, w)
    bg, mask, alpha_w = lc.MODES[mode]
    y = lc.yardsticks(family, h, w, weights, mode)
    ch, tag = y["ch"], "%s %dx%d l1 %g ssim %g %s" % (family, h, w, weights[0], weights[1], mode)
    missed = []

    loss, g = fused(ctx, dev, img, gt, weights, bg, mask, alpha_w)
    assert g.shape == (h, w, 4) and np.isfinite(g).all() and np.isfinite(loss)
    if ch == 3:
        assert not g[..., 3].any()
    e_gpu, e_or, floor = abs(float(loss) - y["loss64"]), abs(y["loss32"] - y["loss64"]), 2e-6 * max(1.0, abs(y["loss64"]))
    print("RATIO %s | fused loss | gpu %.3g oracle %.3g floor %.3g" % (tag, e_gpu, e_or, floor))
    if not _held(e_gpu, e_or, floor):
        missed.append(("fused loss", e_gpu, e_or, floor))

    # the stand-alone pair of loss.hip on the same case, chain factor 1 / (3 h w) (alpha plane: alpha weight / (h w))
    pred_t, gt_t = _img_dev(img[..., :ch], dev), _gt_dev(gt, dev)
    lm = ba.image_loss(pred_t, gt_t, weights[0], weights[1], composite_bg=bg, mask=mask, ctx=ctx).cpu().numpy().transpose(2, 0, 1)
    dl_t = _img_dev(y["dl"].transpose(1, 2, 0), dev)
    gs = ba.image_loss_backward(pred_t, gt_t, dl_t, weights[0], weights[1], composite_bg=bg, mask=mask, ctx=ctx).cpu().numpy()
    assert np.isfinite(lm).all() and np.isfinite(gs).all()
    e_gpu, e_or = float(np.abs(lm.astype(np.float64) - y["map64"]).max()), float(np.abs(y["map32"].astype(np.float64) - y["map64"]).max())
    floor = 2e-6 * max(1.0, float(np.abs(y["map64"]).max()))
    print("RATIO %s | standalone map | gpu %.3g oracle %.3g floor %.3g" % (tag, e_gpu, e_or, floor))
    if not _held(e_gpu, e_or, floor):
        missed.append(("standalone map", e_gpu, e_or, floor))

    floor = 2e-6 * float(np.abs(y["grad64"]).max())
    for name, where in lc.regions(h, w).items():
        e_or = lc.grad_err(y["grad32"], y, where)
        for what, got in (("fused grad", g), ("standalone grad", gs)):
            e_gpu = lc.grad_err(got, y, where)
            print("RATIO %s | %s %s | gpu %.3g oracle %.3g floor %.3g ratio %.3g" % (tag, what, name, e_gpu, e_or, floor, e_gpu / e_or if e_or else np.inf))
            if not _held(e_gpu, e_or, floor):
                missed.append((what + " " + name, e_gpu, e_or, floor))
    assert not missed, (tag, missed)


# ---------------------------------------------------------------------------------------------------------------------------
# D2: each term alone
# ---------------------------------------------------------------------------------------------------------------------------
L1_MODES = [(None, False, 0.0), ((0.0, 0.0, 0.0), False, 0.1), (None, True, 0.1)]   # (bg = 0: contraction may fuse a composite's multiply-add)


def l1_gradient_f32(img, gt, mask, alpha_w):
    """Pass B with ssim_w = 0, l1_w = 1, restated in float32: fma(0, ssim_grad, 1 * sign * chain) = sign * chain for any finite
    ssim_grad.  -> [H,W,4]."""
    h, w = gt.shape
    f = np.float32
    d = lc.decode_f32(gt)
    ga = d[..., 3]
    dl_rgb = f(1.0) / f(h * w * 3)
    dl_alpha = f(alpha_w) / f(h * w) if alpha_w > 0 else f(0.0)
    chain_rgb = (dl_rgb * ga if mask else np.full((h, w), dl_rgb, f)).astype(f)
    chain_a = (dl_alpha * ga if mask else np.full((h, w), dl_alpha, f)).astype(f)
    out = np.zeros((h, w, 4), f)
    out[..., :3] = np.sign(img[..., :3] - d[..., :3]).astype(f) * chain_rgb[..., None]
    if alpha_w > 0:
        out[..., 3] = np.sign(img[..., 3] - ga).astype(f) * chain_a
    return out


@gpu
@pytest.mark.parametrize("h,w", lc.SHAPES)
@pytest.mark.parametrize("family", list(lc.FAMILIES))
def test_l1_term_alone_is_exact(dev, ctx, family, h, w):
    from oracle import autograd_loss_ref
    img, gt = lc.case(family, h, w)
    ties = img == lc.decode_f32(gt)   # [H,W,4]
    if family == "identical":
        ys, xs = lc.identical_patch(h, w)
        outside = np.ones((h, w), bool)
        outside[ys, xs] = False
        assert ties[outside].all() and (outside.any() or h * w == 1)
    if family == "black_bg":
        assert ties[~lc.disc(h, w)].all()
    for bg, mask, alpha_w in L1_MODES:
        tag = (family, h, w, bg, mask, alpha_w)
        loss, g = fused(ctx, dev, img, gt, (1.0, 0.0), bg, mask, alpha_w)
        want = l1_gradient_f32(img, gt, mask, alpha_w)
        # (value equality of floats is bit equality except between +0 and -0: a tie's gradient may be either)
        bad = g != want
        assert not bad.any(), (tag, int(bad.sum()), [tuple(i) for i in np.argwhere(bad)[:4]], g[bad][:4], want[bad][:4])
        nch = 4 if alpha_w > 0 else 3
        assert not g[..., :nch][ties[..., :nch]].any(), tag   # every tie: exactly zero
        if nch == 3:
            assert not g[..., 3].any(), tag
        m = autograd_loss_ref.loss_map(torch.tensor(np.ascontiguousarray(img[..., :nch].transpose(2, 0, 1)).astype(np.float64)), gt, 1.0, 0.0, bg, mask).numpy()
        ref = float(m[:3].mean() + (alpha_w * m[3].mean() if nch == 4 else 0.0))
        assert abs(float(loss) - ref) <= 2e-6 * max(1.0, abs(ref)), (tag, float(loss), ref)


@gpu
@pytest.mark.parametrize("h,w", lc.SHAPES)
def test_ssim_term_alone_on_identical_images_is_one(dev, ctx, h, w):
    """The figure of test_gpu_loss_optim.py::test_ssim_of_identical_images_is_one, 1e-5, for the stand-alone map; the fused loss is
    the float32 mean of such values: 1e-5 plus the suite's 2e-6 for the summation."""
    import brush_amd as ba
    img, gt = lc.identical(h, w, 1, patch=False)
    lm = ba.image_loss(_img_dev(img[..., :3], dev), _gt_dev(gt, dev), 0.0, 1.0, ctx=ctx).cpu().numpy()
    assert np.abs(lm - 1.0).max() <= 1e-5, float(np.abs(lm - 1.0).max())
    loss, g = fused(ctx, dev, img, gt, (0.0, 1.0), None, False, 0.0)
    assert abs(float(loss) - 1.0) <= 1e-5 + 2e-6, float(loss)
    assert np.isfinite(g).all()


# ---------------------------------------------------------------------------------------------------------------------------
# D3: strip windows through the hook
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mask,alpha_w", [(False, 0.0), (True, 0.1)], ids=["plain", "mask_alpha"])
@pytest.mark.parametrize("family", ["noise", "converged"])
@pytest.mark.parametrize("h,w", [(115, 40), (115, 18), (83, 260)])
def test_strip_windows(dev, ctx, h, w, family, mask, alpha_w):
    img, gt = lc.case(family, h, w)
    weights, gy = (0.8, -0.2), (h + 15) // 16
    img_t, gt_t = _img_dev(img, dev), _gt_dev(gt, dev)
    whole_loss, whole = fused(ctx, dev, img, gt, weights, None, mask, alpha_w)
    assert np.isfinite(whole).all() and np.isfinite(whole_loss)
    rng = np.random.default_rng(h * 131 + w)
    shares = {}
    for y0, y1 in WINDOWS:
        if y0 >= gy:
            continue   # (refused: test_window_hook_refusals)
        r0, r1 = 16 * y0, min(16 * y1, h)
        tag = (h, w, family, mask, y0, y1)
        rc, loss, v = window(ctx, img_t, gt_t, h, w, weights, None, mask, alpha_w, y0, y1)   # y1 as asked: the launcher clips it
        assert rc == 0, (tag, ctx.lib.bh_last_error(ctx._h))
        # each output's arithmetic does not depend on where its 32-row block starts
        assert np.array_equal(_bits(v[r0:r1]), _bits(whole[r0:r1])), (tag, int((_bits(v[r0:r1]) != _bits(whole[r0:r1])).sum()))
        outside = np.concatenate([_bits(v[:r0]).ravel(), _bits(v[r1:]).ravel()])
        assert (outside == FILL).all(), (tag, "rows outside the window were written", int((outside != FILL).sum()))
        assert np.isfinite(loss), tag
        shares[(y0, min(y1, gy))] = loss
        if (y0, min(y1, gy)) == (0, gy):
            assert _bits(loss) == _bits(whole_loss), (tag, float(loss), float(whole_loss))
        # the halo contract (brush_hip.h): nothing further than 21 rows outside the strip reaches an output
        far = np.ones(h, bool)
        far[max(r0 - 21, 0):min(r1 + 21, h)] = False
        if far.any():
            img2, gt2 = img.copy(), gt.copy()
            img2[far] = np.nan
            gt2[far] = rng.integers(0, 1 << 32, gt2[far].shape, dtype=np.uint64).astype(np.uint32)
            rc, loss2, v2 = window(ctx, _img_dev(img2, dev), _gt_dev(gt2, dev), h, w, weights, None, mask, alpha_w, y0, y1)
            assert rc == 0, tag
            assert np.array_equal(_bits(v2), _bits(v)), (tag, "rows beyond the 21-row halo reach v_output", int((_bits(v2) != _bits(v)).sum()))
            assert _bits(loss2) == _bits(loss), (tag, "rows beyond the 21-row halo reach the loss", float(loss2), float(loss))
    assert (0, gy) in shares
    for part in PARTITIONS:
        part = [(a, min(b, gy)) for a, b in part if a < gy]
        assert part[0][0] == 0 and part[-1][1] == gy and all(p[1] == q[0] for p, q in zip(part, part[1:]))
        for p in part:
            if p not in shares:
                rc, shares[p], _ = window(ctx, img_t, gt_t, h, w, weights, None, mask, alpha_w, p[0], p[1])
                assert rc == 0, p
        total = sum(float(shares[p]) for p in part)
        assert abs(total - float(whole_loss)) <= 2e-6 * max(1.0, abs(float(whole_loss))), (part, total, float(whole_loss))   # the summation order differs


@gpu
def test_window_hook_refusals(dev, ctx):
    """launch_image_loss_fused_window clips tile_y1 to the image's tile rows and refuses an empty window with BH_ERR_INVALID_ARG (-1);
    the hook refuses null pointers, an empty image and tile_y0 >= tile_y1 with the same code, and a null ctx."""
    from brush_amd import host
    h, w, gy = 40, 24, 3
    img, gt = lc.case("noise", h, w)
    img_t, gt_t = _img_dev(img, dev), _gt_dev(gt, dev)
    fill = int(np.uint32(FILL).view(np.int32))
    loss = torch.full((1,), fill, dtype=torch.int32, device=dev)
    v = torch.full((h, w, 4), fill, dtype=torch.int32, device=dev)
    cfg = host._loss_cfg(0.8, -0.2, None, False)
    fn = ctx.lib.bh_debug_image_loss_window
    good = [_ptr(img_t), _ptr(gt_t), h, w, C.byref(cfg), 0.1, 0, gy, _ptr(loss), _ptr(v)]

    def call(**over):
        a = list(good)
        for i, val in over.items():
            a[int(i[1:])] = val
        return fn(ctx._h, *a)
    for y0, y1 in ((1, 1), (2, 1), (gy, gy + 1), (gy + 4, gy + 9), (gy, 0xFFFFFFFF)):   # empty; behind the last tile row
        assert call(a6=y0, a7=y1) == -1, (y0, y1)
        assert b"empty tile-row window" in ctx.lib.bh_last_error(ctx._h), (y0, y1)
    for i in (0, 1, 4, 8, 9):
        assert call(**{"a%d" % i: None}) == -1, i
    assert call(a2=0) == -1 and call(a3=0) == -1
    assert fn(None, *good) == -1
    torch.cuda.synchronize(dev)
    assert (loss.cpu().numpy().view(np.uint32) == FILL).all() and (v.cpu().numpy().view(np.uint32) == FILL).all()   # nothing ran
    assert call() == 0   # ... and the same arguments untouched are taken
    assert np.isfinite(v.cpu().numpy().view(np.float32)).all()
