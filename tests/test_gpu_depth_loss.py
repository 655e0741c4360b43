"""bh_depth_loss_value_and_grad / bh_eval_depth_metrics (include/brush_hip_depth_loss.h) against tests/depth_loss_ref.py
on real expected-depth maps: a small synth scene's against a perturbed copy's, with a block of NaN / inf / 0 / -1 targets and an
empty border (E == 0).

Bounds (eps = 2^-24, one f32 rounding; c = f32(weight / (H W)); S = the exact float64 sum of |E - t| or |1/E - t| over valid pixels):
  v_depth, L1         sign(E - t) c: no rounding at all                                  -> bit-exact
  v_depth, disparity  -(s c) / (E E): one product and one quotient, and one more quotient (1/E) that only decides the sign
                      -> |delta| <= 3 eps |v|.  Pixels with |1/E - t| <= 2^-20 t (the sign may hang on the last place of 1/E) are
                      left out; they are at most 1 % of the valid pixels (checked with the restatement alone)
  loss[0]             per-pixel f32 terms: eps |d| for the difference, for disparity eps / E more for the quotient; the f64 sum
                      of N terms N 2^-52 S at most; one final rounding eps c S
  metrics             per-pixel terms and sums in float64 (N 2^-52 relative), one final rounding -> 2 eps relative; counts exact
Measured on an MI355X: disparity v_depth worst 0.00 eps, |loss - c S| at most a third of its bound, metrics within
0.71 eps."""
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import depth_loss_ref as dr
import util

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
SHAPES = {(16, 16): (400, 0x1D1), (37, 23): (1200, 0x1D2), (123, 82): (3000, 0x1D3)}   # (w, h) -> (splats, seed)
ALIGN = [(1.0, 0.0), (0.7, 0.05)]


def _depth_of(ba, ctx, sc, cam, w, h, dev):
    spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
    node = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx)
    d = node.depth("expected")
    ctx.sync()
    return d.cpu().numpy()


@pytest.fixture(scope="module")
def maps(dev):
    """(w, h) -> (E, z_gt): the scene's expected depth and a perturbed copy's with the invalid block; computed once, never written."""
    import brush_amd as ba
    out = {}
    ctx = ba.Context(dev)
    try:
        for (w, h), (n, seed) in SHAPES.items():
            cp = synth.default_camera_params(w, h)
            tans = (math.tan(cp["fov_x"] / 2.0), math.tan(cp["fov_y"] / 2.0))
            sc = synth.make_scene(n, seed, log_scale_range=(math.log(0.03), math.log(0.25)), tan_half_fov=tans, spread=0.6)
            cam = util.hip_camera(ba, cp)
            e = _depth_of(ba, ctx, sc, cam, w, h, dev)
            moved = dict(sc, transforms=sc["transforms"].copy())
            rng = np.random.default_rng(seed)
            moved["transforms"][:, :3] *= rng.uniform(0.9, 1.12, (n, 1)).astype(np.float32)   # along each splat's viewing ray
            z = _depth_of(ba, ctx, moved, cam, w, h, dev)
            z[h // 2, 2:6] = [np.nan, np.inf, 0.0, -1.0]
            z[h // 2 + 1, 2:6] = [-np.inf, np.nan, -0.0, -3.5]
            assert (e == 0).any() and (e > 0).sum() > e.size // 5
            e.setflags(write=False)
            z.setflags(write=False)
            out[(w, h)] = (e, z)
    finally:
        ctx.close()
    return out


def _gt(z, kind):
    if kind == "l1":
        return z
    with np.errstate(divide="ignore", invalid="ignore"):
        g = (np.float32(1.0) / z).astype(np.float32)
    g[~np.isfinite(z)] = z[~np.isfinite(z)]   # (NaN and inf targets stay what they are)
    return g


def _run(dev, e, gt, kind, weight, scale, offset, grad=True):
    import brush_amd as ba
    loss, v = ba.depth_loss_value_and_grad(torch.from_numpy(e.copy()).to(dev), torch.from_numpy(gt.copy()).to(dev), kind, weight, scale, offset, want_grad=grad)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), (v.cpu().numpy() if grad else None)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("kind", ["l1", "disparity"])
@pytest.mark.parametrize("scale,offset", ALIGN)
def test_kernel_against_the_restatement(dev, maps, shape, kind, scale, offset):
    e, z = maps[shape]
    gt = _gt(z, kind)
    weight = 0.5
    assert dr.t_is_safe(gt, scale, offset)
    ref = dr.loss_and_grad(e, gt, kind, weight, scale, offset)
    assert 0 < ref["count"] < e.size and not ref["valid"][e == 0].any()
    loss, v = _run(dev, e, gt, kind, weight, scale, offset)
    assert loss[1] == ref["count"]
    assert not v[~ref["valid"]].any() and not np.signbit(v[~ref["valid"]]).any()
    if kind == "l1":
        assert np.array_equal(v.view(np.int32), ref["v_depth"].view(np.int32))
        worst = 0.0
    else:
        ties = dr.tie_mask(e, gt, scale, offset)
        assert ties.sum() <= 0.01 * ref["count"], (int(ties.sum()), ref["count"])
        keep = ref["valid"] & ~ties
        d = np.abs(v.astype(np.float64) - ref["v_depth"].astype(np.float64))[keep]
        mag = np.abs(ref["v_depth"].astype(np.float64))[keep]
        worst = float((d / (EPS * mag)).max())
        assert (d <= 3 * EPS * mag).all(), worst
    # the loss against the exact float64 sum
    val = ref["valid"]
    ed, td = e[val].astype(np.float64), ref["t"][val].astype(np.float64)
    x = ed if kind == "l1" else 1.0 / ed
    exact = np.abs(x - td)
    c = float(dr.constant(weight, e.size))
    S = float(exact.sum())
    per_pixel = EPS * exact.sum() + (EPS * (1.0 / ed).sum() if kind == "disparity" else 0.0)
    bound = c * per_pixel + c * S * (EPS + ref["count"] * 2.0 ** -52)
    err = abs(float(loss[0]) - c * S)
    print("%s %s align (%g, %g): loss %.9g, |loss - c S| = %.3e (bound %.3e), v_depth worst %.2f eps, %d valid of %d"
          % (shape, kind, scale, offset, loss[0], err, bound, worst, ref["count"], e.size))
    assert err <= bound
    assert loss[0].tobytes() == ref["loss"].tobytes() or abs(float(loss[0]) - float(ref["loss"])) <= bound
    # two calls, and a call without a gradient, give the same bits
    loss2, v2 = _run(dev, e, gt, kind, weight, scale, offset)
    loss3, _ = _run(dev, e, gt, kind, weight, scale, offset, grad=False)
    assert loss.tobytes() == loss2.tobytes() == loss3.tobytes() and v.tobytes() == v2.tobytes()


@pytest.mark.parametrize("kind", ["l1", "disparity"])
def test_all_invalid_and_zero_weight(dev, maps, kind):
    e, z = maps[(37, 23)]
    for gt in (np.full_like(z, np.nan), np.zeros_like(z), -np.abs(np.nan_to_num(z, nan=1.0, posinf=1.0, neginf=1.0)) - 1.0):
        loss, v = _run(dev, e, gt, kind, 1.0, 1.0, 0.0)
        assert loss.tobytes() == np.zeros(2, np.float32).tobytes() and v.tobytes() == np.zeros_like(e).tobytes()
    loss, v = _run(dev, e, _gt(z, kind), kind, 0.0, 1.0, 0.0)
    assert loss.tobytes() == np.zeros(2, np.float32).tobytes() and v.tobytes() == np.zeros_like(e).tobytes()


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("kind", ["l1", "disparity"])
def test_metrics_against_the_restatement(dev, maps, shape, kind):
    import brush_amd as ba
    e, z = maps[shape]
    gt = _gt(z, kind)
    for scale, offset in ALIGN:
        want = dr.metrics(e, gt, kind, scale, offset)
        m = ba.eval_depth_metrics(torch.from_numpy(e.copy()).to(dev), torch.from_numpy(gt.copy()).to(dev), kind, scale, offset)
        m2 = ba.eval_depth_metrics(torch.from_numpy(e.copy()).to(dev), torch.from_numpy(gt.copy()).to(dev), kind, scale, offset)
        torch.cuda.synchronize()
        got = m.cpu().numpy().astype(np.float64)
        rel = np.abs(got[:3] - want[:3]) / np.maximum(np.abs(want[:3]), 1e-300)
        print("%s %s align (%g, %g): abs-rel %.6g rmse %.6g inliers %.6g valid %d; worst relative error %.2f eps (bound 2)"
              % (shape, kind, scale, offset, got[0], got[1], got[2], int(got[3]), rel.max() / EPS))
        assert got[3] == want[3] > 0 and (rel <= 2 * EPS).all()
        assert m.cpu().numpy().tobytes() == m2.cpu().numpy().tobytes()
    m = ba.eval_depth_metrics(torch.from_numpy(e.copy()).to(dev), torch.from_numpy(np.zeros_like(z)).to(dev), kind)
    torch.cuda.synchronize()
    assert m.cpu().numpy().tobytes() == np.zeros(4, np.float32).tobytes()


def test_arguments_are_checked(dev, maps):
    import brush_amd as ba
    e, z = maps[(16, 16)]
    et, zt = torch.from_numpy(e.copy()).to(dev), torch.from_numpy(z.copy()).to(dev)
    with pytest.raises(ba.BrushHipError, match="unknown depth loss kind"):
        ba.depth_loss_value_and_grad(et, zt, kind=2)
    with pytest.raises(ba.BrushHipError, match="unknown depth loss kind"):
        ba.eval_depth_metrics(et, zt, kind=7)
    with pytest.raises(ValueError):
        ba.depth_loss_value_and_grad(et, zt[:8], "l1")
