"""tests/depth_loss_ref.py against itself (no GPU): its v_depth is torch.autograd's in float64 for both kinds, invalid pixels
contribute nothing, an all-invalid map gives loss 0 and a zero gradient, and the metrics of a known map are what they must be."""
import numpy as np
import pytest
import torch

import depth_loss_ref as dr


def _maps(seed=3, h=19, w=27):
    rng = np.random.default_rng(seed)
    e = rng.uniform(0.5, 9.0, (h, w)).astype(np.float32)
    z = (e * rng.uniform(0.7, 1.4, (h, w))).astype(np.float32)
    return e, z


@pytest.mark.parametrize("kind", ["l1", "disparity"])
@pytest.mark.parametrize("scale,offset", [(1.0, 0.0), (0.7, 0.05)])
def test_gradient_is_autograds(kind, scale, offset):
    e, z = _maps()
    gt = z if kind == "l1" else (1.0 / z).astype(np.float32)
    weight = 0.37
    r = dr.loss_and_grad(e, gt, kind, weight, scale, offset)
    assert dr.t_is_safe(gt, scale, offset) and r["count"] == e.size and np.all(r["diff"] != 0)   # no pixel at E == t
    et = torch.tensor(e.astype(np.float64), requires_grad=True)
    t = torch.tensor(r["t"].astype(np.float64))
    x = et if kind == "l1" else 1.0 / et
    loss = float(dr.constant(weight, e.size)) * (x - t).abs().sum()
    loss.backward()
    want = et.grad.numpy()
    # L1: +-c exactly.  Disparity: 1/E decides only the sign; -(s c) / (E E) is two f32 roundings of the float64 value
    assert np.abs(r["v_depth"].astype(np.float64) - want).max() <= (0.0 if kind == "l1" else 2.0 ** -23 * np.abs(want).max())
    if kind == "disparity":
        assert (np.abs(r["v_depth"].astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want)).all()
    # the loss: f32 differences (2^-24 of the larger operand each), float64 sum, one final rounding
    slack = 2.0 ** -24 * (np.abs(x.detach().numpy()) + np.abs(t.numpy())).sum() * float(dr.constant(weight, e.size)) + 2.0 ** -24 * float(loss.detach())
    assert abs(float(r["loss"]) - float(loss.detach())) <= slack


@pytest.mark.parametrize("kind", ["l1", "disparity"])
def test_invalid_pixels_contribute_nothing(kind):
    e, z = _maps(5)
    gt = z if kind == "l1" else (1.0 / z).astype(np.float32)
    base = dr.loss_and_grad(e, gt, kind, 1.0)
    e2, gt2 = e.copy(), gt.copy()
    bad = [(0, 0, np.nan), (1, 3, np.inf), (2, 5, -np.inf), (3, 7, 0.0), (4, 9, -1.0)]
    for y, x, v in bad:
        gt2[y, x] = v
    e2[6, 11] = 0.0
    r = dr.loss_and_grad(e2, gt2, kind, 1.0)
    holes = [(y, x) for y, x, _ in bad] + [(6, 11)]
    assert r["count"] == e.size - len(holes)
    for y, x in holes:
        assert not r["valid"][y, x] and r["v_depth"][y, x] == 0 and not np.signbit(r["v_depth"][y, x])
    keep = np.ones(e.shape, bool)
    for y, x in holes:
        keep[y, x] = False
    assert np.array_equal(r["v_depth"][keep], base["v_depth"][keep])
    assert r["sum"] == pytest.approx(np.abs(base["diff"].astype(np.float64))[keep].sum(), rel=1e-14)
    m = dr.metrics(e2, gt2, kind)
    assert m[3] == r["count"] and np.isfinite(m).all()


def test_all_invalid_and_zero_weight():
    e, z = _maps(7)
    for gt in (np.full_like(z, np.nan), np.zeros_like(z), -z):
        r = dr.loss_and_grad(e, gt, "l1", 1.0)
        assert r["loss"] == 0 and r["count"] == 0 and not r["v_depth"].any() and not np.signbit(r["v_depth"]).any()
        assert np.array_equal(dr.metrics(e, gt), np.zeros(4))
    r = dr.loss_and_grad(np.zeros_like(e), z, "disparity", 1.0)
    assert r["loss"] == 0 and r["count"] == 0 and not r["v_depth"].any()
    r = dr.loss_and_grad(e, z, "l1", 0.0)
    assert r["loss"] == 0 and r["count"] == 0 and not r["v_depth"].any()


def test_metrics_of_a_known_map():
    z = np.full((4, 5), 2.0, np.float32)
    e = z.copy()
    e[0, :] = 3.0    # five pixels 50 % too deep: outside 1.25
    e[1, 0] = 0.0    # empty
    m = dr.metrics(e, z)
    assert m[3] == 19 and m[0] == pytest.approx(5 * 0.5 / 19) and m[1] == pytest.approx(np.sqrt(5.0 / 19)) and m[2] == pytest.approx(14 / 19)
    md = dr.metrics(e, (1.0 / z).astype(np.float32), "disparity")
    assert np.allclose(md, m)
    # an exact E == t pixel: derivative 0, and a sign tie is reported by tie_mask
    r = dr.loss_and_grad(z, z, "l1", 1.0)
    assert r["loss"] == 0 and not r["v_depth"].any() and r["count"] == z.size
    assert dr.tie_mask(z, (1.0 / z).astype(np.float32)).all()
