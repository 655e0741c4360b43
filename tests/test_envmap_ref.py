"""tests/envmap_ref.py, the numpy restatement of include/brush_hip_envmap.h, against a float64 torch.autograd evaluation of the same
formula on the 64x48 scene that sees three faces and a cube corner: the forward to 4 ulp, the integer gradient to the table within
the bound its three roundings give, the gradient to alpha, exact zeros where no pixel reaches, and exact scaling by powers of two.

The float64 evaluation takes the restatement's taps (texel indices and f32 weights) as given: they are the discrete and the
ill-conditioned part of the lookup (floor(u) moves by a whole texel under a rounding), and what is compared is the arithmetic behind
them."""
import numpy as np
import pytest
import torch

import envmap_ref as vr

EPS = 2.0 ** -24
RES = (1, 2, 4, 8, 64)
_CASES = {}


def _case(res):
    if res not in _CASES:
        c = vr.scene(res)
        h, w = c["h"], c["w"]
        texel, weight = vr.taps(c["cam"], h, w, res)
        table = torch.tensor(c["table"].astype(np.float64).reshape(-1, 3), requires_grad=True)
        img = torch.tensor(c["img"].astype(np.float64), requires_grad=True)
        e = (table[torch.from_numpy(texel)] * torch.from_numpy(weight.astype(np.float64))[..., None]).sum(-2)   # [h,w,3]
        out = img[..., :3] + (1.0 - img[..., 3:]) * e
        v = torch.tensor(c["v"].astype(np.float64))
        ((out * v[..., :3]).sum() + (img[..., 3] * v[..., 3]).sum()).backward()
        c.update(texel=texel, weight=weight, out64=out.detach().numpy(), e64=e.detach().numpy(), v_E64=table.grad.numpy().reshape(6, res, res, 3),
                 v_img64=img.grad.numpy(), fwd=vr.composite(c["table"], c["img"], c["cam"]), bwd=vr.backward(c["table"], c["img"], c["v"], c["cam"]))
        _CASES[res] = c
    return _CASES[res]


def test_the_scene_sees_three_faces_and_the_corner():
    c = _case(8)
    faces = set((c["texel"] // 64).reshape(-1).tolist())
    assert faces == {0, 2, 4}
    assert c["texel"].min() >= 0 and c["texel"].max() < 6 * 64
    assert (c["weight"] >= 0).all() and np.abs(c["weight"].astype(np.float64).sum(-1) - 1).max() <= 4 * EPS
    assert 0.25 < (c["img"][..., 3] == 1).mean() < 0.35


@pytest.mark.parametrize("res", RES)
def test_forward_agrees_to_4_ulp(res):
    c = _case(res)
    got = c["fwd"]
    assert got.dtype == np.float32 and np.array_equal(got[..., 3], c["img"][..., 3])
    err = np.abs(got[..., :3].astype(np.float64) - c["out64"])
    ulp = np.spacing(np.abs(c["out64"]).astype(np.float32)).astype(np.float64)
    print("R=%d forward: max err / ulp = %.3f (bound 4)" % (res, float((err / ulp).max())))
    assert (err <= 4 * ulp).all()


@pytest.mark.parametrize("res", RES)
def test_table_gradient_is_within_its_bound_and_zero_where_untouched(res):
    c = _case(res)
    b = c["bwd"]
    exact = c["v_E64"]
    err = np.abs(b["v_E"].astype(np.float64) - exact)
    bound = b["contrib_abs"] * 3 * EPS + b["count"][..., None] / (2 * b["S"]) + np.abs(exact) * EPS
    touched = b["touched"]
    ratio = float((err[touched] / bound[touched]).max())
    print("R=%d v_E: max err / bound = %.3f, max |acc| = 2^%.1f, %d of %d texels touched" %
          (res, ratio, np.log2(float(np.abs(b["acc"]).max())), int(touched.sum()), touched.size))
    assert (err <= bound).all(), ratio
    assert np.abs(b["acc"]).max() < 2 ** 61
    assert not b["v_E"][~touched].any() and not np.signbit(b["v_E"][~touched]).any()
    assert not exact[~touched].any()
    if res == 64:
        assert not touched.all()


@pytest.mark.parametrize("res", RES)
def test_frame_gradient(res):
    """v_img's rgb is v's; its alpha is v_a minus the sky's term sum_c v_c E_c, one exact f32 subtraction away from the term, and the
    term agrees with autograd's (v_a - v_img_a in f64) within 3 * 2^-24 * sum_c |v_c E_c|."""
    c = _case(res)
    b = c["bwd"]
    assert np.array_equal(b["v_img"][..., :3], c["v"][..., :3])
    assert np.array_equal(b["v_img"][..., 3], c["v"][..., 3] - b["sky"])
    sky64 = c["v"][..., 3].astype(np.float64) - c["v_img64"][..., 3]
    assert np.abs(sky64 - (c["v"][..., :3].astype(np.float64) * c["e64"]).sum(-1)).max() <= 1e-14
    mass = np.abs(c["v"][..., :3].astype(np.float64) * c["e64"]).sum(-1)
    err = np.abs(b["sky"].astype(np.float64) - sky64)
    print("R=%d v_a: max err / (2^-24 sum |v_c E_c|) = %.3f (bound 3)" % (res, float((err / (EPS * mass)).max())))
    assert (err <= 3 * EPS * mass).all()


@pytest.mark.parametrize("k", (60, -100))
def test_scaling_the_cotangent_by_a_power_of_two_scales_the_gradient_exactly(k):
    c = _case(8)
    scaled = vr.backward(c["table"], c["img"], np.ldexp(c["v"], k).astype(np.float32), c["cam"])
    assert np.array_equal(scaled["v_E"].astype(np.float64), np.ldexp(c["bwd"]["v_E"].astype(np.float64), k))
    assert np.array_equal(scaled["acc"], c["bwd"]["acc"])


def test_zero_and_non_finite_cotangents():
    c = _case(4)
    z = vr.backward(c["table"], c["img"], np.zeros_like(c["v"]), c["cam"])
    assert not z["v_E"].any() and not np.isnan(z["v_E"]).any() and not z["touched"].any()
    bad = c["v"].copy()
    bad[3, 5, 1] = np.inf
    with pytest.raises(ValueError):
        vr.backward(c["table"], c["img"], bad, c["cam"])


def test_fma32_is_a_correctly_rounded_fma():
    # 1 + 2^-24 + 2^-48 rounds up in one rounding, but (1 + 2^-24) rounded to f64 then f32 ties to even: the case double rounding gets wrong
    a, b = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)          # a b = 1 + 2^-11 + 2^-24
    c = np.float32(2.0 ** -60)
    assert vr.fma32(a, b, c) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert vr.fma32(a, b, -c) == np.float32(1 + 2.0 ** -11)
    rng = np.random.default_rng(7)
    x, y, z = (rng.uniform(-1, 1, 4096).astype(np.float32) for _ in range(3))
    from fractions import Fraction
    got = vr.fma32(x, y, z)
    for i in range(0, 4096, 64):
        exact = Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        assert abs(exact - Fraction(float(got[i]))) <= min(abs(exact - Fraction(float(lo))), abs(exact - Fraction(float(hi))))


def test_adam_is_plain_adam_and_rests_at_zero():
    rng = np.random.default_rng(3)
    p, g = rng.normal(size=24).astype(np.float32), rng.normal(size=24).astype(np.float32)
    q, m1, m2, t = vr.adam_step(p, np.zeros(24, np.float32), np.zeros(24, np.float32), 0, g, 0.01)
    assert t == 1 and q.dtype == np.float32
    assert np.abs(q - (p - 0.01 * np.sign(g))).max() <= 1e-6          # the first step moves every element by lr
    tp = torch.tensor(p.astype(np.float64), requires_grad=True)
    opt = torch.optim.Adam([tp], lr=0.01, betas=(0.9, 0.999), eps=1e-15)
    m1 = m2 = np.zeros(24, np.float32)
    pp, t = p, 0
    for _ in range(5):
        tp.grad = torch.tensor(g.astype(np.float64))
        opt.step()
        pp, m1, m2, t = vr.adam_step(pp, m1, m2, t, g, 0.01)
    assert np.abs(pp - tp.detach().numpy()).max() <= 1e-5
    same, z1, z2, _ = vr.adam_step(p, np.zeros(24, np.float32), np.zeros(24, np.float32), 7, np.zeros(24, np.float32), 0.01)
    assert np.array_equal(same.view(np.int32), p.view(np.int32)) and not z1.any() and not z2.any()
    assert vr.pow_by_squaring(0.9, 5) == 0.9 * (0.9 * 0.9) * (0.9 * 0.9) or abs(vr.pow_by_squaring(0.9, 5) - 0.9 ** 5) < 1e-15
