"""tests/exposure_ref.py against torch autograd in float64 (CPU only, no library): the backward's v and v_m, the L1 masses, the
identity, and Adam against torch.optim.Adam."""
import numpy as np
import torch

import exposure_ref as er


def _case(seed, h, w):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, (h, w, 4))
    v = rng.uniform(-1.0, 1.0, (h, w, 4))
    m = er.IDENTITY + rng.uniform(-0.3, 0.3, 12)
    return m, x, v


def test_backward_is_autograd_of_apply():
    for seed, (h, w) in enumerate(((5, 3), (16, 16), (41, 27))):
        m, x, v = _case(seed, h, w)
        mt = torch.tensor(m, dtype=torch.float64, requires_grad=True)
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        a, b = mt.reshape(3, 4)[:, :3], mt.reshape(3, 4)[:, 3]
        y = torch.cat([xt[..., :3] @ a.T + b, xt[..., 3:]], dim=-1)
        assert np.abs(y.detach().numpy() - er.apply(m, x)).max() <= 1e-14
        (y * torch.tensor(v)).sum().backward()
        got = er.backward(m, x, v)
        assert np.abs(got["v_m"] - mt.grad.numpy()).max() <= 1e-12
        assert np.abs(got["v_img"] - xt.grad.numpy()).max() <= 1e-12
        assert (got["S"] >= np.abs(got["v_m"]) - 1e-12).all() and (got["S"] > 0).all()
        assert (got["v_mass"] >= np.abs(got["v_img"][..., :3]) - 1e-12).all()
        assert (er.apply_mass(m, x) >= np.abs(er.apply(m, x)[..., :3]) - 1e-12).all()


def test_identity_changes_nothing():
    _, x, v = _case(7, 9, 4)
    assert np.array_equal(er.apply(er.IDENTITY, x), x)
    assert np.array_equal(er.backward(er.IDENTITY, x, v)["v_img"], v)


def test_mse_cotangent_is_autograd():
    m, x, _ = _case(3, 6, 5)
    target = er.apply(er.M_STAR, x)
    yt = torch.tensor(er.apply(m, x), requires_grad=True)
    ((yt[..., :3] - torch.tensor(target)[..., :3]) ** 2).mean().backward()
    assert np.abs(er.mse_cotangent(yt.detach().numpy(), target) - yt.grad.numpy()).max() <= 1e-15


def test_adam_is_torch_adam():
    rng = np.random.default_rng(11)
    p = torch.tensor(er.IDENTITY.copy(), requires_grad=True)
    opt = torch.optim.Adam([p], lr=0.01, betas=(0.9, 0.999), eps=1e-8)
    m, m1, m2, t = er.IDENTITY.copy(), np.zeros(12), np.zeros(12), 0
    for _ in range(6):
        g = rng.uniform(-1.0, 1.0, 12)
        p.grad = torch.tensor(g)
        opt.step()
        m, m1, m2, t = er.adam_step(m, m1, m2, t, g, 0.01)
        assert np.abs(m - p.detach().numpy()).max() <= 1e-12
    assert t == 6
    same = er.adam_step(m, m1, m2, t, g, 0.0)
    assert np.array_equal(same[0], m) and same[3] == 7 and not np.array_equal(same[1], m1)


def test_recovery_loop_converges_on_a_synthetic_image():
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 1.0, (12, 10, 4))
    start, end = er.recovery(x)
    assert start == np.abs(er.IDENTITY - er.M_STAR).max() and end <= start / 20.0
