"""Per-view exposure compensation on the GPU (include/brush_hip_exposure.h) against tests/exposure_ref.py: apply,
backward, the device Adam step by step, the recovery of a known transform, and the errors.

Sizes: fewer pixels than a wave, one block, ragged against 64 and 256, and 521x504 = 262,584 pixels, which is one pass of the
backward's capped grid (1024 blocks x 256 lanes = 262,144) plus a ragged remainder of 440."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import exposure_ref as er

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
SIZES = ((5, 3), (16, 16), (123, 82), (521, 504))   # (w, h)
_CASES = {}


def _case(w, h):
    """Seeded inputs and their float64 reference, computed once per size and shared (never modified)."""
    if (w, h) not in _CASES:
        rng = np.random.default_rng(1000 * w + h)
        x = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float32)
        v = rng.uniform(-1.0, 1.0, (h, w, 4)).astype(np.float32)
        m = (er.IDENTITY + rng.uniform(-0.3, 0.3, 12)).astype(np.float32)
        c = dict(x=x, v=v, m=m, y=er.apply(m, x), y_mass=er.apply_mass(m, x), bwd=er.backward(m, x, v))
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CASES[(w, h)] = c
    return _CASES[(w, h)]


@pytest.fixture
def ctx(dev):
    import brush_amd as ba
    c = ba.Context(dev)
    yield c
    c.close()


def _table(ctx, m=None, views=3, lr=1e-3):
    import brush_amd as ba
    tab = ba.ExposureTable(views, lr=lr, ctx=ctx)
    if m is not None:
        tab.set_view(2, m)
    return tab


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("w,h", SIZES)
def test_apply(ctx, dev, w, h):
    c = _case(w, h)
    tab = _table(ctx, c["m"])
    x = torch.from_numpy(c["x"]).to(dev)
    y = tab.apply(2, x)
    got = y.cpu().numpy().astype(np.float64)
    err = np.abs(got[..., :3] - c["y"][..., :3])
    ratio = float((err / (EPS * c["y_mass"])).max())
    print("apply %dx%d: max |y - ref| / (2^-24 mass) = %.3f (bound 4)" % (w, h, ratio))
    assert (err <= 4 * EPS * c["y_mass"]).all(), ratio
    assert torch.equal(_bits(y[..., 3]), _bits(x[..., 3]))
    assert torch.equal(tab.apply(1, x), x)   # row 1 is still the identity
    inplace = x.clone()
    assert tab.apply(2, inplace, out=inplace) is inplace
    assert torch.equal(_bits(inplace), _bits(y))


@pytest.mark.parametrize("w,h", SIZES)
def test_backward(ctx, dev, w, h):
    c = _case(w, h)
    ref = c["bwd"]
    tab = _table(ctx, c["m"])
    x, v = torch.from_numpy(c["x"]).to(dev), torch.from_numpy(c["v"]).to(dev)
    out = tab.backward(2, x, v)
    grad = tab.grads
    got = out.cpu().numpy().astype(np.float64)
    err = np.abs(got[..., :3] - ref["v_img"][..., :3])
    print("backward %dx%d: max |v - ref| / (2^-24 mass) = %.3f (bound 4)" % (w, h, float((err / (EPS * ref["v_mass"])).max())))
    assert (err <= 4 * EPS * ref["v_mass"]).all()
    assert torch.equal(_bits(out[..., 3]), _bits(v[..., 3]))
    gerr = np.abs(grad[1].astype(np.float64) - ref["v_m"])
    print("backward %dx%d: |v_m - ref| / (2^-24 S_k) =" % (w, h), np.round(gerr / (EPS * ref["S"]), 3))
    bound = 3 * EPS * ref["S"]
    bound[3::4] = 2 * EPS * ref["S"][3::4]   # the offset column has no product to round
    assert (gerr <= bound).all(), gerr / (EPS * ref["S"])
    assert not grad[0].any() and not grad[2].any()
    assert np.array_equal(tab.params[1], c["m"])   # update = False leaves the row alone
    # the same inputs give the same bits, in place equals out of place, the identity returns v' unchanged
    again = tab.backward(2, x, v)
    assert torch.equal(_bits(again), _bits(out)) and np.array_equal(tab.grads.view(np.int32), grad.view(np.int32))
    inplace = v.clone()
    assert tab.backward(2, x, inplace, out=inplace) is inplace
    assert torch.equal(_bits(inplace), _bits(out)) and np.array_equal(tab.grads.view(np.int32), grad.view(np.int32))
    assert torch.equal(tab.backward(1, x, v), v)


def test_adam_step_by_step(ctx, dev):
    """Five updates of row 2.  The parameter check is fed the device's own prior state and the f64 value of the device's f32 grad,
    and allows 2^-23 max(|param|, lr): the device steps on the f64 sum, the reference on its f32 rounding.  The moments are held
    to 1e-12 relative, which the f32 rounding of grad (6e-8) cannot meet: for them the reference steps on exposure_ref's own f64
    v_m of the same inputs, which is the device's sum up to its order (256 terms of one sign pattern: below 3e-14 of S_k, and
    S_k / |g_k| < 4 for these inputs, asserted)."""
    w = h = 16
    lr = 0.01
    rng = np.random.default_rng(77)
    tab = _table(ctx, _case(w, h)["m"], lr=lr)
    x_np = _case(w, h)["x"]
    x = torch.from_numpy(x_np).to(dev)
    for step in range(5):
        v_np = (rng.uniform(-1.0, 1.0, (h, w, 4)) + 0.5).astype(np.float32)
        p_all, g_all = tab.params, tab.grads
        states = [tab.state(k) for k in (1, 2, 3)]
        m1, m2, t = states[1]
        assert t == step
        tab.backward(2, x, torch.from_numpy(v_np).to(dev), update=True)
        grad, param = tab.grads[1], tab.params[1]
        ref64 = er.backward(p_all[1], x_np, v_np)
        assert (np.abs(grad) >= 1e-3).all() and (ref64["S"] < 4 * np.abs(ref64["v_m"])).all()
        want, _, _, _ = er.adam_step(p_all[1], m1, m2, t, grad.astype(np.float64), lr)
        tol = 2.0 ** -23 * np.maximum(np.abs(param), lr)
        print("adam step %d: max |param - ref| / tol = %.3f" % (step + 1, float((np.abs(param - want) / tol).max())))
        assert (np.abs(param - want) <= tol).all()
        _, w1, w2, wt = er.adam_step(p_all[1], m1, m2, t, ref64["v_m"], lr)
        n1, n2, nt = tab.state(2)
        assert nt == wt == step + 1
        assert (np.abs(n1 - w1) <= 1e-12 * np.abs(w1)).all() and (np.abs(n2 - w2) <= 1e-12 * np.abs(w2)).all()
        # every other row stays bit for bit untouched
        p_new, g_new = tab.params, tab.grads
        for k in (0, 2):
            assert np.array_equal(p_new[k].view(np.int32), p_all[k].view(np.int32)) and np.array_equal(g_new[k].view(np.int32), g_all[k].view(np.int32))
            s = tab.state(k + 1)
            assert np.array_equal(s[0], states[k][0]) and np.array_equal(s[1], states[k][1]) and s[2] == states[k][2] == 0
    # lr = 0: the row stays, its moments and count advance
    tab.set_lr(0.0)
    before, (m1, _, t) = tab.params, tab.state(2)
    tab.backward(2, x, torch.from_numpy(v_np).to(dev), update=True)
    assert np.array_equal(tab.params.view(np.int32), before.view(np.int32))
    n1, _, nt = tab.state(2)
    assert nt == t + 1 and not np.array_equal(n1, m1)


def _rendered_image(ctx, dev, w=64, h=48):
    import brush_amd as ba
    from brush_amd import synth
    import util
    sc = synth.make_scene(3000, 0x3E, sh_degree=1, log_scale_range=(math.log(0.05), math.log(0.4)),
                          tan_half_fov=(math.tan(math.radians(50)), math.tan(math.radians(50))))
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    img, _ = ba.render_splats(spl, util.hip_camera(ba, synth.default_camera_params(w, h)), (w, h), (0.1, 0.2, 0.3),
                              pass_=ba.RasterPass.Backward, ctx=ctx)
    return img


def test_recovery_of_a_known_transform(ctx, dev):
    """y* = M* x on a rendered frame, mean squared error, v' formed with torch on the device, bh_exposure_backward(update = 1).
    The float64 loop of exposure_ref.recovery on the oracle's render of this scene brings max |m - M*| from 0.3 to 2.11e-3 in
    RECOVERY_ITERS updates at RECOVERY_LR (a factor of 142; at least 20 was asked of the settings); the GPU is asked for half the
    factor that was asked, 10: the problem is a convex least-squares fit, the margin covers f32 parameters only."""
    x = _rendered_image(ctx, dev)
    assert x.shape == (48, 64, 4) and float(x[..., :3].std()) > 0.05
    tab = _table(ctx, None, views=2, lr=er.RECOVERY_LR)
    a = torch.tensor(er.M_STAR.reshape(3, 4), dtype=torch.float32, device=dev)
    target = x[..., :3] @ a[:, :3].T + a[:, 3]
    v = torch.zeros_like(x)
    y = torch.empty_like(x)
    start = float(np.abs(tab.params[0].astype(np.float64) - er.M_STAR).max())
    for _ in range(er.RECOVERY_ITERS):
        tab.apply(1, x, out=y)
        v[..., :3] = (y[..., :3] - target) * (2.0 / target.numel())
        tab.backward(1, x, v, update=True, out=v)
    end = float(np.abs(tab.params[0].astype(np.float64) - er.M_STAR).max())
    print("recovery: max |m - M*| %.4f -> %.3e" % (start, end))
    assert abs(start - 0.3) < 1e-6 and end <= start / 10.0
    assert np.array_equal(tab.params[1], er.IDENTITY.astype(np.float32)) and tab.state(1)[2] == er.RECOVERY_ITERS


def test_errors_change_nothing(ctx, dev):
    import brush_amd as ba
    lib = ctx.lib
    c = _case(16, 16)
    tab = _table(ctx, c["m"])
    x, v = torch.from_numpy(c["x"]).to(dev), torch.from_numpy(c["v"]).to(dev)
    out = torch.full_like(x, -7.0)
    tab.backward(2, x, v, update=True)
    before = (tab.params.copy(), tab.grads.copy(), [tab.state(k) for k in (1, 2, 3)])
    px, pv, po = x.data_ptr(), v.data_ptr(), out.data_ptr()
    bad = [
        lib.bh_exposure_apply(ctx._h, tab._h, 0, px, 16, 16, po), lib.bh_exposure_apply(ctx._h, tab._h, 4, px, 16, 16, po),
        lib.bh_exposure_apply(ctx._h, tab._h, 2, px, 0, 16, po), lib.bh_exposure_apply(ctx._h, tab._h, 2, px, 16, 0, po),
        lib.bh_exposure_apply(ctx._h, tab._h, 2, None, 16, 16, po), lib.bh_exposure_apply(ctx._h, tab._h, 2, px, 16, 16, None),
        lib.bh_exposure_apply(ctx._h, None, 2, px, 16, 16, po),
        lib.bh_exposure_backward(ctx._h, tab._h, 0, px, pv, 16, 16, po, 1), lib.bh_exposure_backward(ctx._h, tab._h, 4, px, pv, 16, 16, po, 1),
        lib.bh_exposure_backward(ctx._h, tab._h, 2, px, pv, 0, 16, po, 1), lib.bh_exposure_backward(ctx._h, tab._h, 2, px, pv, 16, 0, po, 1),
        lib.bh_exposure_backward(ctx._h, tab._h, 2, None, pv, 16, 16, po, 1), lib.bh_exposure_backward(ctx._h, tab._h, 2, px, None, 16, 16, po, 1),
        lib.bh_exposure_backward(ctx._h, tab._h, 2, px, pv, 16, 16, None, 1),
        lib.bh_exposure_get_params(ctx._h, tab._h, 3, 2, before[0].ctypes.data_as(C.POINTER(C.c_float))),
        lib.bh_exposure_get_params(ctx._h, tab._h, 1, 3, None), lib.bh_exposure_set_params(ctx._h, tab._h, 0, 1, before[0].ctypes.data_as(C.POINTER(C.c_float))),
        lib.bh_exposure_get_state(ctx._h, tab._h, 4, None, None, None), lib.bh_exposure_set_adam(ctx._h, tab._h, -1.0, 0.9, 0.999, 1e-8),
        lib.bh_exposure_create(ctx._h, 0, C.byref(C.c_void_p())), lib.bh_train_set_exposure(ctx._h, C.c_void_p(12345)),
    ]
    assert bad == [-1] * len(bad), bad
    assert "exposure" in lib.bh_last_error(ctx._h).decode()
    ctx.sync()
    assert torch.equal(out, torch.full_like(x, -7.0))
    after = (tab.params, tab.grads, [tab.state(k) for k in (1, 2, 3)])
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    for s0, s1 in zip(before[2], after[2]):
        assert np.array_equal(s0[0], s1[0]) and np.array_equal(s0[1], s1[1]) and s0[2] == s1[2]
    # a handle of the other kind of per-view table is a stranger to either kind's entry points
    import util
    util.assert_wrong_kind_handles_refused(ba, ctx)
    # the setters have taken their values when they return: the caller's arrays may change or die at once
    two = _table(ctx, views=2)
    want = [0.5 + k for k in range(12)]
    src = list(want)
    two.set_view(2, src)
    src[:] = [-1.0] * 12
    del src
    assert np.array_equal(two.params[1], np.asarray(want, np.float32)) and np.array_equal(two.params[0], er.IDENTITY.astype(np.float32))
    m1, m2 = np.arange(12, dtype=np.float64) + 0.125, np.arange(12, dtype=np.float64) + 100.0
    a, b = m1.copy(), m2.copy()
    two.set_state(2, a, b, 7)
    a[:] = -1.0
    b[:] = -2.0
    del a, b
    s = two.state(2)
    assert np.array_equal(s[0], m1) and np.array_equal(s[1], m2) and s[2] == 7 and two.state(1)[2] == 0


def test_step_errors_and_destroying_an_attached_table(ctx, dev):
    """A step with view_id 0, with view_id > V or with a tile-row window fails with BH_ERR_INVALID_ARG before anything is queued
    (splats, optimizer state, step count and the table are as they were); destroying the attached table detaches it and the next
    step runs plain."""
    import brush_amd as ba
    from brush_amd import synth
    import util
    w, h = 64, 48
    sc = synth.make_scene(300, 0x3E, sh_degree=1, log_scale_range=(math.log(0.05), math.log(0.4)),
                          tan_half_fov=(math.tan(math.radians(50)), math.tan(math.radians(50))))
    cp = synth.default_camera_params(w, h)
    cam = util.hip_camera(ba, cp)
    gt = torch.from_numpy(np.ascontiguousarray(synth.synthetic_gt_packed(w, h)).view(np.int32)).to(dev)
    spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
    tab = _table(ctx, _case(16, 16)["m"], views=2)
    tr = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=3.0, ctx=ctx, exposure=tab)
    tr.step(ba.SceneBatch(gt, cam, view_id=2), spl)
    ctx.sync()
    snap = [spl.transforms.clone(), spl.sh_coeffs.clone(), spl.raw_opacities.clone()] + [v.clone() for v in tr.state.values()]
    p0, g0, s0 = tab.params, tab.grads, tab.state(2)
    assert s0[2] == 1 and g0[1].any()
    windowed = cam.uniforms((w, h), tile_rows=(0, 2))   # two of the frame's three tile rows
    for batch in (ba.SceneBatch(gt, cam, view_id=0), ba.SceneBatch(gt, cam, view_id=3), ba.SceneBatch(gt, windowed, view_id=2)):
        with pytest.raises(ba.BrushHipError, match="error -1"):
            tr.step(batch, spl)
        assert tr.step_count == 1
    ctx.sync()
    now = [spl.transforms, spl.sh_coeffs, spl.raw_opacities] + list(tr.state.values())
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(snap, now))
    assert np.array_equal(tab.params, p0) and np.array_equal(tab.grads, g0) and tab.state(2)[2] == 1
    # attached by hand, then destroyed: the step after runs plain (view_id 0 would otherwise be refused)
    ctx.check(ctx.lib.bh_train_set_exposure(ctx._h, tab._h))
    tab.close()
    plain = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=3.0, ctx=ctx)
    _, st = plain.step(ba.SceneBatch(gt, cam, view_id=0), spl)
    ctx.sync()
    assert math.isfinite(st.loss)
