"""Environment maps on the GPU (include/brush_hip_envmap.h) against tests/envmap_ref.py, bit for bit: composite,
the gradient to the frame, the integer gradient to the table, the device Adam step by step, state round trips and the refusals.

Shapes: 64x48 at R = 1, 2, 4, 8 (the clamp, the cube corner, the face edges, and many pixels per texel: the block's reduction by
destination, with its wave-wide fast path where a wave's pixels share a texel and the hash table where they do not); 17x13 at R = 4
(partial tiles, odd sizes); 16x16 at R = 64 (every pixel has texels of its own: more distinct texels in the one tile than its table's
probe limit finds room for, so some contributions go straight to memory); and 64x48 at 10 degrees looking into one face at R = 2, where
every pixel of the frame lands in one texel.  Alpha is random with 30 % of the pixels exactly 1."""
import ctypes as C

import numpy as np
import pytest
import torch

import envmap_ref as vr

pytestmark = pytest.mark.gpu
# (name, w, h, R, fov in degrees, direction)
CASES = (("r1", 64, 48, 1, 100.0, (1.0, 1.0, 1.0)), ("r2", 64, 48, 2, 100.0, (1.0, 1.0, 1.0)), ("r4", 64, 48, 4, 100.0, (1.0, 1.0, 1.0)),
         ("r8", 64, 48, 8, 100.0, (1.0, 1.0, 1.0)), ("odd", 17, 13, 4, 100.0, (1.0, 1.0, 1.0)), ("own", 16, 16, 64, 100.0, (1.0, 1.0, 1.0)),
         ("one", 64, 48, 2, 10.0, (1.0, 0.7, 0.7)))
_CASES = {}


def _case(name):
    """Seeded inputs and their restatement, computed once per case and shared (never modified)."""
    if name not in _CASES:
        _, w, h, res, fov, direction = next(c for c in CASES if c[0] == name)
        c = vr.scene(res, w, h, fov, seed=1, direction=direction)
        c.update(out=vr.composite(c["table"], c["img"], c["cam"]), bwd=vr.backward(c["table"], c["img"], c["v"], c["cam"]))
        for a in list(c.values()) + list(c["bwd"].values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CASES[name] = c
    return _CASES[name]


def bh_camera(cam, w, h):
    from brush_amd import _ffi
    c = _ffi.BhCamera()
    for i in range(12):
        c.vm[i] = float(cam["vm"][i])
    c.fx, c.fy, c.cx, c.cy = float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"])
    c.img_w, c.img_h, c.tile_row_end, c.model = w, h, (h + 15) // 16, _ffi.CAMERA_PINHOLE
    return c


@pytest.fixture
def ctx(dev):
    import brush_amd as ba
    c = ba.Context(dev)
    yield c
    c.close()


def _map(ctx, c, lr=1e-3):
    import brush_amd as ba
    m = ba.EnvironmentMap(c["res"], lr=lr, ctx=ctx)
    m.params = c["table"]
    return m


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))


def test_the_cases_are_what_they_claim():
    assert int(_case("one")["bwd"]["touched"].sum()) == 1
    assert set(np.flatnonzero(_case("r8")["bwd"]["touched"].reshape(6, -1).any(1)).tolist()) == {0, 2, 4}
    own = _case("own")["bwd"]
    assert int(own["touched"].sum()) > 512          # more distinct texels in the one tile than the tile's table has entries
    assert int(_case("r1")["bwd"]["count"].max()) > 256   # many pixels per texel, over several tiles
    for name in ("r1", "r8", "odd"):
        a = _case(name)["img"][..., 3]
        assert 0.2 < (a == 1).mean() < 0.4


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_composite_and_backward_equal_the_restatement_in_every_bit(ctx, dev, name):
    c = _case(name)
    w, h = c["w"], c["h"]
    cam = bh_camera(c["cam"], w, h)
    m = _map(ctx, c)
    assert _same(m.params, c["table"]) and not m.grads.any()
    img, v = torch.from_numpy(c["img"]).to(dev), torch.from_numpy(c["v"]).to(dev)
    out = m.composite(img, cam)
    assert _same(out.cpu().numpy(), c["out"])
    inplace = img.clone()
    assert m.composite(inplace, cam, out=inplace) is inplace and torch.equal(_bits(inplace), _bits(out))

    ref = c["bwd"]
    v_img = m.backward(img, cam, v)
    grad = m.grads
    assert _same(v_img.cpu().numpy(), ref["v_img"])
    diff = grad.view(np.int32) != ref["v_E"].view(np.int32)
    assert not diff.any(), "%d of %d gradient words differ, max |d| = %g" % (int(diff.sum()), diff.size, float(np.abs(grad - ref["v_E"]).max()))
    assert not grad[~ref["touched"]].any() and not np.signbit(grad[~ref["touched"]]).any()
    assert _same(m.params, c["table"])               # update = False leaves the table alone
    assert m.state()[2] == 0
    # the same inputs give the same bits, in place equals out of place
    again = m.backward(img, cam, v)
    assert torch.equal(_bits(again), _bits(v_img)) and _same(m.grads, grad)
    vin = v.clone()
    assert m.backward(img, cam, vin, out=vin) is vin
    assert torch.equal(_bits(vin), _bits(v_img)) and _same(m.grads, grad)


def test_zero_cotangent_gives_a_zero_gradient(ctx, dev):
    c = _case("r4")
    cam = bh_camera(c["cam"], c["w"], c["h"])
    m = _map(ctx, c)
    img, v = torch.from_numpy(c["img"]).to(dev), torch.from_numpy(c["v"]).to(dev)
    m.backward(img, cam, v)
    assert m.grads.any()
    z = torch.zeros_like(v)
    z[..., 3] = v[..., 3]                              # (alpha's cotangent is not the table's business)
    out = m.backward(img, cam, z)
    g = m.grads
    assert not g.any() and not np.isnan(g).any() and not np.signbit(g).any()
    assert torch.equal(_bits(out), _bits(z))           # the sky's term is (float)(0 E) = 0


def test_a_cotangent_that_is_not_finite_is_refused_and_nothing_is_touched(ctx, dev):
    import brush_amd as ba
    c = _case("r4")
    cam = bh_camera(c["cam"], c["w"], c["h"])
    m = _map(ctx, c, lr=0.01)
    img, v = torch.from_numpy(c["img"]).to(dev), torch.from_numpy(c["v"]).to(dev)
    m.backward(img, cam, v, update=True)
    before = (m.params, m.grads) + m.state()
    for bad_value in (float("inf"), float("nan")):
        bad = v.clone()
        bad[7, 9, 1] = bad_value
        out = torch.full_like(v, 7.0)
        with pytest.raises(ba.BrushHipError, match="NaN or an infinity"):
            m.backward(img, cam, bad, update=True, out=out)
        after = (m.params, m.grads) + m.state()
        assert all(_same(a, b) for a, b in zip(before[:4], after[:4])) and before[4] == after[4] == 1
        assert bool((out == 7.0).all())
    bad = v.clone()
    bad[7, 9, 3] = float("inf")                        # alpha's cotangent does not reach the table: not refused
    m.backward(img, cam, bad)
    assert _same(m.grads, c["bwd"]["v_E"])


def test_adam_steps_equal_numpy_f32_adam_to_the_bit(ctx, dev):
    c = _case("r8")
    cam = bh_camera(c["cam"], c["w"], c["h"])
    lr = 0.01
    m = _map(ctx, c, lr=lr)
    img, v = torch.from_numpy(c["img"]).to(dev), torch.from_numpy(c["v"]).to(dev)
    g = c["bwd"]["v_E"]
    untouched = ~c["bwd"]["touched"]
    p, m1, m2, t = c["table"], np.zeros_like(g), np.zeros_like(g), 0
    for step in range(4):
        if step == 2:
            m.set_lr(0.003)
            lr = 0.003
        m.backward(img, cam, v, update=True)
        p, m1, m2, t = vr.adam_step(p, m1, m2, t, g, lr)
        got_p, (got_m1, got_m2, got_t) = m.params, m.state()
        assert got_t == t == step + 1
        assert _same(m.grads, g)                       # v_E does not depend on the table
        assert _same(got_m1, m1) and _same(got_m2, m2), "moments differ at step %d" % (step + 1)
        bad = got_p.view(np.int32) != p.view(np.int32)
        assert not bad.any(), "step %d: %d texel words differ, max |d| = %g" % (step + 1, int(bad.sum()), float(np.abs(got_p - p).max()))
        assert _same(got_p[untouched], c["table"][untouched]) and untouched.any()
    m.set_lr(0.0)                                      # lr = 0: the table keeps its bits, moments and count advance
    m.backward(img, cam, v, update=True)
    assert _same(m.params, p) and m.state()[2] == 5 and not _same(m.state()[0], m1)


def test_state_round_trips_and_resumes(ctx, dev):
    import brush_amd as ba
    c = _case("r4")
    cam = bh_camera(c["cam"], c["w"], c["h"])
    a = _map(ctx, c, lr=0.01)
    img, v = torch.from_numpy(c["img"]).to(dev), torch.from_numpy(c["v"]).to(dev)
    for _ in range(2):
        a.backward(img, cam, v, update=True)
    m1, m2, t = a.state()
    assert t == 2 and m1.any() and m2.any()
    b = ba.EnvironmentMap(c["res"], lr=0.01, ctx=ctx)
    b.params = a.params
    b.set_state(m1, m2, t)
    s = b.state()
    assert _same(s[0], m1) and _same(s[1], m2) and s[2] == 2
    a.backward(img, cam, v, update=True)
    b.backward(img, cam, v, update=True)
    assert _same(a.params, b.params) and all(_same(x, y) for x, y in zip(a.state()[:2], b.state()[:2])) and a.state()[2] == b.state()[2] == 3
    b.close()
    b.close()


def test_refusals(ctx, dev):
    import brush_amd as ba
    from brush_amd import _ffi
    lib, h = ctx.lib, ctx._h
    for res in (0, 1025):
        with pytest.raises(ba.BrushHipError, match="resolution"):
            ba.EnvironmentMap(res, ctx=ctx)
    c = _case("r4")
    m = _map(ctx, c)
    with pytest.raises(ValueError):
        m.params = np.zeros((6, 4, 4, 4), np.float32)
    img, v = torch.from_numpy(c["img"]).to(dev), torch.from_numpy(c["v"]).to(dev)
    fish = bh_camera(c["cam"], c["w"], c["h"])
    fish.model = _ffi.CAMERA_KANNALA_BRANDT_4
    with pytest.raises(ba.BrushHipError, match="pinhole"):
        m.composite(img, fish)
    with pytest.raises(ba.BrushHipError, match="pinhole"):
        m.backward(img, fish, v)
    cam = bh_camera(c["cam"], c["w"], c["h"])
    assert lib.bh_envmap_composite(h, m._h, C.byref(cam), None, 48, 64, None) == -1
    assert lib.bh_envmap_composite(h, m._h, C.byref(cam), img.data_ptr(), 0, 64, img.data_ptr()) == -1
    assert lib.bh_envmap_composite(h, m._h, None, img.data_ptr(), 48, 64, img.data_ptr()) == -1
    assert lib.bh_envmap_set_adam(h, m._h, -1.0, 0.9, 0.999, 1e-15) == -1 and lib.bh_envmap_set_adam(h, m._h, 1e-3, 1.0, 0.999, 1e-15) == -1
    other = ba.Context(dev)
    try:
        assert lib.bh_envmap_composite(other._h, m._h, C.byref(cam), img.data_ptr(), 48, 64, img.data_ptr()) == -1   # another context's map
        assert lib.bh_train_set_envmap(other._h, m._h) == -1
    finally:
        other.close()
    assert lib.bh_train_set_envmap(h, m._h) == 0
    m.close()                                           # destroying an attached map detaches it
    assert lib.bh_train_set_envmap(h, None) == 0
    assert _same(vr.composite(c["table"], c["img"], c["cam"]), c["out"])   # the shared case is as it was


def test_a_handle_of_another_kind_of_table_is_a_stranger(ctx):
    import brush_amd as ba
    import util
    util.assert_wrong_kind_handles_refused(ba, ctx)


def test_closing_the_context_frees_tables_of_every_kind(dev):
    """bh_destroy frees what is left on the ctx's one list of tables — the device's free memory says so: the three tables are about
    75 MB each (no image, no kernel beyond the fills of their creation), so one of them left behind is a third of the total, against
    a tenth allowed for whatever else moves on the device — and a table's own close() then must not touch the library."""
    import brush_amd as ba
    torch.cuda.synchronize(dev)
    before = torch.cuda.mem_get_info(dev)[0]
    c = ba.Context(dev)
    tables = (ba.ExposureTable(1 << 18, ctx=c), ba.BilateralGridTable(192, grid=(16, 16, 8), ctx=c), ba.EnvironmentMap(416, ctx=c))
    total = (1 << 18) * (12 * (2 * 8 + 8) + 4) + 192 * ((16 * 16 * 8 * 12) * (2 * 4 + 8) + 4) + 6 * 416 * 416 * 3 * (8 + 2 * 4 + 8)
    assert before - torch.cuda.mem_get_info(dev)[0] >= 0.9 * total
    assert c.lib.bh_train_set_envmap(c._h, tables[2]._h) == 0   # (attached ones included)

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError("close() of a table whose context is closed called %s" % name)

    c.close()
    assert before - torch.cuda.mem_get_info(dev)[0] <= 0.1 * total
    for t in tables:
        t.lib = NoLibrary()
        t.close()
        assert t._h is None
        t.close()


def test_a_new_map_is_black_and_a_new_colour_row_the_identity(ctx):
    """The row pattern a kind hands to the table core: none for a map, at row lengths (18, 162) that are no multiple of twelve, and
    the 3x4 identity for the colour tables, over every view and cell."""
    import brush_amd as ba
    for res in (1, 3):
        m = ba.EnvironmentMap(res, ctx=ctx)
        assert m.shape == (6, res, res, 3) and m.params.shape == m.shape
        m1, m2, t = m.state()
        for a in (m.params, m.grads, m1, m2):
            assert a.shape == m.shape and a.dtype == np.float32 and not a.view(np.int32).any()
        assert t == 0
        m.close()
    ident = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    grid, exp = ba.BilateralGridTable(3, grid=(2, 2, 2), ctx=ctx), ba.ExposureTable(3, ctx=ctx)
    assert grid.params.shape == (3, 2, 2, 2, 12) and exp.params.shape == (3, 12)
    for tab in (grid, exp):
        p = tab.params.reshape(-1, 12)
        assert _same(p, np.tile(ident, (p.shape[0], 1)))
        assert not tab.grads.any()
        for view in (1, 3):
            m1, m2, t = tab.state(view)
            assert not m1.any() and not m2.any() and t == 0
        tab.close()
