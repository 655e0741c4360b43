"""Per-view bilateral grids on the GPU (include/brush_hip_bilagrid.h) against tests/bilagrid_ref.py with float32
coordinates: slice, backward, total variation, the device Adam step by step, the recovery of a known grid, and the errors.

Sizes (w, h): 5x3 (fewer pixels than a wave and fewer than the grid has vertices: most vertices must be exact zeros), 16x16, 123x82
(ragged), and 1025x512 = 524,800 pixels: one pass of the per-pixel kernels' capped grid (BG_PIXEL_MAX_BLOCKS 2048 blocks x 256 lanes =
524,288) plus a ragged remainder, and cells of 69x35 = 2,415 pixels, past BG_UNIT_PIXELS = 2,048, so the v_g pass cuts every cell into
two bands.  Grids (Wg, Hg, L): the default (16,16,8); (3,4,2), which catches swapped axes; (5,6,1), no guidance axis; (1,1,3), no xy
axes (one cell of 10,086 pixels at 123x82: five bands).  Every grid meets the ragged size, every size the default grid.

Bounds: |y - ref| <= K 2^-24 mass_y, |v_img - ref| <= K 2^-24 mass_v, |v_g - ref| <= K_G 2^-24 S, the masses as bilagrid_ref returns
them.  K and K_G are the next power of two at or above twice the largest ratio measured on the MI355X over all cases (the tests print
every case's ratio): y 3.715 and v_img 3.243 give K = 8 (the nested interpolation, three roundings deep, then the four-term chain),
v_g 0.998 gives K_G = 2 (the sum is f64 throughout: what is left is the one rounding into f32, at most 1 by construction)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bilagrid_ref as br

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
MEASURED_Y, MEASURED_V, MEASURED_G = 3.715, 3.243, 0.998   # largest ratios measured on the MI355X (slice 1025x512; v_img 123x82 on (3,4,2); v_g 16x16)
K, K_G = 8, 2
DEFAULT = (16, 16, 8)
BIG = (1025, 512)
CASES = [((5, 3), DEFAULT), ((16, 16), DEFAULT), ((123, 82), DEFAULT), (BIG, DEFAULT),
         ((123, 82), (3, 4, 2)), ((123, 82), (5, 6, 1)), ((123, 82), (1, 1, 3))]   # ((w, h), (Wg, Hg, L))
_CASES = {}


def _shape(grid):
    return (grid[1], grid[0], grid[2])   # (Wg, Hg, L) -> the row's (Hg, Wg, L)


def _case(size, grid):
    """Seeded inputs and their reference with float32 coordinates, computed once per case and shared (never modified)."""
    key = (size, grid)
    if key not in _CASES:
        w, h = size
        x, v, g = br.case_inputs(w, h, _shape(grid), 1000 * w + h + 7 * grid[0] + grid[2])
        c = dict(x=x, v=v, g=g, fwd=br.slice_grid(g, x), bwd=br.backward(g, x, v))
        for d in (c, c["fwd"], c["bwd"]):
            for a in d.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _CASES[key] = c
    return _CASES[key]


@pytest.fixture
def ctx(dev):
    import brush_amd as ba
    c = ba.Context(dev)
    yield c
    c.close()


def _table(ctx, grid, g=None, views=3, lr=2e-3):
    import brush_amd as ba
    tab = ba.BilateralGridTable(views, grid=grid, lr=lr, ctx=ctx)
    if g is not None:
        tab.set_view(2, g)
    return tab


def _bits(t):
    return t.contiguous().view(torch.int32)


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)   # (a copy: the shared case arrays are read-only)


@pytest.mark.parametrize("size,grid", CASES)
def test_slice(ctx, dev, size, grid):
    c = _case(size, grid)
    tab = _table(ctx, grid, c["g"])
    x = _dev(c["x"], dev)
    y = tab.slice(2, x)
    got = y.cpu().numpy().astype(np.float64)
    err = np.abs(got[..., :3] - c["fwd"]["y"][..., :3])
    ratio = float((err / (EPS * c["fwd"]["mass_y"])).max())
    print("slice %dx%d grid %s: max |y - ref| / (2^-24 mass) = %.3f (bound %d)" % (size + (grid, ratio, K)))
    assert (err <= K * EPS * c["fwd"]["mass_y"]).all(), ratio
    assert torch.equal(_bits(y[..., 3]), _bits(x[..., 3]))
    assert torch.equal(_bits(tab.slice(1, x)), _bits(x))   # view 1 is still the identity grid
    inplace = x.clone()
    assert tab.slice(2, inplace, out=inplace) is inplace
    assert torch.equal(_bits(inplace), _bits(y))


@pytest.mark.parametrize("size,grid", CASES)
def test_backward(ctx, dev, size, grid):
    c = _case(size, grid)
    ref = c["bwd"]
    tab = _table(ctx, grid, c["g"])
    x, v = _dev(c["x"], dev), _dev(c["v"], dev)
    out = tab.backward(2, x, v)
    got = out.cpu().numpy().astype(np.float64)
    err = np.abs(got[..., :3] - ref["v_img"][..., :3])
    ratio_v = float((err / (EPS * ref["mass_v"])).max())
    grads = tab.grads
    vg = grads[1].astype(np.float64)
    dead = ref["S"] == 0
    err_g = np.abs(vg - ref["v_g"])
    ratio_g = float((err_g[~dead] / (EPS * ref["S"][~dead])).max())
    print("backward %dx%d grid %s: max |v_img - ref| / (2^-24 mass) = %.3f (bound %d), max |v_g - ref| / (2^-24 S) = %.3f (bound %d), "
          "%d of %d vertices unreached" % (size + (grid, ratio_v, K, ratio_g, K_G, int((~ref["reached"]).sum()), ref["reached"].size)))
    assert (err <= K * EPS * ref["mass_v"]).all(), ratio_v
    assert (err_g <= K_G * EPS * ref["S"]).all(), ratio_g
    assert (grads[1][dead].view(np.int32) == 0).all()   # exact zeros, whatever the scratch held
    if size == (5, 3) and grid == DEFAULT:
        assert (~ref["reached"]).sum() > ref["reached"].size // 2
    assert torch.equal(_bits(out[..., 3]), _bits(v[..., 3]))
    assert not grads[0].any() and not grads[2].any()
    # a second call gives the same bits, in place equals out of place, update=False left the grid alone
    again = tab.backward(2, x, v)
    assert torch.equal(_bits(again), _bits(out)) and np.array_equal(tab.grads.view(np.int32), grads.view(np.int32))
    inplace = v.clone()
    assert tab.backward(2, x, inplace, out=inplace) is inplace
    assert torch.equal(_bits(inplace), _bits(out)) and np.array_equal(tab.grads.view(np.int32), grads.view(np.int32))
    p = tab.params
    assert np.array_equal(p[1].view(np.int32), c["g"].view(np.int32)) and tab.state(2)[2] == 0
    assert np.array_equal(p[0], br.identity_grid(*_shape(grid)).astype(np.float32)) and np.array_equal(p[0], p[2])


def test_identity_grid_returns_its_input(ctx, dev):
    rng = np.random.default_rng(21)
    x = torch.from_numpy(rng.uniform(0.02, 0.98, (82, 123, 4)).astype(np.float32)).to(dev)   # luminance strictly inside (0, 1)
    v = torch.from_numpy(rng.uniform(-1.0, 1.0, (82, 123, 4)).astype(np.float32)).to(dev)
    tab = _table(ctx, DEFAULT)
    assert torch.equal(_bits(tab.slice(3, x)), _bits(x))
    assert torch.equal(_bits(tab.backward(3, x, v)), _bits(v))
    wild = torch.from_numpy(rng.uniform(-0.2, 1.2, (82, 123, 4)).astype(np.float32)).to(dev)   # clamped luminances: x still comes back
    assert torch.equal(_bits(tab.slice(3, wild)), _bits(wild))


@pytest.mark.parametrize("grid", [DEFAULT, (3, 4, 2), (5, 6, 1), (1, 1, 3)])
def test_total_variation_and_its_gradient(ctx, dev, grid):
    c = _case((123, 82), grid)
    tab = _table(ctx, grid, c["g"])
    tv, tv_grad = br.total_variation(c["g"])
    got = float(tab.tv(2).cpu().numpy()[0])
    print("tv grid %s: %.9g, reference %.9g" % (grid, got, tv))
    assert tv > 0 and abs(got - tv) <= 1e-6 * tv
    assert float(tab.tv(1).cpu().numpy()[0]) == 0.0
    x, v = _dev(c["x"], dev), _dev(c["v"], dev)
    tab.backward(2, x, v, tv_weight=0.75)
    want = c["bwd"]["v_g"] + 0.75 * tv_grad
    bound = K_G * EPS * (c["bwd"]["S"] + 0.75 * np.abs(tv_grad))   # one rounding of a sum of at most this size
    got_g = tab.grads[1].astype(np.float64)
    assert (np.abs(got_g - want) <= bound).all()
    assert (np.abs(got_g - c["bwd"]["v_g"]) > bound).any()   # the term is there


def test_adam_step_by_step(ctx, dev):
    c = _case((16, 16), DEFAULT)
    lr = 0.01
    tab = _table(ctx, DEFAULT, c["g"], lr=lr)
    x, v = _dev(c["x"], dev), _dev(c["v"], dev)
    before_other = (tab.params[0].copy(), tab.params[2].copy())
    for step in range(1, 6):
        p0 = tab.params[1].astype(np.float64)
        m1, m2, t = tab.state(2)
        assert t == step - 1
        tab.backward(2, x, v, tv_weight=0.5, update=True)
        g = br.backward(p0, c["x"], c["v"])["v_g"] + 0.5 * br.total_variation(p0)[1]
        want_p, want_m1, want_m2, want_t = br.adam_step(p0, m1, m2, t, g, lr)
        p1 = tab.params[1].astype(np.float64)
        n1, n2, t1 = tab.state(2)
        assert t1 == want_t == step
        assert (np.abs(p1 - want_p) <= 2.0 ** -23 * np.maximum(np.abs(want_p), lr)).all()
        assert (np.abs(n1 - want_m1) <= 2.0 ** -23 * np.abs(want_m1) + 1e-30).all()
        assert (np.abs(n2 - want_m2) <= 2.0 ** -23 * np.abs(want_m2) + 1e-30).all()
        assert n1.dtype == np.float32 and np.abs(p1 - p0).max() > 0.5 * lr
    assert np.array_equal(tab.params[0], before_other[0]) and np.array_equal(tab.params[2], before_other[1])
    assert tab.state(1)[2] == 0 and tab.state(3)[2] == 0 and not tab.state(1)[0].any() and not tab.state(3)[1].any()


def test_lr_zero_keeps_the_grid_while_the_count_advances(ctx, dev):
    c = _case((16, 16), DEFAULT)
    tab = _table(ctx, DEFAULT, c["g"], lr=0.0)
    x, v = _dev(c["x"], dev), _dev(c["v"], dev)
    tab.backward(2, x, v, tv_weight=1.0, update=True)
    tab.backward(2, x, v, tv_weight=1.0, update=True)
    assert np.array_equal(tab.params[1].view(np.int32), c["g"].view(np.int32))
    m1, m2, t = tab.state(2)
    assert t == 2 and m1.any() and m2.any()


def test_recovers_a_known_smooth_grid(ctx, dev):
    """The target is x through a known smooth grid on a fixed 64x48 image; 300 Adam steps on the cotangent of the squared error."""
    import brush_amd as ba
    w, h = 64, 48
    rng = np.random.default_rng(64048)
    x_np = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float32)
    target = torch.from_numpy(br.slice_grid(br.smooth_grid(*_shape(DEFAULT)), x_np)["y"].astype(np.float32)).to(dev)
    x = torch.from_numpy(x_np).to(dev)
    tab = ba.BilateralGridTable(1, grid=DEFAULT, lr=0.01, ctx=ctx)
    y, v = torch.empty_like(x), torch.empty_like(x)
    residual = {}
    for step in range(301):
        tab.slice(1, x, out=y)
        torch.sub(y, target, out=v)
        v[..., 3] = 0.0
        if step in (0, 300):
            residual[step] = float((v * v).sum())
        if step < 300:
            tab.backward(1, x, v, update=True, out=v)
    print("recovery: squared residual %.4e -> %.4e after 300 steps" % (residual[0], residual[300]))
    assert residual[0] > 0 and residual[300] < 0.1 * residual[0]
    assert tab.state(1)[2] == 300


def test_errors(ctx, dev):
    import brush_amd as ba
    tab = _table(ctx, (3, 4, 2))
    x = torch.zeros((4, 5, 4), device=dev)
    before = tab.params.copy()
    for view in (0, 4):
        with pytest.raises(ba.BrushHipError, match="view out of range"):
            tab.slice(view, x)
        with pytest.raises(ba.BrushHipError, match="view out of range"):
            tab.backward(view, x, x)
        with pytest.raises(ba.BrushHipError, match="view out of range"):
            tab.tv(view)
        with pytest.raises(ba.BrushHipError, match="view out of range"):
            tab.state(view)
    lib, h, p = ctx.lib, ctx._h, x.data_ptr()
    assert lib.bh_bilagrid_slice(h, tab._h, 1, None, 4, 5, p) == -1 and lib.bh_bilagrid_slice(h, tab._h, 1, p, 4, 5, None) == -1
    assert lib.bh_bilagrid_slice(h, tab._h, 1, p, 0, 5, p) == -1 and lib.bh_bilagrid_slice(h, tab._h, 1, p, 4, 0, p) == -1
    assert lib.bh_bilagrid_backward(h, tab._h, 1, p, None, 4, 5, p, 0.0, 0) == -1 and lib.bh_bilagrid_backward(h, tab._h, 1, p, p, 0, 5, p, 0.0, 1) == -1
    assert lib.bh_bilagrid_backward(h, tab._h, 1, p, p, 4, 5, p, -1.0, 1) == -1
    assert lib.bh_bilagrid_tv(h, tab._h, 1, None) == -1 and lib.bh_bilagrid_slice(h, None, 1, p, 4, 5, p) == -1
    assert lib.bh_bilagrid_get_params(h, tab._h, 1, 1, None) == -1 and lib.bh_bilagrid_set_params(h, tab._h, 3, 2, before.ctypes.data_as(C.POINTER(C.c_float))) == -1
    assert lib.bh_bilagrid_set_adam(h, tab._h, -1.0, 0.9, 0.999, 1e-15) == -1 and lib.bh_bilagrid_set_adam(h, tab._h, 1e-3, 1.0, 0.999, 1e-15) == -1
    bad = C.c_void_p()
    for dims in ((0, 4, 2), (3, 0, 2), (3, 4, 0), (2048, 4, 2), (1024, 1024, 1)):
        assert lib.bh_bilagrid_create(h, 2, dims[0], dims[1], dims[2], C.byref(bad)) == -1 and not bad.value
    assert lib.bh_bilagrid_create(h, 0, 3, 4, 2, C.byref(bad)) == -1 and not bad.value
    w_, h_, l_, n_ = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert lib.bh_bilagrid_dims(h, tab._h, C.byref(n_), C.byref(w_), C.byref(h_), C.byref(l_)) == 0
    assert (n_.value, w_.value, h_.value, l_.value) == (3, 3, 4, 2)
    assert np.array_equal(tab.params, before) and tab.state(1)[2] == 0 and not tab.grads.any()
    other = ba.Context(dev)
    try:
        with pytest.raises(ba.BrushHipError, match="not a bilateral-grid table of this context"):
            other.check(other.lib.bh_train_set_bilagrid(other._h, tab._h, 1.0))
    finally:
        other.close()
    # ... and so is a handle of the other kind of per-view table on the same context
    import util
    util.assert_wrong_kind_handles_refused(ba, ctx)
    assert np.array_equal(tab.params, before) and tab.state(1)[2] == 0 and not tab.grads.any()
    tab.close()
    tab.close()


def test_gsplat_layout_round_trip(ctx, dev):
    c = _case((123, 82), (3, 4, 2))
    tab = _table(ctx, (3, 4, 2), c["g"])
    s = tab.to_gsplat()
    assert s.shape == (3, 12, 2, 4, 3) and np.array_equal(s[1], br.to_gsplat(c["g"]))
    other = _table(ctx, (3, 4, 2))
    other.from_gsplat(torch.from_numpy(s))
    assert np.array_equal(other.params, tab.params)
