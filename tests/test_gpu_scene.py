"""Scene editing on the GPU (include/brush_hip_scene.h): bh_splats_transform equals the float32 restatement of
tests/scene_ref.py bit for bit — every degree, tile boundaries, in place, unaligned base pointers — leaves rows alone that are not its
business, refuses overlapping outputs, and passes the end-to-end invariant (the transformed scene from the transformed camera is the
same image) on the scenes and by the criterion of the CPU test; bh_splats_select_region equals its restatement exactly, and crop_splats
returns the kept rows in source order."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import scene_ref as sr
import util

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 127, 129, 255, 256, 257, 1029]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    """Bit for bit, NaNs comparing as equal."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _scene(n, degree, seed):
    rng = np.random.default_rng(seed)
    tr = np.concatenate([rng.uniform(-4, 4, (n, 3)), rng.normal(size=(n, 4)), rng.uniform(-4, 0, (n, 3))], axis=1).astype(np.float32)
    sh = rng.uniform(-1, 1, (n, (degree + 1) ** 2, 3)).astype(np.float32)
    return tr, sh, rng.uniform(-2, 4, n).astype(np.float32), rng.uniform(0, 0.1, n).astype(np.float32)


def _transform(ba, seed=5):
    rng = np.random.default_rng(seed)
    return ba.SceneTransform.from_quat(rng.normal(size=4), rng.uniform(-3, 3, 3), math.exp(rng.uniform(-1, 1)))


@pytest.fixture(scope="module")
def ctx(dev):
    import brush_amd as ba
    c = ba.Context(dev)
    yield c
    c.close()


@pytest.mark.parametrize("degree", [0, 1, 2, 3, 4])
def test_transform_equals_the_restatement_bit_for_bit(dev, ctx, degree):
    import brush_amd as ba
    T = _transform(ba, 5 + degree)
    rec = sr.record_from_struct(T.as_struct())
    for n in SIZES:
        tr, sh, op, ms = _scene(n, degree, 31 * n + degree)
        want_tr, want_sh, want_ms = sr.transform_f32(rec, tr, sh, ms)
        for with_ms in (False, True):
            spl = ba.Splats(tr, sh, op, device=dev, min_scale=ms if with_ms else None)
            out = spl.transformed(T, ctx=ctx)
            assert _same(out.transforms.cpu().numpy(), want_tr), (n, "transforms")
            assert _same(out.sh_coeffs.cpu().numpy(), want_sh), (n, "sh")
            assert (out.min_scale is None) if not with_ms else _same(out.min_scale.cpu().numpy(), want_ms)
            assert _same(out.raw_opacities.cpu().numpy(), op) and _same(spl.transforms.cpu().numpy(), tr) and _same(spl.sh_coeffs.cpu().numpy(), sh)
            same = spl.transform_(T, ctx=ctx)   # in place
            assert same is spl and _same(spl.transforms.cpu().numpy(), want_tr) and _same(spl.sh_coeffs.cpu().numpy(), want_sh), (n, "in place")
            assert not with_ms or _same(spl.min_scale.cpu().numpy(), want_ms)
        # sh_coeffs = NULL: transforms alone, the SH output untouched
        t_in, t_out = torch.from_numpy(tr).to(dev), torch.full((n, 10), 7.0, device=dev)
        sh_out = torch.full(sh.shape, 7.0, device=dev)
        ctx.check(ctx.lib.bh_splats_transform(ctx._h, C.byref(T.as_struct()), n, sh.shape[1], t_in.data_ptr(), None, None, t_out.data_ptr(), sh_out.data_ptr(), None))
        assert _same(t_out.cpu().numpy(), want_tr) and bool((sh_out == 7.0).all())


@pytest.mark.parametrize("degree", [0, 1, 2, 3, 4])
def test_transform_with_base_pointers_off_by_one_float(dev, ctx, degree):
    """Raw pointers one float past an aligned allocation (nothing re-aligns them): the 4-byte path, out of place and in place, and the
    floats in front of and behind every buffer stay as they were."""
    import brush_amd as ba
    T = _transform(ba, 15 + degree)
    rec = sr.record_from_struct(T.as_struct())
    lib, h = ctx.lib, ctx._h
    for n in (1, 65, 257, 1029):
        tr, sh, _, ms = _scene(n, degree, 77 * n + degree)
        c = sh.shape[1]
        want_tr, want_sh, want_ms = sr.transform_f32(rec, tr, sh, ms)

        def padded(a):
            buf = torch.full((a.size + 2,), -9.0, device=dev)
            assert buf.data_ptr() % 16 == 0
            buf[1:-1] = torch.from_numpy(a.reshape(-1)).to(dev)
            return buf

        ins = [padded(tr), padded(sh), padded(ms)]
        outs = [torch.full_like(b, -9.0) for b in ins]
        ptr = [b.data_ptr() + 4 for b in ins + outs]
        ctx.check(lib.bh_splats_transform(h, C.byref(T.as_struct()), n, c, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], ptr[5]))
        for o, want in zip(outs, (want_tr, want_sh, want_ms)):
            got = o.cpu().numpy()
            assert got[0] == -9.0 and got[-1] == -9.0 and _same(got[1:-1], want.reshape(-1)), n
        ctx.check(lib.bh_splats_transform(h, C.byref(T.as_struct()), n, c, ptr[0], ptr[1], ptr[2], ptr[0], ptr[1], ptr[2]))   # in place
        for o, want in zip(ins, (want_tr, want_sh, want_ms)):
            got = o.cpu().numpy()
            assert got[0] == -9.0 and got[-1] == -9.0 and _same(got[1:-1], want.reshape(-1)), (n, "in place")
        # one side aligned, the other not
        al, off = torch.empty((n, 10), device=dev), padded(tr)
        ctx.check(lib.bh_splats_transform(h, C.byref(T.as_struct()), n, c, off.data_ptr() + 4, None, None, al.data_ptr(), None, None))
        assert _same(al.cpu().numpy(), want_tr)


def test_nothing_is_launched_for_an_empty_scene_and_bad_arguments_are_refused(dev, ctx):
    import brush_amd as ba
    T = _transform(ba)
    lib, h = ctx.lib, ctx._h
    assert lib.bh_splats_transform(h, C.byref(T.as_struct()), 0, 16, None, None, None, None, None, None) == 0
    assert lib.bh_splats_transform(h, C.byref(T.as_struct()), 0, 5, None, None, None, None, None, None) == -1
    empty = ba.Splats(np.zeros((0, 10), np.float32), np.zeros((0, 1, 3), np.float32), np.zeros(0, np.float32), device=dev)
    assert empty.transformed(T, ctx=ctx).num_splats() == 0
    t = torch.zeros((8, 10), device=dev)
    for coeffs in (0, 2, 3, 24, 26, 36):
        assert lib.bh_splats_transform(h, C.byref(T.as_struct()), 8, coeffs, t.data_ptr(), None, None, t.data_ptr(), None, None) == -1
    assert lib.bh_splats_transform(h, None, 8, 1, t.data_ptr(), None, None, t.data_ptr(), None, None) == -1
    assert lib.bh_splats_transform(h, C.byref(T.as_struct()), 8, 1, t.data_ptr(), None, None, None, None, None) == -1
    assert lib.bh_splats_transform(h, C.byref(T.as_struct()), 8, 1, t.data_ptr(), t.data_ptr(), None, t.data_ptr(), None, None) == -1   # SH without an output


def test_identity_returns_the_input_bits(dev, ctx):
    import brush_amd as ba
    n, degree = 300, 2
    tr, sh, op, ms = _scene(n, degree, 3)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-42], np.float32)   # (a denormal too)
    tr.reshape(-1)[::7] = np.resize(special, tr.reshape(-1)[::7].size)
    sh.reshape(-1)[::5] = np.resize(special, sh.reshape(-1)[::5].size)
    ms[::3] = np.resize(special, ms[::3].size)
    tr.reshape(-1)[3] = np.float32(np.uint32(0x7FC12345).view(np.float32))   # a NaN with a payload
    ident = ba.SceneTransform.from_quat((3.0, 0, 0, 0), (0, 0, 0), 1.0)
    spl = ba.Splats(tr, sh, op, device=dev, min_scale=ms)
    out = spl.transformed(ident, ctx=ctx)
    for got, want in ((out.transforms, tr), (out.sh_coeffs, sh), (out.min_scale, ms)):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    spl.transform_(ident, ctx=ctx)
    for got, want in ((spl.transforms, tr), (spl.sh_coeffs, sh), (spl.min_scale, ms)):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))


def test_non_finite_rows_disturb_no_other_row(dev, ctx):
    import brush_amd as ba
    n, degree = 300, 3
    T = _transform(ba, 9)
    rec = sr.record_from_struct(T.as_struct())
    tr, sh, op, ms = _scene(n, degree, 4)
    clean = sr.transform_f32(rec, tr, sh, ms)
    bad = (0, 64, n - 1)
    for k, r in enumerate(bad):
        tr[r], sh[r], ms[r] = (np.nan, np.inf, -np.inf)[k], (np.inf, np.nan, np.nan)[k], np.nan
    spl = ba.Splats(tr, sh, op, device=dev, min_scale=ms)
    for out in (spl.transformed(T, ctx=ctx), spl.transform_(T, ctx=ctx)):
        rows = np.setdiff1d(np.arange(n), bad)
        for got, want in zip((out.transforms, out.sh_coeffs, out.min_scale), clean):
            got = got.cpu().numpy()
            assert np.array_equal(_bits(got[rows]), _bits(want[rows]))
            assert not np.isfinite(got[list(bad)]).all()


def test_an_overlapping_output_is_refused_and_nothing_is_written(dev, ctx):
    import brush_amd as ba
    T = _transform(ba)
    lib, h = ctx.lib, ctx._h
    n = 100
    tr, sh, _, ms = _scene(n, 1, 6)
    buf = torch.from_numpy(np.concatenate([tr.reshape(-1), np.zeros(40, np.float32)])).to(dev)
    shb, msb = torch.from_numpy(sh).to(dev), torch.from_numpy(ms).to(dev)
    before = [b.clone() for b in (buf, shb, msb)]
    p, s, m = buf.data_ptr(), shb.data_ptr(), msb.data_ptr()
    spare = torch.zeros((n * 12,), device=dev)
    free = spare.data_ptr()
    calls = (
        (p, None, None, p + 40, None, None),     # shifted by one row
        (p, None, None, p + 4, None, None),      # ... by one float
        (p + 40, None, None, p, None, None),
        (p, s, None, free, s + 12, None),        # the SH output overlaps the SH input
        (p, s, None, s, free, None),             # an output over another input
        (p, s, m, free, s, s),                   # two outputs on the same memory
        (p, s, m, p, s, m + 4),
    )
    for a in calls:
        assert lib.bh_splats_transform(h, C.byref(T.as_struct()), n, 4, *a) == -1, a
        assert b"overlap" in lib.bh_last_error(h)
    ctx.sync()
    for b, was in zip((buf, shb, msb), before):
        assert torch.equal(b, was)
    # adjacent is not overlapping
    assert lib.bh_splats_transform(h, C.byref(T.as_struct()), 50, 4, p, None, None, p + 50 * 40, None, None) == 0


def test_transform_then_inverse_returns_the_means(dev, ctx):
    import brush_amd as ba
    T = _transform(ba, 12)
    tr, sh, op, ms = _scene(2000, 2, 8)
    spl = ba.Splats(tr, sh, op, device=dev, min_scale=ms)
    back = spl.transformed(T, ctx=ctx).transform_(T.inverse(), ctx=ctx)
    got = back.transforms.cpu().numpy()
    # (not bit-exact and not claimed to be): 1e-5 relative to the scene's extent
    assert np.abs(got[:, :3] - tr[:, :3]).max() <= 1e-5 * np.abs(tr[:, :3]).max()
    assert np.abs(got[:, 7:] - tr[:, 7:]).max() <= 1e-5 * np.abs(tr[:, 7:]).max()
    assert np.abs(back.min_scale.cpu().numpy() - ms).max() <= 1e-5 * ms.max()
    assert np.abs(back.sh_coeffs.cpu().numpy() - sh).max() <= 1e-5


@pytest.mark.parametrize("degree,mip,seed", sr.INVARIANT_CASES)
def test_transformed_scene_from_transformed_camera_is_the_same_image(dev, ctx, degree, mip, seed):
    import brush_amd as ba
    sc, (q, t, s) = sr.invariant_case(degree, seed)
    T = ba.SceneTransform.from_quat(q, t, s)
    cam = util.hip_camera(ba, sr.CAM)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], render_mip=bool(mip), device=dev)
    size = (sr.IMG_W, sr.IMG_H)
    a, _ = ba.render_splats(spl, cam, size, pass_=ba.RasterPass.Backward, ctx=ctx)
    b, _ = ba.render_splats(spl.transformed(T, ctx=ctx), cam.transformed(T), size, pass_=ba.RasterPass.Backward, ctx=ctx)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert float(a[..., 3].max()) > 0.5
    sr.assert_same_image(a, b)


def _region(kind, invert=False, floor=-math.inf, seed=1):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    R = sr.quat_to_matrix(q / np.linalg.norm(q)).astype(np.float32)
    return dict(kind=kind, invert=int(invert), center=rng.uniform(-1, 1, 3).astype(np.float32), half_extent=rng.uniform(1.5, 3.5, 3).astype(np.float32),
                rot=R.reshape(-1), min_raw_opacity=np.float32(floor))


def _host_region(ba, g):
    return ba.SceneRegion(("box", "ellipsoid")[g["kind"]], tuple(g["center"]), tuple(g["half_extent"]), tuple(g["rot"]), bool(g["invert"]), float(g["min_raw_opacity"]))


@pytest.mark.parametrize("kind", [0, 1])
def test_select_region_equals_the_restatement(dev, ctx, kind):
    import brush_amd as ba
    for n in (1, 255, 256, 257, 5000):
        tr, sh, op, _ = _scene(n, 0, 13 * n + kind)
        if n > 10:
            tr[3, 0], tr[5, 1], tr[7, 2], tr[9, :3] = np.nan, np.inf, -np.inf, np.nan
            op[11], op[12], op[13] = np.nan, np.inf, -np.inf
        spl = ba.Splats(tr, sh, op, device=dev)
        for invert in (False, True):
            for floor in (-math.inf, 1.0):
                g = _region(kind, invert, floor, seed=n + kind)
                want = sr.select_region_f32(g, tr, op)
                keep, count = ba.select_region(spl, _host_region(ba, g), ctx=ctx, return_count=True)
                got = keep.cpu().numpy()
                assert np.array_equal(got, want), (n, invert, floor, int((got != want).sum()))
                assert count == int(got.sum()) == int(want.sum())
                assert np.array_equal(ba.select_region(spl, _host_region(ba, g), ctx=ctx).cpu().numpy(), want)   # without the count
                assert n < 5000 or 0 < count < n
                if n > 10:
                    assert not got[[3, 5, 7, 9, 11]].any()
        # opacities not given: the geometric test and the finite means alone
        g = _region(kind, False, 1.0, seed=n + kind)
        keep = torch.empty((n,), device=dev)
        cnt = C.c_uint32(99)
        ctx.check(ctx.lib.bh_splats_select_region(ctx._h, C.byref(_host_region(ba, g).as_struct()), spl.transforms.data_ptr(), None, n, keep.data_ptr(), C.byref(cnt)))
        want = sr.select_region_f32(g, tr, None)
        assert np.array_equal(keep.cpu().numpy(), want) and cnt.value == int(want.sum())


def test_select_region_all_none_and_refusals(dev, ctx):
    import brush_amd as ba
    n = 1000
    tr, sh, op, _ = _scene(n, 0, 17)
    spl = ba.Splats(tr, sh, op, device=dev)
    big = ba.SceneRegion("box", (0, 0, 0), (10, 10, 10))
    far = ba.SceneRegion("ellipsoid", (100, 0, 0), (1, 1, 1))
    assert ba.select_region(spl, big, ctx=ctx, return_count=True)[1] == n and bool((ba.select_region(spl, big, ctx=ctx) == 1.0).all())
    assert ba.select_region(spl, far, ctx=ctx, return_count=True)[1] == 0 and bool((ba.select_region(spl, far, ctx=ctx) == 0.0).all())
    everything, idx = ba.crop_splats(spl, big, return_indices=True, ctx=ctx)
    assert everything.num_splats() == n and np.array_equal(idx.cpu().numpy(), np.arange(n))
    assert ba.crop_splats(spl, far, ctx=ctx).num_splats() == 0
    cnt = C.c_uint32(99)
    assert ctx.lib.bh_splats_select_region(ctx._h, C.byref(big.as_struct()), None, None, 0, None, C.byref(cnt)) == 0 and cnt.value == 0
    keep = torch.full((n,), 5.0, device=dev)
    for bad in (dict(half_extent=(1, 0, 1)), dict(half_extent=(1, -1, 1)), dict(half_extent=(1, math.inf, 1)), dict(center=(math.nan, 0, 0)),
                dict(min_raw_opacity=math.nan), dict(rotation=(math.nan,) + (0.0,) * 8)):
        g = ba.SceneRegion(**dict(dict(kind="box"), **bad)).as_struct()
        assert ctx.lib.bh_splats_select_region(ctx._h, C.byref(g), spl.transforms.data_ptr(), None, n, keep.data_ptr(), None) == -1, bad
    g = big.as_struct()
    g.kind = 2
    assert ctx.lib.bh_splats_select_region(ctx._h, C.byref(g), spl.transforms.data_ptr(), None, n, keep.data_ptr(), None) == -1
    assert bool((keep == 5.0).all())


def test_crop_returns_the_kept_rows_in_source_order(dev, ctx):
    import brush_amd as ba
    n = 5000
    tr, sh, op, ms = _scene(n, 2, 19)
    spl = ba.Splats(tr, sh, op, device=dev, min_scale=ms)
    g = _region(1, False, 0.0, seed=23)
    want = np.nonzero(sr.select_region_f32(g, tr, op))[0]
    assert 100 < want.size < n - 100
    crop, idx = ba.crop_splats(spl, _host_region(ba, g), return_indices=True, ctx=ctx)
    assert np.array_equal(idx.cpu().numpy(), want)
    for got, src in ((crop.transforms, tr), (crop.sh_coeffs, sh), (crop.raw_opacities, op), (crop.min_scale, ms)):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(src[want]))
    assert ba.crop_splats(spl, _host_region(ba, g), ctx=ctx).num_splats() == want.size
