"""bh_splat_to_compressed_ply on the GPU against the numpy restatement tests/compressed_ply_ref.py, byte for byte: sizes, SH
degrees, header variants, the edge rows of the contract, the row order, the size query, the 3D-filter floor, the header parser, the
read-back through load_splat_from_ply and, at 1 M splats / SH 3, the render of the re-imported model."""
import numpy as np
import pytest
import torch

import compressed_ply_ref as ref

pytestmark = pytest.mark.gpu


def _splats(ba, dev, t, sh, o, mip=False, min_scale=None):
    return ba.Splats(torch.from_numpy(t), torch.from_numpy(sh), torch.from_numpy(o), render_mip=mip, device=dev,
                     min_scale=None if min_scale is None else torch.from_numpy(min_scale))


def _first_difference(a, b):
    if len(a) != len(b):
        return "lengths %d != %d" % (len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8))
    return "%d bytes differ, first at %d" % (d.size, d[0]) if d.size else "equal"


def _empty_export(ba, dev, d, mip, up):
    import ctypes as C
    ctx = ba.get_context(dev)
    upf = (C.c_float * 3)(*up) if up is not None else None
    need = C.c_uint64(0)
    ctx.check(ctx.lib.bh_splat_to_compressed_ply(ctx._h, None, None, None, None, 0, d, int(mip), upf, None, None, 0, C.byref(need)))
    buf = (C.c_char * need.value)()
    ctx.check(ctx.lib.bh_splat_to_compressed_ply(ctx._h, None, None, None, None, 0, d, int(mip), upf, None, buf, need.value, C.byref(need)))
    return bytes(buf)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 4097, 100000])
@pytest.mark.parametrize("d", [0, 1, 2, 3, 4])
def test_bytes_equal_the_restatement(dev, n, d):
    import brush_amd as ba
    t, sh, o = ref.random_scene(n, d, seed=1000 * d + n)
    for mip, up in ((False, None), (True, None), (False, (0.0, 0.0, -1.0)), (True, (0.25, -1.0, 1e-3))):
        # (an empty Splats carries one coefficient: the degree of an empty export goes through the C ABI)
        got = ba.splat_to_compressed_ply(_splats(ba, dev, t, sh, o, mip), up_axis=up) if n else _empty_export(ba, dev, d, mip, up)
        want = ref.compressed_ply(t, sh, o, render_mip=mip, up_axis=up)
        assert got == want, (mip, up, _first_difference(got, want))


@pytest.mark.parametrize("d", [0, 1, 2, 3, 4])
def test_edge_rows_bytes_equal_the_restatement(dev, d):
    import brush_amd as ba
    t, sh, o = ref.edge_scene(d, seed=d)
    got, order = ba.splat_to_compressed_ply(_splats(ba, dev, t, sh, o), return_order=True)
    want, want_order = ref.compressed_ply(t, sh, o, return_order=True)
    assert np.array_equal(order.cpu().numpy().view(np.uint32), want_order)
    assert got == want, _first_difference(got, want)


def test_order_is_the_stable_argsort_of_the_keys(dev):
    import brush_amd as ba
    n = 70000
    t, sh, o = ref.random_scene(n, 1, seed=3)
    t[:, 0:3] = np.round(t[:, 0:3] / 2) * 2   # 6 values per axis: equal cells, whose rows must keep input order
    _, order = ba.splat_to_compressed_ply(_splats(ba, dev, t, sh, o), return_order=True)
    keys = ref.morton_keys(t[:, 0:3])
    assert np.array_equal(order.cpu().numpy().view(np.uint32), np.argsort(keys, kind="stable"))
    assert np.unique(keys).size < n // 4


def test_size_query_and_repeat_calls(dev):
    import ctypes as C
    import brush_amd as ba
    t, sh, o = ref.random_scene(5000, 3, seed=4)
    s = _splats(ba, dev, t, sh, o)
    ctx = ba.get_context(s.device)
    need = C.c_uint64(0)
    # a size query reads no tensor: null pointers are fine
    ctx.check(ctx.lib.bh_splat_to_compressed_ply(ctx._h, None, None, None, None, 5000, 3, 0, None, None, None, 0, C.byref(need)))
    a = ba.splat_to_compressed_ply(s)
    b = ba.splat_to_compressed_ply(s)
    assert need.value == len(a) and a == b
    buf = (C.c_char * (need.value - 1))()
    assert ctx.lib.bh_splat_to_compressed_ply(ctx._h, ba.host._ptr(s.transforms), ba.host._ptr(s.sh_coeffs), ba.host._ptr(s.raw_opacities), None,
                                              5000, 3, 0, None, None, buf, need.value - 1, C.byref(need)) == -1
    assert ctx.lib.bh_splat_to_compressed_ply(ctx._h, None, None, None, None, 10, 5, 0, None, None, None, 0, C.byref(need)) == -1
    empty = ba.splat_to_compressed_ply(_splats(ba, dev, t[:0], sh[:0], o[:0]))
    assert empty == ref.compressed_ply(t[:0], sh[:0, :1], o[:0])   # an empty Splats carries one coefficient


def test_min_scale_is_folded_first(dev):
    import brush_amd as ba
    t, sh, o = ref.random_scene(3000, 2, seed=5)
    ms = np.random.default_rng(6).uniform(0, 0.05, 3000).astype(np.float32)
    s = _splats(ba, dev, t, sh, o, min_scale=ms)
    ft, fo = s.folded()
    folded = ba.Splats(ft, s.sh_coeffs, fo, device=dev)
    a = ba.splat_to_compressed_ply(s)
    assert a == ba.splat_to_compressed_ply(folded)
    assert a == ref.compressed_ply(t, sh, o, min_scale=ms)


def test_header_parses_and_reads_back(dev):
    import brush_amd as ba
    from oracle import ply as oply
    for n, d, mip, up in ((3000, 3, True, (0.0, 0.0, -1.0)), (600, 0, False, None), (257, 4, False, (1.0, 0.0, 0.0))):
        t, sh, o = ref.random_scene(n, d, seed=7 + d)
        data, order = ba.splat_to_compressed_ply(_splats(ba, dev, t, sh, o, mip), up_axis=up, return_order=True)
        meta = ba.ply_parse_header(data)
        assert meta.compressed and meta.total_splats == n and meta.sh_degree == d
        assert meta.render_mode == ("mip" if mip else "default")
        assert meta.up_axis == (tuple(np.float32(v) for v in up) if up else (0.0, -1.0, 0.0))
        back, _ = ba.load_splat_from_ply(data, device=dev)
        want = oply.load_compressed_ply(data)
        for got, exp in ((back.transforms, want["transforms"]), (back.sh_coeffs, want["sh"]), (back.raw_opacities, want["raw_opac"])):
            g = got.cpu().numpy()
            assert g.shape == exp.shape
            assert np.allclose(g, exp, rtol=1e-6, atol=1e-6, equal_nan=True)
        assert back.render_mip == mip
        bad = ref.round_trip_violations(data, order.cpu().numpy().view(np.uint32), t, sh, o)
        assert not any(bad.values()), bad


def test_1m_sh3_bytes_and_render_psnr(dev):
    """1 M splats of synth.make_scene at SH degree 3: bytes equal the restatement, and the re-imported model renders the 1920x1080
    default view close to the original.  Measured on the MI355X: PSNR 30.44 dB; the floor is 28 dB.  Most of the loss is the reader's
    u8 / 254 SH decode, which moves every higher-band coefficient by up to 0.0315: the writer's bytes are pinned
    exactly above, so the floor guards the round trip as a whole."""
    import brush_amd as ba
    from brush_amd import synth
    import util
    sc = synth.make_scene(1_000_000, seed=11, sh_degree=3)
    s = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    data = ba.splat_to_compressed_ply(s)
    want = ref.compressed_ply(sc["transforms"], sc["sh"], sc["raw_opac"])
    assert data == want, _first_difference(data, want)
    back, _ = ba.load_splat_from_ply(data, device=dev)
    w, h = 1920, 1080
    cam = util.hip_camera(ba, synth.default_camera_params(w, h))
    a, _ = ba.render_splats(s, cam, (w, h), (0, 0, 0), ba.RasterPass.Backward)
    b, _ = ba.render_splats(back, cam, (w, h), (0, 0, 0), ba.RasterPass.Backward)
    mse = float(((a[..., :3].double() - b[..., :3].double()) ** 2).mean())
    psnr = 10 * np.log10(1.0 / max(mse, 1e-20))
    print("compressed round trip: PSNR %.2f dB over %d x %d" % (psnr, w, h))
    assert psnr >= 28.0, psnr
