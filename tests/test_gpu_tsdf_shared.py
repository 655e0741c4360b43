"""The pieces the dense and the sparse TSDF volume share (brush_amd/csrc/device_tsdf.h: the clear kernel, the load / fuse / store of a
sample, the integrate and the extraction driver), at the shapes where they can go wrong, and the `who` prefix of the refusals they
word for both volumes.

Shapes: 3x3x3 (27 samples: less than one block of the clear kernel, not a multiple of anything); 9x10x11 (no side a multiple of 8:
2x2x2 sparse blocks whose last blocks hold 1, 2 and 3 samples) with two 16x12 views, once with images into volumes without colour (the
alpha test applies, the colourless instantiation runs) and once without images into volumes with colour (the same instantiation, rgb
untouched).  The refusal texts are those of the commit before the drivers were shared."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import test_gpu_mesh as tgm
import test_gpu_sparse_mesh as tgs
import tsdf_ref as tr

pytestmark = pytest.mark.gpu
F = np.float32
DIMS, VOXEL = (9, 10, 11), 0.12
ORIGIN = tuple(float(c - 0.5 * VOXEL * (d - 1)) for c, d in zip(tgm.CENTRE, DIMS))   # the grid is centred on tgm's sphere
TRUNC = float(4 * F(VOXEL))
W, H = 16, 12
_CACHE = {}


@pytest.fixture
def ctx(dev):
    import brush_amd as ba
    c = ba.Context(dev)
    yield c
    c.close()


def _views():
    """Two 16x12 views of tgm's sphere with images whose alpha straddles ALPHA_MIN; computed once, never modified."""
    if "views" not in _CACHE:
        rng = np.random.default_rng(23)
        cams, depths, images = [], [], []
        for pos in ((1.9, 0.1, 0.9), (-0.4, 0.6, 2.1)):
            cam = tgm._bh_camera(pos, tgm.CENTRE, w=W, h=H, f=15.0)
            depth = tgm._sphere_depth(cam)
            assert (depth > 0).sum() > 20
            img = rng.uniform(0.0, 1.0, (H, W, 4)).astype(F)
            for a in (depth, img):
                a.setflags(write=False)
            cams.append(cam); depths.append(depth); images.append(img)
        _CACHE["views"] = (cams, depths, images)
    return _CACHE["views"]


def _ref(with_images):
    """The numpy restatement's {T, W} after the two views (no colour either way)."""
    if ("ref", with_images) not in _CACHE:
        cams, depths, images = _views()
        tw, _ = tr.new_volume(DIMS, False)
        tr.integrate(tw, None, ORIGIN, VOXEL, F(TRUNC), 64.0, [tgm._cam_dict(c) for c in cams], depths, images if with_images else None,
                     depth_min=tgm.DEPTH_MIN, alpha_min=tgm.ALPHA_MIN)
        tw.setflags(write=False)
        _CACHE[("ref", with_images)] = tw
    return _CACHE[("ref", with_images)]


def _fused(ctx, colour, with_images):
    """(dense, sparse) over the same grid after the two views."""
    import brush_amd as ba
    cams, depths, images = _views()
    dev = ctx.device
    args = ([torch.tensor(d, device=dev) for d in depths], cams, [torch.tensor(i, device=dev) for i in images] if with_images else None)
    dense = ba.TsdfVolume(ORIGIN, VOXEL, DIMS, trunc=TRUNC, colour=colour, ctx=ctx)
    sparse = ba.SparseTsdfVolume(ORIGIN, VOXEL, DIMS, trunc=TRUNC, colour=colour, ctx=ctx)
    sparse.mark(*args, alpha_min=tgm.ALPHA_MIN)
    assert sparse.commit() > 0
    for vol in (dense, sparse):
        vol.integrate(*args, depth_min=tgm.DEPTH_MIN, alpha_min=tgm.ALPHA_MIN)
    return dense, sparse


# ---- clear -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", [True, False])
def test_clear_of_27_samples(ctx, colour):
    import brush_amd as ba
    vol = ba.TsdfVolume((0.0, 0.0, 0.0), 1.0, (3, 3, 3), colour=colour, ctx=ctx)
    vol.tw.fill_(7.0)
    if colour:
        vol.rgb.fill_(7.0)
    vol.clear()
    assert np.array_equal(tgm._bits(vol.tw.cpu().numpy()), np.broadcast_to(tgm._bits(np.asarray([1.0, 0.0], F)), (3, 3, 3, 2)))
    assert (vol.rgb is None) == (not colour)
    if colour:
        assert np.array_equal(tgm._bits(vol.rgb.cpu().numpy()), np.zeros((3, 3, 3, 3), np.uint32))


# ---- integrate -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour,with_images", [(False, True), (True, False)])
def test_integrate_without_a_colour_to_fuse(ctx, colour, with_images):
    want = _ref(with_images)
    seen = want[..., 1] > 0
    assert 50 < seen.sum() < seen.size and (want[..., 0][seen] < 0).any()
    assert (_ref(False)[..., 1] > 0).sum() > (_ref(True)[..., 1] > 0).sum()   # the alpha test removed pixels
    dense, sparse = _fused(ctx, colour, with_images)
    dense_tw = dense.tw.cpu().numpy()
    assert np.array_equal(tgm._bits(dense_tw), tgm._bits(want))
    have = tgs._same_as_dense(sparse, dense_tw, dense.rgb.cpu().numpy() if colour else None)
    assert (have & seen).sum() > 50
    if colour:   # no image: the colour stays as cleared
        assert (dense.rgb == 0).all() and (sparse.rgb == 0).all()
    else:
        assert dense.rgb is None and sparse.rgb is None


# ---- extract ---------------------------------------------------------------------------------------------------------------------
def test_a_volume_without_a_crossing_extracts_nothing(ctx):
    import brush_amd as ba
    dense = ba.TsdfVolume(ORIGIN, VOXEL, DIMS, trunc=TRUNC, ctx=ctx)
    sparse = ba.SparseTsdfVolume(ORIGIN, VOXEL, DIMS, trunc=TRUNC, ctx=ctx)
    sparse.bits.fill_(0xFF)   # all 2x2x2 blocks
    assert sparse.commit(0) == 8
    nv, nt = C.c_uint32(9), C.c_uint32(9)
    for vol, struct, entry in ((dense, dense.grid, ctx.lib.bh_tsdf_extract), (sparse, sparse.vol, ctx.lib.bh_sptsdf_extract)):
        vol.tw[..., 1] = 1.0   # observed everywhere, T = 1 everywhere
        assert vol.count() == (0, 0)
        v, c, t = vol.extract_mesh()
        assert v.shape == (0, 3) and c.shape == (0, 3) and t.shape == (0, 3)
        s = struct()
        nv.value = nt.value = 9
        assert entry(ctx._h, C.byref(s), None, None, None, 0, 0, C.byref(nv), C.byref(nt)) == 0 and (nv.value, nt.value) == (0, 0)


# ---- the refusals' prefixes ------------------------------------------------------------------------------------------------------
def test_refusals_carry_the_entry_points_own_name(ctx):
    from brush_amd import _ffi
    lib, h = ctx.lib, ctx._h
    dense, sparse = _fused(ctx, False, True)
    cams, depths, _ = _views()
    d = torch.tensor(depths[0], device=ctx.device)
    cfg = _ffi.BhTsdfIntegrateConfig(0.0, math.inf, 0.5, 0)
    nv, nt = C.c_uint32(), C.c_uint32()

    def refused(rc, text):
        assert rc == -1 and lib.bh_last_error(h).decode() == text, lib.bh_last_error(h).decode()

    for vol, struct, prefix in ((dense, dense.grid, "tsdf"), (sparse, sparse.vol, "sptsdf")):
        before = tgm._bits(vol.tw.cpu().numpy()).copy()
        s = struct()
        integrate, count, extract = (getattr(lib, "bh_%s_%s" % (prefix, e)) for e in ("integrate", "extract_count", "extract"))
        one, ptr = (_ffi.BhCamera * 1)(cams[0]), (C.c_void_p * 1)(d.data_ptr())
        refused(integrate(h, C.byref(s), 1, one, ptr, None, None), prefix + "_integrate: null config")
        one[0].model = _ffi.CAMERA_KANNALA_BRANDT_4
        refused(integrate(h, C.byref(s), 1, one, ptr, None, C.byref(cfg)), prefix + "_integrate: pinhole cameras only")
        refused(count(h, C.byref(s), None, C.byref(nt)), prefix + "_extract_count: null count pointer")
        n_v, n_t = vol.count()
        assert n_v > 10 and n_t > 10
        verts = torch.empty((n_v, 3), device=ctx.device)
        tris = torch.empty((n_t, 3), dtype=torch.int32, device=ctx.device)
        refused(extract(h, C.byref(s), verts.data_ptr(), None, tris.data_ptr(), n_v - 1, n_t, C.byref(nv), C.byref(nt)), prefix + "_extract: output capacity too small")
        assert (nv.value, nt.value) == (n_v, n_t)
        refused(extract(h, C.byref(s), verts.data_ptr(), verts.data_ptr(), tris.data_ptr(), n_v, n_t, C.byref(nv), C.byref(nt)),
                prefix + "_extract: colours of a volume without rgb")
        refused(extract(h, C.byref(s), None, None, tris.data_ptr(), n_v, n_t, C.byref(nv), C.byref(nt)), prefix + "_extract: null output")
        assert np.array_equal(tgm._bits(vol.tw.cpu().numpy()), before)   # nothing was launched on the volume
    g = dense.grid()
    g.nx = 1
    refused(lib.bh_tsdf_clear(h, C.byref(g)), "tsdf_clear: every dimension of the grid must be at least 2")
    refused(lib.bh_sptsdf_to_dense(h, C.byref(sparse.vol()), 0, 0, 0, C.byref(g)), "sptsdf_to_dense: every dimension of the dense grid must be at least 2")
    g.nx, g.ny, g.nz = 2048, 1024, 1024
    refused(lib.bh_tsdf_clear(h, C.byref(g)), "tsdf_clear: more than 2^31 - 1 samples")
    refused(lib.bh_sptsdf_to_dense(h, C.byref(sparse.vol()), 0, 0, 0, C.byref(g)), "sptsdf_to_dense: more than 2^31 - 1 dense samples")
    v = sparse.vol()
    v.ny = 1
    refused(lib.bh_sptsdf_clear(h, C.byref(v)), "sptsdf_clear: every dimension of the grid must be at least 2")
