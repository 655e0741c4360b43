"""Sparse TSDF volumes on the GPU (include/brush_hip_sparse_mesh.h), through brush_amd/host.py and the C ABI.

Exact, bit for bit: the marked and the allocated sets, rank and keys against the restatement tests/sptsdf_ref.py; every allocated sample
against the dense TsdfVolume fused with the same views (and {1, 0, 0} elsewhere in the dense image); the mesh against the dense
extraction of bh_sptsdf_to_dense's volume, each vertex matched through its owner sample and edge direction (sptsdf_ref.sparse_order),
triangles as canonical sets.  Against DENSE FUSION the mesh is compared only where containment was established: tests/sptsdf_cases.py's
two scenes (asserted on the CPU in tests/test_sptsdf_ref.py) and the splat scene, whose containment is computed here from the depth maps
read back, before the meshes are compared.

Shapes: 40x33x26 (5x5x4 blocks, last blocks of 8, 1 and 2 samples; the sphere leaves the grid), 24^3 and 16^3 written straight into
the pool, and one 4096^3 virtual grid the dense path refuses."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import sptsdf_cases as sc
import sptsdf_ref as sr
import test_gpu_mesh as tgm
import tsdf_ref as tr

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture
def ctx(dev):
    import brush_amd as ba
    c = ba.Context(dev)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _sparse(ctx, name="three", colour=True, max_weight=64.0, **kw):
    import brush_amd as ba
    s = sc.SCENES[name]
    args = dict(origin=s["origin"], voxel_size=sc.VOXEL, dims=s["dims"], trunc=sc.TRUNC, max_weight=max_weight, colour=colour, ctx=ctx)
    args.update(kw)
    return ba.SparseTsdfVolume(**args)


def _dense(ctx, name="three", colour=True, max_weight=64.0):
    import brush_amd as ba
    s = sc.SCENES[name]
    return ba.TsdfVolume(s["origin"], sc.VOXEL, s["dims"], trunc=sc.TRUNC, max_weight=max_weight, colour=colour, ctx=ctx)


def _call(vol, what, name, idx, with_images=True):
    cams, depths, images = sc.views(sc.SCENES[name]["n_views"])
    dev = vol.device
    args = ([torch.tensor(depths[i], device=dev) for i in idx], [cams[i] for i in idx], [torch.tensor(images[i], device=dev) for i in idx] if with_images else None)
    if what == "mark":
        vol.mark(*args, alpha_min=sc.ALPHA_MIN)
    else:
        vol.integrate(*args, depth_min=sc.DEPTH_MIN, alpha_min=sc.ALPHA_MIN)


def _fuse(ctx, name, colour=True, with_images=True, max_weight=64.0, dilate=1):
    n = sc.SCENES[name]["n_views"]
    vol = _sparse(ctx, name, colour, max_weight)
    _call(vol, "mark", name, range(n), with_images)
    assert vol.commit(dilate) > 0
    _call(vol, "integrate", name, range(n), with_images)
    return vol


# ---- 1. marking ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_images", [True, False])
def test_marking_matches_the_restatement_bit_for_bit(ctx, with_images):
    want = sc.marked("three", with_images)
    bits, _, _ = sr.index_of(want)
    assert 0 < want.sum() < want.size
    one = _sparse(ctx)
    assert one.n_words == len(bits) == 4 and (one.bits == 0).all()
    _call(one, "mark", "three", [0, 1, 2], with_images)
    assert np.array_equal(_u32(one.bits), bits)
    two = _sparse(ctx)
    _call(two, "mark", "three", [0], with_images)
    assert np.array_equal(_u32(two.bits), sr.index_of(sc.marked("three", with_images, n_views=1))[0])
    _call(two, "mark", "three", [1, 2], with_images)
    _call(two, "mark", "three", [1], with_images)   # marking is idempotent
    assert np.array_equal(_u32(two.bits), bits)
    two.mark_clear()
    assert (two.bits == 0).all()


@pytest.mark.parametrize("dilate", [0, 1, 2])
def test_commit_dilates_ranks_and_counts(ctx, dilate):
    marked = sc.marked("three")
    bits, rank, keys = sr.index_of(sr.dilate(marked, dilate))
    vol = _sparse(ctx)
    _call(vol, "mark", "three", [0, 1, 2])
    assert vol.commit(dilate) == len(keys) == vol.n_blocks
    assert np.array_equal(_u32(vol.bits), bits) and np.array_equal(_u32(vol.rank), rank) and np.array_equal(_u32(vol.keys), keys)
    assert vol.tw.shape == (len(keys), 8, 8, 8, 2) and vol.rgb.shape == (len(keys), 8, 8, 8, 3)
    assert (vol.tw.cpu().numpy() == np.asarray([1.0, 0.0], F)).all() and (vol.rgb == 0).all()
    with pytest.raises(ValueError, match="mark_clear"):
        _call(vol, "mark", "three", [0])


def test_commit_of_a_bitmap_that_spans_many_words(ctx):
    """A 200x40x40 grid: 25x5x5 = 625 blocks in 20 words, rows that straddle words; random marks, all three radii."""
    import brush_amd as ba
    rng = np.random.default_rng(9)
    marked = rng.uniform(size=(5, 5, 25)) < 0.03
    marked[0, 0, 0] = marked[4, 4, 24] = True
    for dilate in (0, 1, 2):
        vol = ba.SparseTsdfVolume((0.0, 0.0, 0.0), 0.1, (200, 40, 40), colour=False, ctx=ctx)
        vol.bits.copy_(torch.from_numpy(sr.index_of(marked)[0].view(np.int32)))
        bits, rank, keys = sr.index_of(sr.dilate(marked, dilate))
        assert vol.commit(dilate) == len(keys)
        assert np.array_equal(_u32(vol.bits), bits) and np.array_equal(_u32(vol.rank), rank) and np.array_equal(_u32(vol.keys), keys)


# ---- 2. integration --------------------------------------------------------------------------------------------------------------
def _same_as_dense(sparse, dense_tw, dense_rgb):
    """to_dense(sparse) holds the dense volume's bits on every allocated sample and {1, 0, 0} elsewhere; the pool's samples that do not
    exist are as cleared."""
    keys = _u32(sparse.keys)
    have = sr.pool_indices(keys, sparse.dims) >= 0
    image = sparse.to_dense()
    got = image.tw.cpu().numpy()
    assert np.array_equal(_bits(got[have]), _bits(dense_tw[have])), "%d allocated samples differ" % (_bits(got[have]) != _bits(dense_tw[have])).any(axis=-1).sum()
    assert (got[~have] == np.asarray([1.0, 0.0], F)).all()
    pool_tw = sparse.tw.cpu().numpy()
    want_pool, _ = sr.to_pool(np.where(have[..., None], dense_tw, np.asarray([1.0, 0.0], F)), None, keys, sparse.dims)
    assert np.array_equal(_bits(pool_tw), _bits(want_pool))
    if sparse.rgb is not None:
        rgb = image.rgb.cpu().numpy()
        assert np.array_equal(_bits(rgb[have]), _bits(dense_rgb[have])) and (rgb[~have] == 0).all()
    return have


@pytest.mark.parametrize("colour,with_images", [(True, True), (False, True), (True, False)])
def test_integration_equals_the_dense_volume_on_every_allocated_sample(ctx, colour, with_images):
    sparse = _fuse(ctx, "three", colour, with_images)
    dense = _dense(ctx, "three", colour)
    _call(dense, "integrate", "three", [0, 1, 2], with_images)
    dense_tw, dense_rgb = dense.tw.cpu().numpy(), dense.rgb.cpu().numpy() if colour else None
    want_tw, want_rgb = sc.fused("three", colour, with_images)
    assert np.array_equal(_bits(dense_tw), _bits(want_tw))
    have = _same_as_dense(sparse, dense_tw, dense_rgb)
    touched = have & (want_tw[..., 1] > 0)
    assert touched.sum() > 500 and (want_tw[..., 1][have] == 3).any() and (want_tw[..., 0][have] < 0).any() and (have & (want_tw[..., 1] == 0)).any()
    if colour and not with_images:
        assert (sparse.rgb == 0).all()


def test_a_batch_of_eleven_views_equals_eleven_single_calls(ctx):
    want_tw, want_rgb = sc.fused("sphere", True, True, 4.0)
    assert want_tw[..., 1].max() == 4.0 and (want_tw[..., 1] == 4.0).sum() > 100   # the clamp at max_weight is reached
    batched = _fuse(ctx, "sphere", max_weight=4.0)
    single = _sparse(ctx, "sphere", max_weight=4.0)
    _call(single, "mark", "sphere", range(11))
    assert single.commit() == batched.n_blocks
    for i in range(11):
        _call(single, "integrate", "sphere", [i])
    for vol in (batched, single):
        _same_as_dense(vol, want_tw, want_rgb)
    assert np.array_equal(_bits(batched.tw.cpu().numpy()), _bits(single.tw.cpu().numpy()))


# ---- 3. extraction ---------------------------------------------------------------------------------------------------------------
def _check_extract(vol, closed=False):
    """The sparse mesh against the dense extraction of the volume's dense image."""
    keys = _u32(vol.keys)
    image = vol.to_dense()
    dense_tw = image.tw.cpu().numpy()
    want_tw, want_rgb = sr.to_dense(vol.tw.cpu().numpy(), vol.rgb.cpu().numpy() if vol.rgb is not None else None, keys, vol.dims)
    assert np.array_equal(_bits(dense_tw), _bits(want_tw))
    if vol.rgb is not None:
        assert np.array_equal(_bits(image.rgb.cpu().numpy()), _bits(want_rgb))
    dv, dc, dt = image.extract_mesh()
    perm = sr.sparse_order(dense_tw, keys, vol.dims)
    assert len(perm) == len(dv)
    want_v, want_c, want_t = sr.reorder_mesh(dv.cpu().numpy(), dc.cpu().numpy() if dc is not None else None, _u32(dt), perm)
    assert vol.count() == (len(want_v), len(want_t)) == image.count()
    v, c, t = vol.extract_mesh()
    v, t = v.cpu().numpy(), _u32(t)
    assert v.shape == want_v.shape and t.shape == want_t.shape
    assert np.array_equal(_bits(v), _bits(want_v)), "%d vertices differ" % (_bits(v) != _bits(want_v)).any(axis=1).sum()
    if vol.rgb is not None:
        assert np.array_equal(_bits(c.cpu().numpy()), _bits(want_c))
    else:
        assert c is None
    if len(t):
        assert t.max() < len(v) and np.array_equal(np.unique(t), np.arange(len(v)))
    assert np.array_equal(tr.canonical(t), tr.canonical(want_t))
    if closed:
        e = tr.directed_edges(t)
        assert len(np.unique(e[:, 0] * len(v) + e[:, 1])) == len(e) and len(tr.boundary_edges(t)) == 0 and tr.signed_volume(v, t) > 0
    again = vol.extract_mesh()
    assert np.array_equal(_bits(again[0].cpu().numpy()), _bits(v)) and np.array_equal(_u32(again[2]), t)
    return v, c, t


def _written(ctx, dims, origin, voxel, allocated, tw, rgb=None):
    """A sparse volume with the blocks `allocated` [NBZ,NBY,NBX] whose pool holds the dense arrays' samples."""
    import brush_amd as ba
    vol = ba.SparseTsdfVolume(origin, voxel, dims, colour=rgb is not None, ctx=ctx)
    bits, _, keys = sr.index_of(allocated)
    vol.bits.copy_(torch.from_numpy(bits.view(np.int32)))
    assert vol.commit(0) == len(keys) and np.array_equal(_u32(vol.keys), keys)
    ptw, prgb = sr.to_pool(tw, rgb, keys, dims)
    vol.tw.copy_(torch.from_numpy(ptw))
    if rgb is not None:
        vol.rgb.copy_(torch.from_numpy(prgb))
    return vol


def test_extract_the_fused_scene_with_colours(ctx):
    vol = _fuse(ctx, "three")
    v, c, t = _check_extract(vol)
    assert len(t) > 100 and c.shape == v.shape
    # containment holds on this scene (tests/test_sptsdf_ref.py): the mesh is the mesh of dense fusion
    tw, rgb = sc.fused("three")
    s = sc.SCENES["three"]
    want = sr.reorder_mesh(*tr.extract(tw, rgb, s["origin"], sc.VOXEL), sr.sparse_order(tw, _u32(vol.keys), s["dims"]))
    assert np.array_equal(_bits(v), _bits(want[0])) and np.array_equal(_bits(c.cpu().numpy()), _bits(want[1]))
    assert np.array_equal(tr.canonical(t), tr.canonical(want[2]))


@pytest.mark.parametrize("which", ["all", "shell", "half"])
def test_extract_an_analytic_sphere_written_into_the_pool(ctx, which):
    n, origin, voxel = 24, (-1.15,) * 3, 0.1
    tw, _ = tr.new_volume((n, n, n), False)
    px, py, pz = tr.sample_positions(origin, voxel, (n, n, n))
    r = np.sqrt(px * px + py * py + pz * pz).astype(F)
    tw[..., 0] = np.clip((r - F(1.0)) / F(0.15), -1, 1).astype(F)
    tw[..., 1] = 1.0
    band = np.abs(tw[..., 0]) < 1
    allocated = np.ones((3, 3, 3), bool)
    if which == "shell":   # only the blocks that hold a sample of the band: the centre block is not one of them
        allocated = band.reshape(3, 8, 3, 8, 3, 8).any(axis=(1, 3, 5))
        assert allocated.sum() == 26 and not allocated[1, 1, 1]
    elif which == "half":   # the blocks of the lower two layers: the surface ends at unallocated blocks
        allocated[2] = False
    vol = _written(ctx, (n, n, n), origin, voxel, allocated, tw)
    v, _, t = _check_extract(vol, closed=which != "half")
    assert len(t) > 2000
    if which != "half":   # the whole sphere, whatever lies unallocated inside it
        full = tr.extract(tw, None, origin, voxel)
        assert (len(v), len(t)) == (len(full[0]), len(full[2]))
    else:
        assert v[:, 2].max() <= F(origin[2]) + F(voxel) * F(15) and len(tr.boundary_edges(t)) > 0


def test_crossings_on_block_faces_edges_and_the_shared_corner(ctx):
    """16^3 samples in 2x2x2 blocks; the zero level passes between the blocks: a plane between two layers of blocks, a plane through the
    four blocks' shared edge, a small sphere around the shared corner, and random signs everywhere with a few samples unobserved."""
    rng = np.random.default_rng(21)
    dims, origin, voxel = (16, 16, 16), (0.3, -0.7, 1.1), 0.25
    k, j, i = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij")
    fields = [
        (i - 7.5) / 4.0,                                                       # the face between bx = 0 and 1
        (i + j - 15.0) / 6.0,                                                  # through the edge the four (bx, by) share
        (np.sqrt((i - 7.5) ** 2 + (j - 7.5) ** 2 + (k - 7.5) ** 2) - 1.3) / 3.0,   # around the corner all eight share
        np.where(rng.uniform(size=i.shape) < 0.5, -1.0, 1.0) * rng.uniform(0.1, 1.0, i.shape),
    ]
    for n, field in enumerate(fields):
        tw, rgb = tr.new_volume(dims, True)
        tw[..., 0] = np.clip(field, -1, 1).astype(F)
        tw[..., 1] = (rng.uniform(size=i.shape) > (0.02 if n == 3 else 0.0)).astype(F)
        rgb[...] = rng.uniform(size=rgb.shape).astype(F)
        vol = _written(ctx, dims, origin, voxel, np.ones((2, 2, 2), bool), tw, rgb)
        v, _, t = _check_extract(vol, closed=n == 2)
        want = tr.extract(tw, rgb, origin, voxel)
        assert len(t) == len(want[2]) > 40 and len(v) == len(want[0])
    # one block of the eight missing: its samples count as unobserved
    allocated = np.ones((2, 2, 2), bool)
    allocated[1, 0, 1] = False
    tw, _ = tr.new_volume(dims, False)
    tw[..., 0] = np.clip(fields[1], -1, 1).astype(F)
    tw[..., 1] = 1.0
    _, _, t = _check_extract(_written(ctx, dims, origin, voxel, allocated, tw))
    assert 0 < len(t) < len(tr.extract(tw, None, origin, voxel)[2])


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------
def test_the_sphere_scene_fused_sparsely_has_the_mesh_of_dense_fusion(ctx):
    vol = _fuse(ctx, "sphere")
    v, c, t = _check_extract(vol)
    tw, rgb = sc.fused("sphere")
    s = sc.SCENES["sphere"]
    want = sr.reorder_mesh(*tr.extract(tw, rgb, s["origin"], sc.VOXEL), sr.sparse_order(tw, _u32(vol.keys), s["dims"]))
    assert len(t) > 500 and np.array_equal(_bits(v), _bits(want[0])) and np.array_equal(_bits(c.cpu().numpy()), _bits(want[1]))
    assert np.array_equal(tr.canonical(t), tr.canonical(want[2]))


def test_fuse_views_gives_the_dense_mesh_from_both_volumes(ctx):
    """test_gpu_mesh's splat scene: about 300 splats on a sphere, four 64x48 cameras, fused through fuse_views into a dense and a sparse
    volume.  Containment is computed from the rendered depth maps first (and asserted: the comparison stands on it)."""
    import brush_amd as ba
    n, w, h = 300, 64, 48
    rng = np.random.default_rng(3)
    p = rng.normal(size=(n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    tf = np.zeros((n, 10), F)
    tf[:, :3] = p + np.asarray([0.0, 0.0, 3.0])
    tf[:, 3] = 1.0
    tf[:, 7:] = np.log(rng.uniform(0.12, 0.2, (n, 3)))
    splats = ba.Splats(tf, rng.uniform(0.0, 1.5, (n, 1, 3)).astype(F), np.full(n, 4.0, F), device=ctx.device)
    cams = [ba.Camera(position=pos, fov_x=0.9, fov_y=0.7, center_uv=(0.52, 0.47)) for pos in ((0.6, 0.3, 0.0), (-0.6, 0.3, 0.1), (0.5, -0.4, -0.1), (-0.4, -0.5, 0.0))]
    dims, origin, voxel, trunc = (26, 27, 28), (-1.25, -1.3, 1.65), 0.1, 0.4
    dense = ba.fuse_views(splats, cams, (w, h), ba.TsdfVolume(origin, voxel, dims, trunc=trunc, ctx=ctx))
    sparse = ba.fuse_views(splats, cams, (w, h), ba.SparseTsdfVolume(origin, voxel, dims, trunc=trunc, ctx=ctx))
    assert 0 < sparse.n_blocks <= 4 * 4 * 4
    # containment, from the depth maps the forward renders
    dicts, depths, images = [], [], []
    for cam in cams:
        node = ba.render_splats_diff(splats, cam, (w, h), ctx=ctx)
        depths.append(node.depth("expected").cpu().numpy())
        images.append(node.img.clone().cpu().numpy())
        dicts.append(sc.cam_dict(cam.uniforms((w, h))))
    marked = np.zeros((4, 4, 4), bool)
    sr.mark(marked, origin, voxel, dims, trunc, dicts, depths, images)
    allocated = sr.dilate(marked, 1)
    assert np.array_equal(_u32(sparse.keys), sr.index_of(allocated)[2])
    needed = sr.dilate(sr.band_blocks(origin, voxel, dims, trunc, dicts, depths, images), 1)
    print("fuse_views: %d of %d blocks marked, %d needed, %d allocated" % (marked.sum(), marked.size, needed.sum(), allocated.sum()))
    assert needed.any() and not (needed & ~allocated).any()
    dense_tw, dense_rgb = dense.tw.cpu().numpy(), dense.rgb.cpu().numpy()
    _same_as_dense(sparse, dense_tw, dense_rgb)
    v, c, t = _check_extract(sparse)
    dv, dc, dt = dense.extract_mesh()
    want = sr.reorder_mesh(dv.cpu().numpy(), dc.cpu().numpy(), _u32(dt), sr.sparse_order(dense_tw, _u32(sparse.keys), dims))
    assert len(t) > 300 and np.array_equal(_bits(v), _bits(want[0])) and np.array_equal(_bits(c.cpu().numpy()), _bits(want[1]))
    assert np.array_equal(tr.canonical(t), tr.canonical(want[2]))


# ---- 5. a grid the dense path cannot hold -----------------------------------------------------------------------------------------
def test_a_4096_cubed_grid_around_a_small_plane(ctx):
    """6.9e10 virtual samples at 2^-8 (3.9 mm) over 16 m.  One 64x48 view sees a 16x12 pixel patch of a plane one unit away.  The voxel
    size is a power of two and the origin a multiple of it, so origin + voxel * (i0 + i) = (origin + voxel * i0) + voxel * i exactly in
    f32 (asserted): the restatement runs on a window around the allocated blocks alone and must give the same bits."""
    import brush_amd as ba
    dims, origin, voxel = (4096,) * 3, (-8.0,) * 3, 2.0 ** -8
    trunc = 4 * voxel
    with pytest.raises(ValueError, match="samples"):
        ba.TsdfVolume(origin, voxel, dims, ctx=ctx)
    w, h = 64, 48
    cam = tgm._bh_camera((0.1, -0.2, -0.3), (0.3, 0.1, 1.0), w=w, h=h, f=200.0)
    depth = np.zeros((h, w), F)
    depth[20:32, 22:38] = 1.0
    rng = np.random.default_rng(17)
    image = rng.uniform(0.0, 1.0, (h, w, 4)).astype(F)
    image[..., 3] = 1.0
    dev = ctx.device
    vol = ba.SparseTsdfVolume(origin, voxel, dims, ctx=ctx)
    assert vol.block_dims == (512,) * 3 and vol.n_words == 2 ** 22 and vol.mark_steps() == 2
    args = ([torch.tensor(depth, device=dev)], [cam], [torch.tensor(image, device=dev)])
    vol.mark(*args)
    n_blocks = vol.commit()
    vol.integrate(*args)
    print("4096^3: %d blocks allocated of %d, %.1f KB of pool" % (n_blocks, 512 ** 3, n_blocks * 512 * 20 / 1024))
    assert 8 <= n_blocks <= 200
    keys = _u32(vol.keys)
    bx, by, bz = sr.block_coords(keys, dims)
    # the allocated set: the restatement's marks, dilated inside a window of blocks around them
    cd = sc.cam_dict(cam)
    lo = np.asarray([bx.min(), by.min(), bz.min()]) - 1
    nb = np.asarray([bx.max(), by.max(), bz.max()]) + 2 - lo
    win_origin = tuple(float(origin[a] + voxel * 8 * lo[a]) for a in range(3))
    win_dims = tuple(int(8 * nb[a]) for a in range(3))
    for a in range(3):   # exactness of the window's positions
        idx = np.arange(win_dims[a])
        assert np.array_equal(F(win_origin[a]) + F(voxel) * idx.astype(F), F(origin[a]) + F(voxel) * (idx + 8 * lo[a]).astype(F))
    marked = np.zeros(tuple(nb[::-1]), bool)
    sr.mark(marked, win_origin, voxel, win_dims, trunc, [cd], [depth], [image])
    assert marked.any() and not marked[0].any() and not marked[:, 0].any() and not marked[:, :, 0].any() and not marked[-1].any()
    allocated = sr.dilate(marked, 1)
    wz, wy, wx = np.nonzero(allocated)
    assert np.array_equal(np.sort(((wz + lo[2]) * 512 + (wy + lo[1])) * 512 + (wx + lo[0])), keys.astype(np.int64))
    win_keys = sr.index_of(allocated)[2]   # (the same order: key order is z, y, x order in both)
    # the samples and the mesh: the restatement on the window, cleared outside the allocated blocks
    tw, rgb = tr.new_volume(win_dims, True)
    tr.integrate(tw, rgb, win_origin, voxel, trunc, 64.0, [cd], [depth], [image])
    want_tw, want_rgb = sr.to_pool(tw, rgb, win_keys, win_dims)
    assert (want_tw[..., 1] > 0).sum() > 1000 and (want_tw[..., 0] < 0).any()
    assert np.array_equal(_bits(vol.tw.cpu().numpy()), _bits(want_tw)) and np.array_equal(_bits(vol.rgb.cpu().numpy()), _bits(want_rgb))
    image_tw, image_rgb = sr.to_dense(want_tw, want_rgb, win_keys, win_dims)
    window = vol.to_dense(tuple(int(8 * v) for v in lo), win_dims)
    assert np.array_equal(_bits(window.tw.cpu().numpy()), _bits(image_tw)) and np.array_equal(_bits(window.rgb.cpu().numpy()), _bits(image_rgb))
    want = sr.reorder_mesh(*tr.extract(image_tw, image_rgb, win_origin, voxel), sr.sparse_order(image_tw, win_keys, win_dims))
    v, c, t = vol.extract_mesh()
    v, t = v.cpu().numpy(), _u32(t)
    assert vol.count() == (len(want[0]), len(want[2])) and len(t) > 100
    assert np.array_equal(_bits(v), _bits(want[0])) and np.array_equal(_bits(c.cpu().numpy()), _bits(want[1]))
    assert np.array_equal(tr.canonical(t), tr.canonical(want[2]))
    # the mesh lies in the plane z_camera = 1 to within a voxel
    vm = np.asarray([cam.vm[n] for n in range(12)], np.float64).reshape(4, 3).T
    zc = v.astype(np.float64) @ vm[2, :3] + vm[2, 3]
    print("4096^3: %d vertices, %d triangles, distance from the plane max %.3f voxel" % (len(v), len(t), np.abs(zc - 1.0).max() / voxel))
    assert np.abs(zc - 1.0).max() < voxel


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    import brush_amd as ba
    from brush_amd import _ffi
    lib, h = ctx.lib, ctx._h
    vol = _fuse(ctx, "three", colour=False)
    before = _bits(vol.tw.cpu().numpy()).copy()
    bits_before = _u32(vol.bits).copy()
    cams, depths, _ = sc.views(3)
    d = torch.tensor(depths[0], device=vol.device)
    cfg = _ffi.BhTsdfIntegrateConfig(0.0, math.inf, 0.5, 0)
    one_cam, one_ptr = (_ffi.BhCamera * 1)(cams[0]), (C.c_void_p * 1)(d.data_ptr())
    nv, nt, nb = C.c_uint32(), C.c_uint32(), C.c_uint32(77)

    def pool_entries(v):   # the entry points that need a committed volume
        return [lib.bh_sptsdf_clear(h, C.byref(v)), lib.bh_sptsdf_integrate(h, C.byref(v), 1, one_cam, one_ptr, None, C.byref(cfg)),
                lib.bh_sptsdf_extract_count(h, C.byref(v), C.byref(nv), C.byref(nt)), lib.bh_sptsdf_extract(h, C.byref(v), None, None, None, 0, 0, C.byref(nv), C.byref(nt))]

    def every_entry(v):
        return [lib.bh_sptsdf_mark_clear(h, C.byref(v)), lib.bh_sptsdf_mark(h, C.byref(v), 1, one_cam, one_ptr, None, C.byref(cfg)),
                lib.bh_sptsdf_commit(h, C.byref(v), 1, C.byref(nb))] + pool_entries(v)

    # the volume: a dimension above 8192 or below 2, numbers that are not finite and positive, null index arrays
    for field, value in (("nx", 8193), ("nz", 1), ("ny", 0), ("trunc", 0.0), ("trunc", math.nan), ("voxel_size", -1.0), ("voxel_size", math.inf), ("max_weight", 0.5),
                         ("bits", None), ("rank", None)):
        bad = vol.vol()
        setattr(bad, field, value)
        assert every_entry(bad) == [-1] * 7, field
    # the mark step count: trunc = 129 voxels is M = 65
    bad = vol.vol()
    bad.trunc = 129 * bad.voxel_size
    assert lib.bh_sptsdf_mark(h, C.byref(bad), 1, one_cam, one_ptr, None, C.byref(cfg)) == -1
    assert sr.mark_steps(sc.VOXEL, 129 * F(sc.VOXEL)) == 65 and sr.mark_steps(sc.VOXEL, 128 * F(sc.VOXEL)) == 64
    with pytest.raises(ValueError, match="steps"):
        _sparse(ctx, trunc=129 * sc.VOXEL).mark([d], [cams[0]])
    # too many allocated blocks; before a commit: no blocks, or no pool
    for field, value in (("n_blocks", (2 ** 31 - 1) // 512 + 1), ("n_blocks", 0), ("keys", None), ("tw", None)):
        bad = vol.vol()
        setattr(bad, field, value)
        assert pool_entries(bad) == [-1] * 4, field
        dense = _dense(ctx, colour=False).grid()
        assert lib.bh_sptsdf_to_dense(h, C.byref(bad), 0, 0, 0, C.byref(dense)) == -1
    fresh = _sparse(ctx)
    for call in (fresh.clear, fresh.count, fresh.extract_mesh, fresh.to_ply, fresh.to_dense, lambda: fresh.integrate([d], [cams[0]])):
        with pytest.raises(ValueError, match="commit"):
            call()
    assert fresh.commit() == 0 and fresh.n_blocks == 0   # nothing marked: no pool
    # dilate
    for dilate in (3, 0xFFFFFFFF):
        assert lib.bh_sptsdf_commit(h, C.byref(vol.vol()), dilate, C.byref(nb)) == -1 and nb.value == 77
    for dilate in (-1, 3, 1.5, True):
        with pytest.raises(ValueError, match="dilate"):
            _sparse(ctx).commit(dilate)
    # the views
    for entry in (lib.bh_sptsdf_mark, lib.bh_sptsdf_integrate):
        for change in ("model", "window", "depth", "config"):
            arr = (_ffi.BhCamera * 2)(cams[0], cams[1])
            ptrs = (C.c_void_p * 2)(d.data_ptr(), d.data_ptr())
            if change == "model":
                arr[1].model = _ffi.CAMERA_KANNALA_BRANDT_4
            elif change == "window":
                arr[1].tile_row_begin, arr[1].tile_row_end = 0, 1
            elif change == "depth":
                ptrs[1] = None
            assert entry(h, C.byref(vol.vol()), 2, arr, ptrs, None, C.byref(cfg) if change != "config" else None) == -1, change
    with pytest.raises(ValueError, match="pinhole"):
        vol.integrate([d], [ba.Camera(fov_x=1.0, fov_y=0.8, camera_model="kb4", dist=(0.01, 0.0, 0.0, 0.0))])
    # the dense grid of to_dense
    for field, value in (("tw", None), ("nx", 1)):
        dense = _dense(ctx, colour=False).grid()
        setattr(dense, field, value)
        assert lib.bh_sptsdf_to_dense(h, C.byref(vol.vol()), 0, 0, 0, C.byref(dense)) == -1, field
    # extraction: capacities below the counts (the counts still returned, nothing written), colours from a volume without rgb
    n_v, n_t = vol.count()
    assert n_v > 50 and n_t > 50
    verts = torch.full((n_v, 3), 7.0, device=vol.device)
    tris = torch.full((n_t, 3), 7, dtype=torch.int32, device=vol.device)
    v = vol.vol()
    for cap_v, cap_t in ((n_v - 1, n_t), (n_v, n_t - 1), (0, 0)):
        nv.value = nt.value = 0
        assert lib.bh_sptsdf_extract(h, C.byref(v), verts.data_ptr(), None, tris.data_ptr(), cap_v, cap_t, C.byref(nv), C.byref(nt)) == -1
        assert (nv.value, nt.value) == (n_v, n_t)
    assert (verts == 7.0).all() and (tris == 7).all()
    colours = torch.empty((n_v, 3), device=vol.device)
    assert lib.bh_sptsdf_extract(h, C.byref(v), verts.data_ptr(), colours.data_ptr(), tris.data_ptr(), n_v, n_t, C.byref(nv), C.byref(nt)) == -1
    assert lib.bh_sptsdf_extract(h, C.byref(v), verts.data_ptr(), None, tris.data_ptr(), n_v, n_t, C.byref(nv), C.byref(nt)) == 0
    # nothing above was launched: the pool and the index are as they were
    assert np.array_equal(_bits(vol.tw.cpu().numpy()), before) and np.array_equal(_u32(vol.bits), bits_before)


# ---- 7. PLY ----------------------------------------------------------------------------------------------------------------------
def test_to_ply_is_mesh_to_ply_of_the_extracted_arrays(ctx):
    import brush_amd as ba
    for colour in (True, False):
        vol = _fuse(ctx, "three", colour)
        v, c, t = vol.extract_mesh()
        data = vol.to_ply()
        assert data == ba.mesh_to_ply(v, t, c, ctx=ctx) == tr.mesh_to_ply(v.cpu().numpy(), c.cpu().numpy() if colour else None, _u32(t))
        n_v, vprops, n_t, _ = tgm._read_ply(data)
        assert (n_v, n_t) == (len(v), len(t)) and len(vprops) == (6 if colour else 3)
