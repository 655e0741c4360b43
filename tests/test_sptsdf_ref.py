"""The restatement of the sparse volume (tests/sptsdf_ref.py) against itself and a brute force, without a GPU: rank and select are
mutually inverse, the separable dilation is the Chebyshev ball, the block layout of a ragged grid round-trips through the dense volume,
and — what the GPU's mesh-equality tests stand on — the allocation of mark + commit(1) contains every block that holds a band sample
and its 26 neighbours on both test scenes (tests/sptsdf_cases.py)."""
import numpy as np
import pytest

import sptsdf_cases as sc
import sptsdf_ref as sr
import tsdf_ref as tr

F = np.float32


def test_rank_and_select_are_mutually_inverse():
    rng = np.random.default_rng(2)
    for shape, p in (((4, 5, 5), 0.3), ((3, 7, 11), 0.05), ((1, 1, 33), 0.9), ((2, 3, 4), 0.0), ((5, 8, 8), 1.0)):
        marked = rng.uniform(size=shape) < p
        bits, rank, keys = sr.index_of(marked)
        total = marked.size
        assert len(bits) == len(rank) == (total + 31) // 32 and len(keys) == marked.sum()
        assert (np.diff(keys.astype(np.int64)) > 0).all()
        assert np.array_equal(rank, np.concatenate([[0], np.cumsum([bin(int(w)).count("1") for w in bits])[:-1]]))
        slots = [sr.slot_of(bits, rank, key) for key in range(total)]
        for key in range(total):
            if marked.reshape(-1)[key]:
                assert keys[slots[key]] == key          # select(rank(key)) = key
            else:
                assert slots[key] is None
        assert [slots[int(k)] for k in keys] == list(range(len(keys)))   # rank(select(slot)) = slot
        if total % 32:
            assert int(bits[-1]) >> (total % 32) == 0   # no bit beyond the last block


@pytest.mark.parametrize("r", [0, 1, 2])
def test_dilation_against_a_brute_force(r):
    rng = np.random.default_rng(7 + r)
    for shape in ((4, 5, 5), (1, 6, 9), (7, 2, 3)):
        marked = rng.uniform(size=shape) < 0.04
        marked[0, 0, 0] = marked[-1, -1, -1] = True   # the faces of the grid
        want = np.zeros(shape, bool)
        for z, y, x in zip(*np.nonzero(marked)):
            want[max(z - r, 0):z + r + 1, max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1] = True
        got = sr.dilate(marked, r)
        assert np.array_equal(got, want)
        if r == 0:
            assert np.array_equal(got, marked)


def test_boundary_blocks_of_a_ragged_grid():
    dims = sc.SCENES["three"]["dims"]
    assert dims == (40, 33, 26) and sr.block_dims(dims) == (5, 5, 4) and sr.n_words(dims) == 4
    assert [d - 8 * (n - 1) for d, n in zip(dims, sr.block_dims(dims))] == [8, 1, 2]   # samples the last blocks hold per axis
    rng = np.random.default_rng(4)
    marked = rng.uniform(size=(4, 5, 5)) < 0.5
    marked[3, 4, 4] = True
    _, _, keys = sr.index_of(marked)
    idx = sr.pool_indices(keys, dims)
    assert idx.shape == (26, 33, 40)
    have = idx >= 0
    assert len(np.unique(idx[have])) == have.sum()   # no two samples share a pool entry
    bx, by, bz = sr.block_coords(keys, dims)
    exist = np.minimum(8, 40 - 8 * bx) * np.minimum(8, 33 - 8 * by) * np.minimum(8, 26 - 8 * bz)
    assert have.sum() == exist.sum() and exist[-1] == 8 * 1 * 2
    # a dense volume -> pool -> dense: allocated samples survive bit for bit, the rest is cleared, samples that do not exist stay cleared
    tw = rng.normal(size=(26, 33, 40, 2)).astype(F)
    rgb = rng.uniform(size=(26, 33, 40, 3)).astype(F)
    ptw, prgb = sr.to_pool(tw, rgb, keys, dims)
    assert ptw.shape == (len(keys), 8, 8, 8, 2)
    last = ptw[-1]   # block (4, 4, 3): 8 x 1 x 2 samples
    assert np.array_equal(last[:2, :1, :, :], tw[24:26, 32:33, 32:40]) and (last[2:, :, :, 1] == 0).all() and (last[:, 1:, :, 0] == 1).all()
    back_tw, back_rgb = sr.to_dense(ptw, prgb, keys, dims)
    assert np.array_equal(back_tw[have].view(np.uint32), tw[have].view(np.uint32)) and np.array_equal(back_rgb[have], rgb[have])
    assert (back_tw[~have] == np.asarray([1, 0], F)).all() and (back_rgb[~have] == 0).all()


def test_marking_follows_the_rays_through_the_band():
    s = sc.SCENES["three"]
    assert sr.mark_steps(sc.VOXEL, sc.TRUNC) == 2 and sr.mark_steps(0.1, 0.1 * 4 * 64 / 2) == 64 and sr.mark_steps(0.1, 13.0) == 65
    with_images, without = sc.marked("three"), sc.marked("three", with_images=False)
    assert 0 < with_images.sum() < with_images.size and (without | with_images == without).all()   # the alpha test only removes pixels
    one, two = sc.marked("three", n_views=1), sc.marked("three", n_views=2)
    assert one.sum() < two.sum() <= with_images.sum() and (two | one == two).all()
    # a depth map of zeros, NaN and negatives marks nothing; neither does a surface beyond depth_max
    cams, depths, _ = sc.views(3)
    for depth, kw in ((np.zeros_like(depths[0]), {}), (np.full_like(depths[0], np.nan), {}), (-np.abs(depths[0]), {}), (depths[0], dict(depth_max=0.5))):
        m = np.zeros(with_images.shape, bool)
        sr.mark(m, s["origin"], sc.VOXEL, s["dims"], sc.TRUNC, [sc.cam_dict(cams[0])], [depth], **kw)
        assert not m.any()


@pytest.mark.parametrize("name", ["three", "sphere"])
def test_the_allocation_contains_the_band_and_its_neighbours(name):
    """Measured (and asserted: it holds on both scenes, so both stay in the GPU's mesh-equality tests): on the three-view scene 18 of
    100 blocks are marked, 60 are needed (a band sample or a neighbour of one) and 64 allocated with dilate = 1; on the sphere scene
    14 of 18 are marked and all 18 needed and allocated.  A pixel is about half a voxel wide here, far below a block."""
    needed, allocated = sc.containment(name)
    marked = sc.marked(name)
    print("%s: %d of %d blocks marked, %d needed, %d allocated, %d needed but not allocated" % (name, marked.sum(), marked.size, needed.sum(), allocated.sum(),
                                                                                           (needed & ~allocated).sum()))
    assert needed.any() and not (needed & ~allocated).any()
    assert (marked.sum(), needed.sum(), allocated.sum()) == {"three": (18, 60, 64), "sphere": (14, 18, 18)}[name]
    # ... hence the mesh of the sparse volume's dense image is the mesh of dense fusion
    tw, rgb = sc.fused(name)
    _, _, keys = sr.index_of(allocated)
    s = sc.SCENES[name]
    sparse_tw, sparse_rgb = sr.to_dense(*sr.to_pool(tw, rgb, keys, s["dims"]), keys, s["dims"])
    a, b = tr.extract(tw, rgb, s["origin"], sc.VOXEL), tr.extract(sparse_tw, sparse_rgb, s["origin"], sc.VOXEL)
    assert len(a[2]) > 100 and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
