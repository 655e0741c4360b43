"""The radix sorts without their row-scan launch (sort.hip, depth_sort.hip): a scatter block finds its offsets by adding up the
totals of the groups of SORT_GROUP_BLOCKS (= 32) histogram blocks in front of its own group and the histograms of the earlier
blocks of its own group.  That sum can go wrong at a block edge, at a group edge and in the first block of a later group, and
the group tables are accumulated by atomics into memory that the sort BEFORE on the same context has to leave zero — so the
sizes sit at those seams, and every case runs on a context that has just sorted something of another size.  Sorts of more than
SORT_DIRECT_GROUPS (= 32) groups take another path — a scan launch over the group table, the scatter blocks read prefixes — so
the largest sort without it and the smallest with it are cases too.  numpy is the checker: argsort(kind="stable"), cumsum of the gathered counts, searchsorted for the offsets table."""
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import util

pytestmark = pytest.mark.gpu

G = 32                    # context.h SORT_GROUP_BLOCKS
DIRECT = 32               # context.h SORT_DIRECT_GROUPS: more groups than this and the group table is scanned by a launch
DS_CHUNK = 2048           # depth_sort.hip DS_TILE: keys per histogram block of the depth sort
W, H = 320, 176


def _dev_u32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)


# ---- depth sort (through the forward: its only entry point) ---------------------------------------------------------------------
def _depth_scene(n, seed, kind):
    """n splats in front of the identity camera of synth.default_camera_params (depth == z, exactly); the depth keys of splats
    behind the camera or off the image are the culled key."""
    rng = np.random.default_rng(seed)
    sc = synth.make_scene(n, seed, sh_degree=0, log_scale_range=(math.log(0.004), math.log(0.02)))
    t = sc["transforms"]
    z0 = t[:, 2].copy()
    if kind == "half_culled":
        z = np.where(rng.random(n) < 0.5, z0, -z0).astype(np.float32)
    elif kind == "all_culled":
        z = -z0
    elif kind == "all_equal":
        z = np.full(n, 5.0, np.float32)
    elif kind == "thin_shell":    # 97 % of the keys within 1 % of one depth
        z = np.where(rng.random(n) < 0.97, 6.0 + rng.random(n) * 0.06, 2.0 + rng.random(n) * 10.0).astype(np.float32)
    else:
        raise ValueError(kind)
    f = np.abs(z) / z0
    t[:, 0] *= f
    t[:, 1] *= f
    t[:, 2] = z
    return sc


def _check_depth_order(ba, ctx, dev, sc, what):
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    cam = util.hip_camera(ba, synth.default_camera_params(W, H))
    _, aux = ba.render_splats(spl, cam, (W, H), (0, 0, 0), ba.RasterPass.Backward, ctx=ctx)
    nv = aux.num_visible
    gfc = util.u32(aux.global_from_compact_gid)[:nv].astype(np.int64)
    z = sc["transforms"][:, 2]
    ids = np.sort(gfc)
    assert ids.size == nv and (nv == 0 or np.all(np.diff(ids) > 0)), what + ": the order is not a permutation of the visible ids"
    assert np.all(z[ids] > 0), what
    # positive floats order as their bit patterns: the key the sort sees
    want = ids[np.argsort(z[ids].view(np.uint32), kind="stable")]
    assert np.array_equal(gfc, want), what + ": order"
    assert np.array_equal(aux.depths_sorted.cpu().numpy()[:nv], z[want]), what + ": sorted depths"
    counts = util.u32(aux.intersect_counts).astype(np.int64)
    assert np.array_equal(util.u32(aux.cum_tiles_hit)[:nv].astype(np.int64), np.cumsum(counts[want])), what + ": cum_tiles_hit"
    assert nv == 0 or int(np.cumsum(counts[want])[-1]) == aux.num_intersections, what
    return nv


DEPTH_SIZES = [1, DS_CHUNK - 1, DS_CHUNK, DS_CHUNK + 1, G * DS_CHUNK - 1, G * DS_CHUNK, G * DS_CHUNK + 1, 3 * G * DS_CHUNK + 5,
               DIRECT * G * DS_CHUNK, DIRECT * G * DS_CHUNK + 1]   # (the last two: 32 groups, and a 33rd of one key)


@pytest.fixture(scope="module")
def depth_ctx(dev):
    import brush_amd as ba
    ctx = ba.Context(dev)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("n", DEPTH_SIZES[::-1] + [DS_CHUNK + 1])   # (descending, then a small one again: a short sort behind a long one)
def test_depth_sort_at_block_and_group_edges(dev, depth_ctx, n):
    import brush_amd as ba
    nv = _check_depth_order(ba, depth_ctx, dev, _depth_scene(n, 0x900 + n % 251, "half_culled"), "n=%d" % n)
    assert n < 64 or 0 < nv < n


@pytest.mark.parametrize("kind", ["all_culled", "all_equal"])
def test_depth_sort_degenerate_keys(dev, depth_ctx, kind):
    import brush_amd as ba
    n = G * DS_CHUNK + 1
    nv = _check_depth_order(ba, depth_ctx, dev, _depth_scene(n, 0x77, kind), kind)
    assert (nv == 0) == (kind == "all_culled")


def test_depth_sort_thin_shell_two_frames_on_one_context(dev):
    """A fresh context: the first frame sorts a sample first (>= 131072 splats, no splitter table yet), the second splits at the
    first's quantiles — the same paths as before the group sums; a third frame of another size follows on the same tables."""
    import brush_amd as ba
    n = 3 * G * DS_CHUNK + 5
    assert n >= 131072
    sc = _depth_scene(n, 0x51, "thin_shell")
    ctx = ba.Context(dev)
    try:
        a = _check_depth_order(ba, ctx, dev, sc, "thin shell, first frame")
        b = _check_depth_order(ba, ctx, dev, sc, "thin shell, second frame")
        assert a == b and a > n // 4
        _check_depth_order(ba, ctx, dev, _depth_scene(G * DS_CHUNK, 0x52, "half_culled"), "behind the thin shell")
    finally:
        ctx.close()


# ---- generic argsort -------------------------------------------------------------------------------------------------------------
SORT_SIZES = [1, 4095, 4096, 4097, G * 2048 + 1, G * 4096 + 1, 3 * G * 4096 + 7,
              DIRECT * G * 4096, DIRECT * G * 4096 + 1]   # (4096-key blocks beyond 2 M keys: 32 groups, and a 33rd of one key)


@pytest.fixture(scope="module")
def sort_ctx(dev):
    import brush_amd as ba
    ctx = ba.Context(dev)
    yield ctx
    ctx.close()


def _check_argsort(ba, ctx, dev, n, bits, seed):
    rng = np.random.default_rng(seed)
    # many ties in the sorted bits, garbage above them (the contract: only the low `bits` bits order the pairs)
    low = rng.integers(0, 41, n, dtype=np.uint64) * np.uint64((2 ** bits - 1) // 41)
    high = rng.integers(0, 2 ** 32, n, dtype=np.uint64) << np.uint64(bits)
    keys = ((low | high) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    vals = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    ok, ov = ba.radix_argsort(_dev_u32(keys, dev), _dev_u32(vals, dev), bits, ctx=ctx)
    mask = np.uint32(0xFFFFFFFF if bits == 32 else (1 << bits) - 1)
    idx = np.argsort(keys & mask, kind="stable")
    assert np.array_equal(util.u32(ok), keys[idx]), "keys (n=%d, bits=%d)" % (n, bits)
    assert np.array_equal(util.u32(ov), vals[idx]), "values (n=%d, bits=%d)" % (n, bits)


@pytest.mark.parametrize("bits", [8, 13, 32])
@pytest.mark.parametrize("n", SORT_SIZES[::-1])
def test_argsort_at_block_and_group_edges(dev, sort_ctx, n, bits):
    """(consecutive cases share one context: every sort runs behind one of another size, and a 32-bit sort is four passes that
    hand the group tables on to each other)"""
    import brush_amd as ba
    _check_argsort(ba, sort_ctx, dev, n, bits, n * 31 + bits)
    _check_argsort(ba, sort_ctx, dev, max(1, n // 3), bits, n * 37 + bits)


# ---- tile sort + offsets ---------------------------------------------------------------------------------------------------------
def _check_tile_sort(ba, ctx, dev, n, hot, seed):
    num_tiles = 8160   # 13-bit tile ids
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, num_tiles, n).astype(np.uint32)
    if hot:
        keys = np.where(rng.random(n) < 0.6, 4000 + rng.integers(0, 32, n), keys).astype(np.uint32)
    vals = np.arange(n, dtype=np.uint32)   # pairs in depth order: the value is the pair's rank
    ok, ov, offs = ba.tile_sort_offsets(_dev_u32(keys, dev), _dev_u32(vals, dev), num_tiles, ctx=ctx)
    idx = np.argsort(keys, kind="stable")
    sk = keys[idx]
    assert np.array_equal(util.u32(ok), sk) and np.array_equal(util.u32(ov), vals[idx]), "order (n=%d)" % n
    tiles = np.arange(num_tiles, dtype=np.uint32)
    begin, end = np.searchsorted(sk, tiles, side="left"), np.searchsorted(sk, tiles, side="right")
    want = np.stack([np.where(end > begin, begin, 0), np.where(end > begin, end, 0)], axis=1).astype(np.uint32)   # absent tiles: (0, 0)
    assert np.array_equal(util.u32(offs).reshape(-1, 2), want), "offsets (n=%d)" % n


@pytest.mark.parametrize("hot", [False, True])
@pytest.mark.parametrize("n", [DIRECT * G * 4096 + 1, DIRECT * G * 4096, 300_000, G * 4096 + 1, G * 2048 + 1, 4096, 1, 0])
def test_tile_sort_offsets_at_group_edges(dev, sort_ctx, n, hot):
    import brush_amd as ba
    _check_tile_sort(ba, sort_ctx, dev, n, hot, n + 17 * hot)


# ---- device-side length ----------------------------------------------------------------------------------------------------------
def _render_exact_and_sliced(ba, ctx, spl, cam, size, bg, share):
    img_e, aux_e = ba.render_splats(spl, cam, size, bg, ba.RasterPass.Backward, ctx=ctx)
    ba.host.set_list_slicing(share, ctx)
    try:
        img_s, aux_s = ba.render_splats(spl, cam, size, bg, ba.RasterPass.Backward, ctx=ctx, sliced=True)
        near, far = ba.host.last_list_counts(ctx)
    finally:
        ba.host.set_list_slicing(0.0, ctx)
    return img_e, aux_e, img_s, aux_s, near, far


# (splats, image side, pairs the frame must exceed): several groups of 2048-pair blocks, sorted directly; and more than 32 groups
# of 4096-pair blocks, the scanned path
DEV_SCENES = [(100_000, 512, 3 * G * 2048), (520_000, 1024, DIRECT * G * 4096)]


@pytest.mark.parametrize("opacity", [(0.02, 0.1), (0.9, 0.99)], ids=["translucent", "opaque"])
@pytest.mark.parametrize("n,side,min_pairs", DEV_SCENES)
def test_device_length_sort_then_a_plain_sort(dev, n, side, min_pairs, opacity):
    """No hook exposes the device-side length, so: a depth-sliced forward.  Its far slice sorts with a bound of ALL the frame's
    pairs (the grid, the block table and the group count are sized for it) and a live count of what the near slice left
    unfinished: the live blocks end groups before the bound's last group, whose rows stay zero.  The opaque scene saturates every
    tile in the near slice and the gate switches the far sort off (far == 0).  Blending is order-dependent float arithmetic, so a
    bit-identical image with the same visible flags pins the far lists' order; a plain sort on the same context behind it
    finds clean group tables."""
    import brush_amd as ba
    sc = synth.make_scene(n, 0x5B, sh_degree=0, log_scale_range=(math.log(0.02), math.log(0.1)), opacity_range=opacity)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    cam = util.hip_camera(ba, synth.default_camera_params(side, side))
    ctx = ba.Context(dev)
    try:
        img_e, aux_e, img_s, aux_s, near, far = _render_exact_and_sliced(ba, ctx, spl, cam, (side, side), (0.1, 0.3, 0.2), 0.33)
        ni = aux_e.num_intersections
        print("pairs %d, near %d, far %d" % (ni, near, far))
        assert ni > min_pairs
        assert aux_s.num_visible == aux_e.num_visible and aux_s.num_intersections == ni
        if opacity[0] > 0.5:
            assert far == 0, "the gate did not switch the far sort off"
        else:
            assert 0 < far < ni - ni // 4, "the far sort's live count is not well below its bound"
        assert torch.equal(img_e, img_s), "image differs: max %g" % float((img_e.float() - img_s.float()).abs().max())
        assert torch.equal(aux_e.visible, aux_s.visible)
        _check_argsort(ba, ctx, dev, G * 2048 + 1, 13, 5)
        _check_tile_sort(ba, ctx, dev, G * 2048 + 1, False, 6)
    finally:
        ctx.close()
