"""Mask lifting on the GPU (include/brush_hip_lift.h).

A. Bit identity with the library's own forward weights.  bh_render_features folds a channel with one fmaf(f, w, acc), so with
   `features` an identity block (rows [b, b + 256) = I_256, zero elsewhere) the map [H,W,256] IS w_ip of those splats; blocks of 256
   rows give every weight, tests/lift_ref.py::votes_from_weights turns them into tables, and votes, max_weight and pixel_count must
   be EQUAL to the library's.
B. Against the float64 renderer (tests/feature_ref.py), tie pixels labelled 255.  Bound 1e-4 of the largest summed weight (the
   project's gradient-grade TOL; the feature maps measured 2.7e-6 against the same reference).
C. The same bits from two calls, complete and cut lists, near + far lists, a retained node, two tile-row windows, both band modes.
D. Against the route the parent offered: v_features of a feature backward with a one-hot cotangent.
E. Edges and refusals.   F. assign / select / compact_splats against the restatement, exactly.   G. Two objects end to end.
H. Lift calls between train steps change nothing.

Measured on an MI355X: B within 1.16e-5 of a largest summed weight of 193 (6.0e-8 of it) over the eight cases, tie
pixels 3 / 4 / 0 / 8; D within 1.16e-5 of 118.6 (9.8e-8); the 43 cases take 5 s together, none above 0.5 s."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import depth_ref
import lift_ref as lr
import util

pytestmark = pytest.mark.gpu
TOL = 1e-4   # the project's gradient-grade figure
REF_CASES = [("pinhole", False), ("pinhole", True), ("kb4", False), ("kb4", True)]
ALL_MODES = [(s, mip, m) for s in (False, True) for mip in (False, True) for m in ("pinhole", "kb4")]
# every mode at the largest N, two complementary ones at the others; both image sizes everywhere (33 x 17: partial tiles on both edges)
IDENTITY_CASES = [(600, size, *mode) for size in ((64, 48), (33, 17)) for mode in ALL_MODES] + \
                 [(n, size, *mode) for n in (1, 63, 256) for size in ((64, 48), (33, 17)) for mode in ((False, False, "pinhole"), (True, True, "kb4"))]


def _pass(ba, smooth):
    return ba.RasterPass.BackwardSmoothCutoff if smooth else ba.RasterPass.Backward


def _scene(n, w, h, seed, model="pinhole", z_range=(2.0, 9.0), scales=(0.2, 0.8), opacity=(0.03, 0.3)):
    """Large, faint splats: long lists that are walked far (few pixels saturate early)."""
    cp = {k: v for k, v in synth.default_camera_params(w, h).items() if k not in ("img_w", "img_h")}
    tans = (math.tan(cp["fov_x"] / 2.0), math.tan(cp["fov_y"] / 2.0))
    sc = synth.make_scene(n, seed, sh_degree=0, log_scale_range=(math.log(scales[0]), math.log(scales[1])), z_range=z_range, tan_half_fov=tans,
                          opacity_range=opacity)
    if model != "pinhole":
        cp["model"], cp["dist"] = util.REF_LENSES[model]
    return sc, cp


def _xy(w, h, L):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx + 3 * yy) % L).astype(np.uint8)


def _blocks(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx // 16 + 2 * (yy // 16)) % 4).astype(np.uint8)


def _with_holes(lab, L):
    out = lab.copy()
    out[::5, ::7] = 255
    out[1::6, 2::5] = L          # the first value that is no label
    out[2::7, 1::6] = 200        # something in [L, 255)
    return out


def _label_maps(w, h):
    """[(name, labels or None, L)]"""
    maps = [("none", None, 1), ("constant", np.full((h, w), 2, np.uint8), 3), ("blocks", _blocks(w, h), 4), ("holes", _with_holes(_xy(w, h, 5), 5), 5),
            ("all ignored", np.full((h, w), 255, np.uint8), 2)]
    return maps + [("xy%d" % L, _xy(w, h, L), L) for L in (1, 2, 5, 17, 256)]


def _gpu_weights(node, n, dev):
    """w [N,H,W] f32 of the node through bh_render_features with identity blocks: bit for bit what the blend multiplied in."""
    w, h = node.img_size
    out = torch.zeros((n, h, w), device=dev)
    for b in range(0, n, 256):
        rows = min(256, n - b)
        f = torch.zeros((n, 256), device=dev)
        f[b:b + rows, :rows] = torch.eye(rows, device=dev)
        out[b:b + rows] = node.features(f)[..., :rows].permute(2, 0, 1)
    return out.cpu().numpy()


def _list_lengths(node, dev):
    from brush_amd import host
    w, h = node.img_size
    tiles = ((w + 15) // 16) * ((h + 15) // 16)
    to = host._view(node.out.tile_offsets, (tiles, 2), torch.int32, dev).cpu().numpy().astype(np.int64)
    length = to[:, 1] - to[:, 0]
    if node.out.tile_offsets_far:
        far = host._view(node.out.tile_offsets_far, (tiles, 2), torch.int32, dev).cpu().numpy().astype(np.int64)
        length = length + far[:, 1] - far[:, 0]
    return length


def _tables(acc):
    return acc.votes.cpu().numpy(), acc.max_weight.cpu().numpy(), acc.pixel_count.cpu().numpy().astype(np.int64)


def _dev_labels(lab, dev):
    return None if lab is None else torch.from_numpy(lab).to(dev)


def _equal_tables(acc, want, what):
    votes, wmax, count = _tables(acc)
    assert np.array_equal(votes, want[0]), (what, "votes", int(np.abs(votes - want[0]).max()))
    assert np.array_equal(wmax.view(np.uint32), np.asarray(want[1], np.float32).view(np.uint32)), (what, "max_weight")
    assert np.array_equal(count, want[2]), (what, "pixel_count")


# ---- A. bit identity with the forward's own weights ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,size,smooth,mip,model", [pytest.param(*c, id="N%d-%dx%d-%s%s-%s" % (c[0], c[1][0], c[1][1], "smooth" if c[2] else "hard", "-mip" if c[3] else "", c[4]))
                                                     for c in IDENTITY_CASES])
def test_tables_equal_the_forward_weights_bit_for_bit(dev, n, size, smooth, mip, model):
    import brush_amd as ba
    w, h = size
    # (256 splats put more than 128 into one tile only when they are large: 189 .. 224 listed at these scales, 275 .. 444 of the 600)
    sc, cp = _scene(n, w, h, 0xA0 + n, model, scales=(0.2, 0.8) if n > 256 else (0.5, 1.5))
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], render_mip=mip, device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), pass_=_pass(ba, smooth), ctx=ctx)
        if n >= 256:
            assert int(_list_lengths(node, dev).max()) > 128, "no tile stages more than two batches"
        weights = _gpu_weights(node, n, dev)
        assert float(weights.max()) > (0.0 if n == 1 else 0.02) and float(weights.max()) <= 0.999
        for name, lab, L in _label_maps(w, h):
            want = lr.votes_from_weights(weights, lab, L)
            acc = ba.LiftAccumulator(n, L, dev, ctx=ctx).add(node, _dev_labels(lab, dev))
            _equal_tables(acc, want, name)
            if name in ("holes", "xy17"):   # without the statistics: the other instantiation, the same votes
                bare = ba.LiftAccumulator(n, L, dev, stats=False, ctx=ctx).add(node, _dev_labels(lab, dev))
                assert bare.max_weight is None and np.array_equal(bare.votes.cpu().numpy(), want[0]), name
            if name == "xy5":
                assert int((want[0] > 0).sum()) > (0 if n == 1 else n), "the case votes"
                # a second view of the same frame: votes and counts double, the maximum stays
                acc.add(node, _dev_labels(lab, dev))
                _equal_tables(acc, (2 * want[0], want[1], 2 * want[2]), "added twice")
                assert np.array_equal(acc.weights().cpu().numpy(), (2 * want[0] / lr.VOTE_ONE).astype(np.float32))
    finally:
        ctx.close()


# ---- B. against the float64 renderer --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smooth", [False, True], ids=["hard", "smooth"])
@pytest.mark.parametrize("model,mip", REF_CASES)
def test_against_the_float64_reference(dev, model, mip, smooth):
    import brush_amd as ba
    sc, cp, w, h, ref = lr.reference(model, mip, smooth)
    tie = depth_ref.tie_mask(ref, "accumulated").numpy()
    assert int(tie.sum()) <= 15, int(tie.sum())   # 0.5 % of 3072; recorded for these cases: 3 / 4 / 0 / 8
    L = 5
    lab = _xy(w, h, L)
    lab[tie] = 255   # tie pixels vote nowhere, here and there
    vis = ref["vis"].numpy()
    n = vis.shape[0]
    want = np.stack([(vis * (lab == l)[None]).reshape(n, -1).sum(axis=1) for l in range(L)], axis=1)
    scale = float(vis.reshape(n, -1).sum(axis=1).max())
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], render_mip=mip, device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), pass_=_pass(ba, smooth), ctx=ctx)
        acc = ba.LiftAccumulator(n, L, dev, ctx=ctx).add(node, torch.from_numpy(lab).to(dev))
        got = acc.votes.cpu().numpy().astype(np.float64) / lr.VOTE_ONE
        err = float(np.abs(got - want).max())
        print("%s mip=%d smooth=%d: max |votes / 2^24 - sum of vis| = %.3e = %.3e of the largest summed weight %.3f, %d tie pixels"
              % (model, mip, smooth, err, err / scale, scale, int(tie.sum())))
        assert err <= TOL * scale, (err, scale)
        # the statistics, where no tie pixel can move them: a splat's maximum over the non-tie pixels is a lower bound
        ref_max = (vis * ~tie[None]).reshape(n, -1).max(axis=1)
        assert (acc.max_weight.cpu().numpy() >= ref_max - TOL).all()
    finally:
        ctx.close()


# ---- C. invariance --------------------------------------------------------------------------------------------------------------
def test_tables_do_not_depend_on_the_list_policy_the_call_or_the_tile_order(dev):
    import brush_amd as ba
    n, w, h, L = 60000, 320, 208, 5
    cp = synth.default_camera_params(w, h)
    tans = (math.tan(cp["fov_x"] / 2.0), math.tan(cp["fov_y"] / 2.0))
    sc = synth.make_scene(n, 0x56, sh_degree=0, log_scale_range=(math.log(0.03), math.log(0.3)), tan_half_fov=tans)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    cam = util.hip_camera(ba, cp)
    lab = torch.from_numpy(_with_holes(_xy(w, h, L), L)).to(dev)
    ctx = ba.Context(dev)

    def lifted(node, labels=lab):
        return ba.LiftAccumulator(n, L, dev, ctx=ctx).add(node, labels)

    def same(a, b, what):
        for x, y, name in ((a.votes, b.votes, "votes"), (a.max_weight.view(torch.int32), b.max_weight.view(torch.int32), "max_weight"), (a.pixel_count, b.pixel_count, "pixel_count")):
            assert torch.equal(x, y), (what, name)

    try:
        base = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx)
        want = lifted(base)
        assert int((want.votes > 0).sum()) > 2000 and int(want.pixel_count.sum()) > 20000
        same(lifted(base), want, "two calls into zeroed tables")
        for mode in (0, 1):
            ctx.set_option("band_mode", mode)
            same(lifted(ba.render_splats_diff(spl, cam, (w, h), ctx=ctx)), want, "band_mode %d" % mode)
        ctx.set_option("band_mode", 1)
        # per-tile cut lists: the second sliced frame of a view
        ba.set_view_id(0xFE, ctx)
        first = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
        assert first.out.tile_offsets_far is None or first.out.list_budget == first.out.num_intersections
        cut = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
        assert cut.out.tile_offsets_far and cut.out.num_listed_splats < cut.out.num_visible, "not a cut frame"
        same(lifted(cut), want, "cut lists")
        # a near + far frame with a fixed near share
        ba.set_view_id(0, ctx)
        ba.host.set_list_slicing(0.5, ctx)
        try:
            half = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, sliced=True)
            assert half.out.tile_offsets_far
            same(lifted(half), want, "near + far")
        finally:
            ba.host.set_list_slicing(0.0, ctx)
        # a retained forward, after another forward has run
        kept = ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, retain=True)
        other = dict(cp)
        other["pos"] = (1.0, -0.2, -1.0)
        ba.render_splats(spl, util.hip_camera(ba, other), (w, h), (0, 0, 0), ba.RasterPass.Backward, ctx=ctx, copy=False)
        same(lifted(kept), want, "retained")
        kept.release()
        # two tile-row windows accumulated one after the other
        rows = (h + 15) // 16
        acc = ba.LiftAccumulator(n, L, dev, ctx=ctx)
        for win in ((0, 5), (5, rows)):
            acc.add(ba.render_splats_diff(spl, cam, (w, h), ctx=ctx, tile_rows=win), lab)
        same(acc, want, "windows")
    finally:
        ctx.close()


# ---- D. against the parent's route ----------------------------------------------------------------------------------------------
def test_votes_match_the_one_hot_feature_backward(dev):
    import brush_amd as ba
    n, w, h, L = 3000, 123, 82, 5
    sc, cp = _scene(n, w, h, 0xD2, scales=(0.03, 0.3), opacity=(0.05, 0.95))
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    lab = _xy(w, h, L)
    onehot = torch.from_numpy(np.eye(L, dtype=np.float32)[lab]).to(dev).contiguous()
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), ctx=ctx)
        want = node.backward(None, v_features=onehot, features=torch.zeros((n, L), device=dev))["v_features"].cpu().numpy().astype(np.float64)
        got = ba.LiftAccumulator(n, L, dev, ctx=ctx).add(node, torch.from_numpy(lab).to(dev)).votes.cpu().numpy().astype(np.float64) / lr.VOTE_ONE
        assert float(want.max()) > 1.0
        err = float(np.abs(got - want).max())
        print("votes / 2^24 against v_features of the one-hot backward: max |diff| = %.3e of %.3f" % (err, float(want.max())))
        assert err <= TOL * float(want.max())
    finally:
        ctx.close()


# ---- E. edges -------------------------------------------------------------------------------------------------------------------
def test_a_frame_that_lists_nothing_and_unlisted_splats(dev):
    import brush_amd as ba
    from brush_amd import host
    n, w, h, L = 3000, 123, 82, 3
    sc, cp = _scene(n, w, h, 0xD2, scales=(0.03, 0.3), opacity=(0.05, 0.95))
    tr = sc["transforms"].copy()
    tr[-50:, 2] = -tr[-50:, 2]   # behind the camera: never listed
    spl = ba.Splats(tr, sc["sh"], sc["raw_opac"], device=dev)
    lab = _xy(w, h, L)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), ctx=ctx)
        gid = host._view(node.out.global_from_compact_gid, (node.out.num_listed_splats,), torch.int32, dev).long()
        unlisted = torch.ones(n, dtype=torch.bool, device=dev)
        unlisted[gid] = False
        assert bool(unlisted[-50:].all()) and int((~unlisted).sum()) > 100
        weights = _gpu_weights(node, n, dev)
        votes, wmax, count = lr.votes_from_weights(weights, lab, L)
        # the tables are added to, max-ed into, and rows of unlisted splats keep every bit
        acc = ba.LiftAccumulator(n, L, dev, ctx=ctx)
        pre_v = (torch.arange(n * L, dtype=torch.int64, device=dev).view(n, L) * 7 + 3)
        acc.votes.copy_(pre_v)
        acc.max_weight.fill_(0.01)
        acc.pixel_count.fill_(3)
        acc.add(node, torch.from_numpy(lab).to(dev))
        _equal_tables(acc, (pre_v.cpu().numpy() + votes, np.maximum(wmax, np.float32(0.01)), count + 3), "prefilled")
        u = unlisted.cpu().numpy()
        assert (votes[u] == 0).all() and int((wmax > 0.01).sum()) > 100
        # a camera that looks away: nothing is listed, the tables stay as they were
        away = dict(cp)
        away["rot_xyzw"] = util.quat_from_axis_angle((0.0, 1.0, 0.0), math.pi)
        spl2 = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
        empty = ba.render_splats_diff(spl2, util.hip_camera(ba, away), (w, h), ctx=ctx)
        assert empty.out.num_intersections == 0
        before = [t.clone() for t in (acc.votes, acc.max_weight, acc.pixel_count)]
        acc.add(empty, torch.from_numpy(lab).to(dev))
        for a, b in zip(before, (acc.votes, acc.max_weight, acc.pixel_count)):
            assert torch.equal(a, b)
    finally:
        ctx.close()


def test_refusals(dev):
    import brush_amd as ba
    from brush_amd import host, _ffi
    sc = util.base_scene()
    cam = util.hip_camera(ba, util.STD_CAM)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, cam, (32, 32), ctx=ctx)
        buf = torch.zeros(4096, dtype=torch.int64, device=dev)   # room for every table of 4 splats
        at = lambda off: C.c_void_p(buf.data_ptr() + off)
        lab = torch.zeros((32, 32), dtype=torch.uint8, device=dev)
        pl = C.c_void_p(lab.data_ptr())
        err = lambda: ctx.lib.bh_last_error(ctx._h)
        lift = lambda saved, labels, L, v, m, c: ctx.lib.bh_lift_accumulate(ctx._h, saved, labels, L, v, m, c)
        out = C.byref(node.out)
        assert lift(out, pl, 2, at(0), at(1024), at(2048)) == 0
        assert lift(None, pl, 2, at(0), None, None) == -1 and b"null" in err()
        assert lift(out, pl, 2, None, at(1024), None) == -1 and b"null" in err()
        assert lift(out, pl, 0, at(0), None, None) == -1 and b"num_labels" in err()
        assert lift(out, pl, 257, at(0), None, None) == -1 and b"num_labels" in err()
        # overlaps: votes [4,2] u64 = 64 bytes at 0
        assert lift(out, pl, 2, at(0), at(60), None) == -1 and b"overlaps" in err()
        assert lift(out, pl, 2, at(0), at(64), at(76)) == -1 and b"overlaps" in err()
        assert lift(out, pl, 2, at(0), None, at(0)) == -1 and b"overlaps" in err()
        assert lift(out, pl, 2, C.c_void_p(lab.data_ptr() + 1000), None, None) == -1 and b"overlaps" in err()
        assert lift(out, pl, 2, at(0), at(64), at(80)) == 0   # adjacent is fine
        # assign and select
        assert ctx.lib.bh_lift_assign(ctx._h, None, 4, 2, 0.0, at(512), None) == -1 and b"null" in err()
        assert ctx.lib.bh_lift_assign(ctx._h, at(0), 4, 0, 0.0, at(512), None) == -1 and b"num_labels" in err()
        assert ctx.lib.bh_lift_assign(ctx._h, at(0), 4, 257, 0.0, at(512), None) == -1 and b"num_labels" in err()
        sel = lambda **kw: C.byref(_ffi.BhLiftSelect(**dict(dict(label=_ffi.LIFT_ANY_LABEL), **kw)))
        select = lambda v, m, c, s: ctx.lib.bh_lift_select(ctx._h, v, m, c, 4, 2, s, at(512))
        assert select(at(0), at(64), at(80), sel(label=1, min_max_weight=0.1, min_pixels=1)) == 0
        assert select(None, None, None, sel()) == 0
        assert select(None, at(64), at(80), sel(label=1)) == -1 and b"votes" in err()
        assert select(None, at(64), at(80), sel(min_weight=0.5)) == -1 and b"votes" in err()
        assert select(at(0), None, at(80), sel(min_max_weight=0.5)) == -1 and b"max_weight" in err()
        assert select(at(0), at(64), None, sel(min_pixels=1)) == -1 and b"pixel_count" in err()
        assert select(at(0), at(64), at(80), sel(label=2)) == -1 and b"label" in err()
        assert select(at(0), at(64), at(80), sel(min_share=math.nan)) == -1 and b"not a number" in err()
        assert select(at(0), at(64), at(80), None) == -1 and b"null" in err()
        with pytest.raises(ba.BrushHipError, match="num_labels"):
            ba.LiftAccumulator(4, 257, dev, ctx=ctx)
        with pytest.raises(ba.BrushHipError, match="labels must be"):
            ba.LiftAccumulator(4, 2, dev, ctx=ctx).add(node, torch.zeros((32, 31), dtype=torch.uint8, device=dev))
        with pytest.raises(ba.BrushHipError, match="tables hold"):
            ba.LiftAccumulator(5, 2, dev, ctx=ctx).add(node)
        # a forward-only frame: BH_ERR_INVALID_ARG, as the maps'
        _, fwd, _ = host._forward(ctx, spl, cam, (32, 32), (0, 0, 0), ba.RasterPass.Forward)
        assert lift(C.byref(fwd), pl, 2, at(0), None, None) == -1 and b"BWD_INFO" in err()
        # a stale BhRenderOut: another forward has run since (BH_ERR_STATE)
        assert lift(out, pl, 2, at(0), None, None) == -4 and b"stale" in err()
        with pytest.raises(ba.BrushHipError, match="stale"):
            ba.LiftAccumulator(4, 2, dev, ctx=ctx).add(node)
    finally:
        ctx.close()


# ---- F. assign / select / compact_splats ----------------------------------------------------------------------------------------
def test_assign_select_and_compact_equal_the_restatement(dev):
    import brush_amd as ba
    n, w, h, L = 600, 64, 48, 5
    sc, cp = _scene(n, w, h, 0xF1)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), ctx=ctx)
        acc = ba.LiftAccumulator(n, L, dev, ctx=ctx).add(node, torch.from_numpy(_with_holes(_xy(w, h, L), L)).to(dev))
        # rows made by hand: zeros, ties, totals next to a threshold of one unit of weight
        hand = torch.tensor([[0, 0, 0, 0, 0], [5, 9, 9, 0, 1], [7, 7, 7, 7, 7], [lr.VOTE_ONE, 0, 0, 0, 0], [0, 0, lr.VOTE_ONE - 1, 0, 0],
                             [1, 0, 0, 0, lr.VOTE_ONE - 1], [0, 0, 0, 3, 3]], dtype=torch.int64, device=dev)
        acc.votes[:hand.shape[0]] = hand
        votes, wmax, count = _tables(acc)
        assert int((votes.sum(axis=1) >= lr.VOTE_ONE).sum()) > 20 and int((votes.sum(axis=1) == 0).sum()) >= 1
        for mw in (0.0, 1.0, float(np.float32(1.0 - 2.0 ** -24)), 0.37, 1e9):
            want_l, want_s = lr.assign(votes, mw)
            got_l, got_s = acc.assign(min_weight=mw, return_share=True)
            assert np.array_equal(got_l.cpu().numpy(), want_l), mw
            assert np.array_equal(got_s.cpu().numpy().view(np.uint32), want_s.view(np.uint32)), mw
            assert np.array_equal(acc.assign(min_weight=mw).cpu().numpy(), want_l)
        assert acc.assign().cpu().numpy()[:7].tolist() == [255, 1, 0, 0, 2, 4, 3]
        cases = [dict(), dict(label=0), dict(label=1, min_share=0.3), dict(label=4, min_share=1.0), dict(label=2, min_share=0.0), dict(min_weight=1.0),
                 dict(label=3, min_weight=0.5, min_share=0.2), dict(min_max_weight=0.05), dict(min_pixels=40), dict(label=0, min_share=0.25, min_max_weight=0.02, min_pixels=10),
                 dict(label=0, invert=True), dict(min_pixels=40, invert=True), dict(label=1, min_share=1.0 / 3.0), dict(label=2, min_share=0.2)]
        kept = set()
        for kw in cases:
            want = lr.select(votes, wmax, count, **kw)
            got = acc.select(**kw).cpu().numpy()
            assert np.array_equal(got, want), kw
            kept.add(int(want.sum()))
        assert len(kept) >= 8, "the selections differ"
        # compact_splats: the rows numpy.nonzero names, in source order
        keep = acc.select(label=1, min_share=0.3)
        out, idx = ba.compact_splats(spl, keep, return_indices=True, ctx=ctx)
        rows = np.nonzero(keep.cpu().numpy())[0]
        assert 0 < rows.size < n and np.array_equal(idx.cpu().numpy(), rows)
        assert torch.equal(out.transforms, spl.transforms[rows]) and torch.equal(out.sh_coeffs, spl.sh_coeffs[rows]) and torch.equal(out.raw_opacities, spl.raw_opacities[rows])
        # ... and what crop_splats returns when fed select_region's keep
        region = ba.SceneRegion(center=(0.0, 0.0, 5.0), half_extent=(2.0, 1.5, 2.5))
        keep_r = ba.select_region(spl, region, ctx=ctx)
        a, ia = ba.crop_splats(spl, region, return_indices=True, ctx=ctx)
        b, ib = ba.compact_splats(spl, keep_r, return_indices=True, ctx=ctx)
        assert 0 < ia.numel() < n and torch.equal(ia, ib) and torch.equal(a.transforms, b.transforms) and torch.equal(a.sh_coeffs, b.sh_coeffs)
        assert torch.equal(a.raw_opacities, b.raw_opacities)
    finally:
        ctx.close()


# ---- G. end to end --------------------------------------------------------------------------------------------------------------
def _erode(mask, r):
    h, w = mask.shape
    pad = np.zeros((h + 2 * r, w + 2 * r), bool)
    pad[r:r + h, r:r + w] = mask
    out = np.ones_like(mask)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out &= pad[dy:dy + h, dx:dx + w]
    return out


def test_two_objects_end_to_end(dev):
    import brush_amd as ba
    sc, cams, w, h, member = lr.two_cluster_case()
    n = member.size
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    ctx = ba.Context(dev)
    try:
        parts = [ba.Splats(*(lr.subset(sc, member == k)[f] for f in ("transforms", "sh", "raw_opac")), device=dev) for k in (0, 1)]
        views, maps = [], []
        for cp in cams:
            cam = util.hip_camera(ba, cp)
            alphas = [ba.render_splats_diff(p, cam, (w, h), ctx=ctx).img[..., 3].cpu().numpy() for p in parts]
            maps.append(lr.cluster_labels(*alphas))
            views.append((cam, torch.from_numpy(maps[-1]).to(dev)))
        acc = ba.lift_labels(spl, views, 2, (w, h), ctx=ctx)
        total = acc.votes.cpu().numpy().sum(axis=1)
        strong = total >= lr.VOTE_ONE
        assert int(strong[member == 0].sum()) >= 10 and int(strong[member == 1].sum()) >= 10
        got = acc.assign(min_weight=1.0).cpu().numpy()
        assert np.array_equal(got[strong], member[strong].astype(np.uint8)) and (got[~strong] == 255).all()
        out, idx = ba.compact_splats(spl, acc.select(label=1, min_weight=1.0), return_indices=True, ctx=ctx)
        assert np.array_equal(idx.cpu().numpy(), np.nonzero(strong & (member == 1))[0])
        # the selection rendered from a training view: nothing where the other object's mask was, away from the mask's border
        alpha = ba.render_splats_diff(out, views[0][0], (w, h), ctx=ctx).img[..., 3].cpu().numpy()
        inner = _erode(maps[0] == 0, 2)
        assert int(inner.sum()) > 20 and float(alpha[inner].max()) < 1.0 / 255.0
        assert float(alpha[maps[0] == 1].mean()) > 0.3
    finally:
        ctx.close()


# ---- H. no interference ---------------------------------------------------------------------------------------------------------
def test_interleaved_lift_calls_do_not_change_training(dev):
    """The one-tile deterministic set-up of tests/test_gpu_features.py::test_interleaved_feature_renders_do_not_change_training (16x16,
    6000 splats, seed 77, 9 steps) with, after every step, the votes of the step's own forward (bh_last_render_out), of a frame
    retained before the first step and of a fresh larger frame: parameters, moments and refine statistics equal a run without."""
    import brush_amd as ba
    from brush_amd import _ffi
    n, w, h, L = 6000, 16, 16, 5
    sc = synth.make_scene(n, 0xD0A, sh_degree=1, log_scale_range=(math.log(0.05), math.log(0.4)),
                          tan_half_fov=(math.tan(math.radians(50)), math.tan(math.radians(50))))
    cams = []
    for i in range(3):
        cc = dict(synth.default_camera_params(w, h))
        cc["rot_xyzw"] = util.quat_from_axis_angle((0, 1, 0), math.radians(-35 + 35 * i))
        cams.append(cc)
    gt = torch.from_numpy(synth.synthetic_gt_packed(w, h).view(np.int32)).to(dev)
    ew, eh = 200, 136
    other = util.hip_camera(ba, synth.default_camera_params(ew, eh))
    labels = torch.from_numpy(_with_holes(_xy(ew, eh, L), L)).to(dev)
    runs = {}
    for key in ("plain", "with_lift"):
        ctx = ba.Context(dev)
        try:
            spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
            tr = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=3.0, ctx=ctx, seed=77)
            if key == "with_lift":
                kept = ba.render_splats_diff(spl, other, (ew, eh), ctx=ctx, retain=True)
                acc = ba.LiftAccumulator(n, L, dev, ctx=ctx)
                own = ba.LiftAccumulator(n, 1, dev, ctx=ctx)
            for s in range(9):
                tr.step(ba.SceneBatch(gt, util.hip_camera(ba, cams[s % len(cams)])), spl)
                if key == "with_lift":
                    last = _ffi.BhRenderOut()
                    ctx.check(ctx.lib.bh_last_render_out(ctx._h, C.byref(last)))
                    ctx.check(ctx.lib.bh_lift_accumulate(ctx._h, C.byref(last), None, 1, C.c_void_p(own.votes.data_ptr()), C.c_void_p(own.max_weight.data_ptr()),
                                                         C.c_void_p(own.pixel_count.data_ptr())))
                    acc.add(kept, labels)
                    acc.add(ba.render_splats_diff(spl, other, (ew, eh), ctx=ctx), labels)
                    acc.select(label=1)
            if key == "with_lift":
                assert int(own.votes.sum()) > 0 and int(acc.pixel_count.sum()) > 0
                kept.release()
            ctx.sync()
            out = {"transforms": spl.transforms.clone(), "sh": spl.sh_coeffs.clone(), "opac": spl.raw_opacities.clone()}
            out.update({k: v.clone() for k, v in tr.state.items()})
            runs[key] = out
        finally:
            ctx.close()
    a, b = runs["plain"], runs["with_lift"]
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
