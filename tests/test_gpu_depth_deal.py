"""The dealing path of the depth order (brush_amd/csrc/depth_deal.h, depth_sort.hip dsort_deal_bucket_kernel) through
bh_debug_depth_deal of the test-hooks library: a stand-in for K1 deals the listed keys into the buckets by the table, the one
bucket launch follows, and a frame that overflows a bucket takes the three launches behind it.  Held to tests/dsort_ref.py bit
for bit (tests/depth_deal_cases.py: the cases and which path each takes; test_depth_deal_ref.py checks those without a GPU):
    out_keys[:nv], out_vals[:nv], cum[:nv]         the stable argsort of the listed keys and the scan, ties in splat-id order
    out_*[nv:], cum[nv:]                           still the fill pattern
    the table's 258 words and the two behind them  the frame's quantiles
    the 255 counter words, the overflow word       sizes and tile sums of the buckets; whether the three launches ran
Cases dealt in five arrival orders (thread t deals element t * stride mod n) must leave identical arrays.
Render level: train steps and complete-list renders with option dsort_deal 0 and 1; cut-list train frames on which K1 deals with the
near counts (SH degree 1: the slot is taken ahead of the colour evaluation, and 3: behind the block totals) compared frame by frame;
and the forward's own overflow recovery, reached with the capacity forced small (bh_debug_set_deal_capacity), with the speculative
list builder and with event waits."""
import ctypes as C
import math

import numpy as np
import pytest

import depth_deal_cases as D
import dsort_ref as R

pytestmark = pytest.mark.gpu

PATTERN = 0xA5C3F00D
GUARD = 64
CASES = D.build_cases()


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(dev)


def _filled(n, dev):
    import torch
    return torch.full((n + GUARD,), int(np.uint32(PATTERN).view(np.int32)), dtype=torch.int32, device=dev)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError("%s: first of %d differences at %d: got 0x%X, want 0x%X" % (what, int((got != want).sum()), i, int(got[i]), int(want[i])))


@pytest.fixture(scope="module")
def ctx(dev):
    import brush_amd as ba
    from brush_amd import _ffi
    c = ba.Context(dev, lib=_ffi.load_test_hooks())
    yield c
    c.close()


def deal_run(ctx, dev, keys, counts, table_dev, cap, stride):
    n = keys.size
    k, c, mm = _dev(keys, dev), _dev(counts, dev), _dev(R.minmax_of(keys), dev)
    ok, ov, cum = _filled(n, dev), _filled(n, dev), _filled(n, dev)
    words, fell = (C.c_uint64 * 256)(), C.c_int(-1)
    ctx.check(ctx.lib.bh_debug_depth_deal(ctx._h, _ptr(k), _ptr(mm), _ptr(c), n, _ptr(ok), _ptr(ov), _ptr(cum), _ptr(table_dev), cap, stride, words, C.byref(fell)))
    assert np.array_equal(_u32(k), keys) and np.array_equal(_u32(c), counts)
    return dict(out_keys=_u32(ok), out_vals=_u32(ov), cum=_u32(cum), words=np.frombuffer(words, np.uint64).copy(), fell_back=fell.value, table=_u32(table_dev))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_dealt_depth_order_equals_the_restatement(dev, ctx, case):
    refs = D.reference(case)
    D.check_claims(case, refs)
    table_in = np.array(case.table)
    table_in[258:] = PATTERN
    first = None
    for stride in case.strides:
        table_dev = _dev(table_in, dev)
        got_all = []
        for step, ((keys, counts), (plan, run)) in enumerate(zip(case.frames, refs)):
            got = deal_run(ctx, dev, keys, counts, table_dev, case.cap, stride)
            got_all.append(got)
            f, n, nv = run.frame, keys.size, run.frame.nv
            what = "%s frame %d stride %d" % (case.id, step, stride)
            assert got["fell_back"] == int(plan.overflow), what
            pattern = np.full(n + GUARD - nv, PATTERN, np.uint32)
            for name, want in (("out_keys", f.out_keys), ("out_vals", f.order), ("cum", f.cum)):
                _same(got[name][:nv], want, what + ": " + name)
                _same(got[name][nv:], pattern, what + ": %s behind the listed prefix" % name)
            want_table = np.array(run.table)
            want_table[258:] = PATTERN
            _same(got["table"], want_table, what + ": the table afterwards")
            if plan.valid:
                _same(got["words"][:255], plan.words(), what + ": bucket words")
            assert (got["words"][255] != 0) == plan.overflow, what
        if first is None:
            first = got_all
        else:   # another arrival order: the same arrays
            for a, b in zip(first, got_all):
                for name in ("out_keys", "out_vals", "cum", "table"):
                    _same(b[name], a[name], "%s stride %d vs stride 1: %s" % (case.id, stride, name))


def test_hook_counts_dealt_frames_and_fallbacks(dev, ctx):
    out = (C.c_uint32 * 2)()
    ctx.check(ctx.lib.bh_debug_dsort_deal_counts(ctx._h, out))
    before = (out[0], out[1])
    case = [c for c in CASES if c.id == "capacity-3001-of-3000"][0]
    keys, counts = case.frames[0]
    got = deal_run(ctx, dev, keys, counts, _dev(case.table, dev), case.cap, 1)
    ctx.check(ctx.lib.bh_debug_dsort_deal_counts(ctx._h, out))
    assert got["fell_back"] == 1 and (out[0], out[1]) == (before[0] + 1, before[1] + 1)


def test_train_steps_and_renders_are_the_same_with_and_without_dealing(dev):
    """256 x 256, 20 000 splats, cut threshold 0: two train steps and then three complete-list renders of the view (the second and third
    of which deal: a table of the view's complete lists exists and holds quantiles), with dsort_deal 0, 0 again and 1.  Image, tile
    offsets, list contents and the counts are identical between the paths at every frame; the parameters after the train steps are
    equal between the paths within the bound two runs of the three-launch path are held to (the backward's float atomics)."""
    import torch

    import brush_amd as ba
    from brush_amd import _ffi, synth
    import util
    n, w, h = 20000, 256, 256
    sc = synth.make_scene(n, 0x5D, sh_degree=1, log_scale_range=(math.log(0.01), math.log(0.06)), tan_half_fov=(math.tan(math.radians(30)), math.tan(math.radians(30))))
    cam = util.hip_camera(ba, synth.default_camera_params(w, h))
    gt_dev = torch.from_numpy(synth.synthetic_gt_packed(w, h).view(np.int32)).to(dev)
    lib = _ffi.load_test_hooks()

    def run(deal):
        ctx = ba.Context(dev, lib=lib, options={"cut_min_pairs": 0, "dsort_deal": deal})
        spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
        trainer = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=3.0, ctx=ctx)
        rng = np.random.default_rng(5)
        frames = []
        for step in range(2):
            noise = torch.from_numpy(rng.normal(size=(n, 3)).astype(np.float32)).to(dev)
            trainer.step(ba.SceneBatch(gt_dev, cam, view_id=1), spl, background=(0.1, 0.2, 0.3), noise_samples=noise)
        params = (spl.transforms.cpu().numpy().copy(), spl.sh_coeffs.cpu().numpy().copy(), spl.raw_opacities.cpu().numpy().copy())
        # the renders run on identical parameters in every run: the FIRST run's
        return ctx, trainer, params, frames

    def renders(ctx, params):
        spl = ba.Splats(params[0].copy(), params[1].copy(), params[2].copy(), device=dev)
        out = []
        ctx.lib.bh_set_view_id(ctx._h, 7)
        for k in range(3):
            img, aux = ba.render_splats(spl, cam, (w, h), (0.1, 0.2, 0.3), ba.RasterPass.Backward, ctx=ctx)
            ni, nv = aux.num_intersections, aux.num_visible
            out.append(dict(img=img.cpu().numpy(), nv=nv, ni=ni, offs=util.u32(aux.tile_offsets).copy(), gids=util.u32(aux.compact_gid_from_isect)[:ni].copy(),
                            tiles=util.u32(aux.tile_id_from_isect)[:ni].copy(), gfc=util.u32(aux.global_from_compact_gid)[:nv].copy()))
        cnt = (C.c_uint32 * 2)()
        ctx.check(ctx.lib.bh_debug_dsort_deal_counts(ctx._h, cnt))
        return out, (cnt[0], cnt[1])

    results = []
    for deal in (0, 0, 1):
        ctx, trainer, params, _ = run(deal)
        stats = trainer.stats(ctx)
        results.append(dict(params=params, loss=stats.loss, nv=stats.num_visible, ni=stats.num_intersections, renders=renders(ctx, results[0]["params"] if results else params)))
        ctx.close()
    a, b, d = results
    assert a["nv"] == b["nv"] == d["nv"] and a["ni"] == b["ni"] == d["ni"]
    # (float atomics of the backward: two runs of ONE path already differ — the project's bound for that, util.assert_adam_close,
    #  holds between the two three-launch runs and between them and the dealing run alike)
    cfg = ba.TrainConfig()
    for other in (b, d):
        print("max |difference| to the first three-launch run:", [float(np.abs(a["params"][i] - other["params"][i]).max()) for i in range(3)])
        util.assert_adam_close(a["params"][0][:, 3:7], other["params"][0][:, 3:7], cfg.lr_rotation, 2, "rotation")
        util.assert_adam_close(a["params"][0][:, 7:10], other["params"][0][:, 7:10], cfg.lr_scale, 2, "scale")
        util.assert_adam_close(a["params"][2], other["params"][2], cfg.lr_opac, 2, "opacity")
        assert abs(a["loss"] - other["loss"]) <= 1e-4 * max(1.0, abs(a["loss"]))
    (ra, ca), (rb, cb), (rd, cd) = a["renders"], b["renders"], d["renders"]
    assert ca == (0, 0) and cb == (0, 0)
    assert ra[0]["nv"] >= R.SPL_MIN_KEYS, ra[0]["nv"]   # the first render leaves quantiles: the next two deal
    assert cd[0] >= 2 and cd[1] == 0, cd
    for fa, fd in zip(ra, rd):
        assert fa["nv"] == fd["nv"] and fa["ni"] == fd["ni"]
        for k in ("img", "offs", "gids", "tiles", "gfc"):
            assert np.array_equal(fa[k], fd[k]), k


# ---- cut-list train frames: K1 deals with the near counts; the forward's overflow recovery --------------------------------------------
_W = _H = 256
_N = 40000
_STEPS = 4
_frames_cache = {}


def _cut_scene(deg):
    from brush_amd import synth
    # (splats large enough that tiles saturate: the view's second frame is cut to ~70 % of its pairs and lists ~25 000 of 37 000 visible
    #  splats — a table of the cut lists with quantiles — and the frames behind it deal)
    return synth.make_scene(_N, 0x5D, sh_degree=deg, log_scale_range=(math.log(0.02), math.log(0.15)), tan_half_fov=(math.tan(math.radians(30)),) * 2)


def _train_frames(dev, deg, options, cap=0):
    """_STEPS train steps of one view, every step on the SAME parameters (uploaded again: the frames of two runs are then comparable bit
    for bit, the backward's float atomics never reach a forward) -> per step what the step's forward left, and the deal counters."""
    import torch

    import brush_amd as ba
    from brush_amd import _ffi, host, synth
    import util
    lib = _ffi.load_test_hooks()
    sc = _cut_scene(deg)
    cam = util.hip_camera(ba, synth.default_camera_params(_W, _H))
    gt_dev = torch.from_numpy(synth.synthetic_gt_packed(_W, _H).view(np.int32)).to(dev)
    ctx = ba.Context(dev, lib=lib, options=dict({"cut_min_pairs": 0}, **options))
    if cap:
        ctx.check(lib.bh_debug_set_deal_capacity(ctx._h, cap))
    trainer = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=3.0, ctx=ctx)
    noise = torch.zeros((_N, 3), device=dev)
    frames = []
    for step in range(_STEPS):
        spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
        trainer.step(ba.SceneBatch(gt_dev, cam, view_id=1), spl, background=(0.1, 0.2, 0.3), noise_samples=noise)
        ctx.sync()
        out = _ffi.BhRenderOut()
        ctx.check(lib.bh_last_render_out(ctx._h, C.byref(out)))
        aux = host._aux_from(out, _N, _W, _H, dev, True, ctx)
        cnt = (C.c_uint32 * 2)()
        ctx.check(lib.bh_debug_dsort_deal_counts(ctx._h, cnt))
        frames.append(dict(img=host._view(out.out_img, (_H, _W, 4), torch.float32, dev).cpu().numpy().copy(), nv=aux.num_visible, ni=aux.num_intersections,
                           nl=aux.num_listed_splats, budget=aux.list_budget, offs=util.u32(aux.tile_offsets), gids=util.u32(aux.compact_gid_from_isect),
                           tiles=util.u32(aux.tile_id_from_isect), gfc=util.u32(aux.global_from_compact_gid), cum=util.u32(aux.cum_tiles_hit),
                           dealt=cnt[0], fell_back=cnt[1], loss=trainer.stats(ctx).loss))
    ctx.close()
    return frames


def _reference_frames(dev, deg):
    if deg not in _frames_cache:
        _frames_cache[deg] = _train_frames(dev, deg, {"dsort_deal": 0})
        assert [f["dealt"] for f in _frames_cache[deg]] == [0] * _STEPS
    return _frames_cache[deg]


def _assert_same_frames(got, want, what):
    for step, (g, w) in enumerate(zip(got, want)):
        assert (g["nv"], g["ni"], g["nl"], g["budget"]) == (w["nv"], w["ni"], w["nl"], w["budget"]), (what, step)
        assert g["loss"] == w["loss"], (what, step)
        for k in ("img", "offs", "gids", "tiles", "gfc", "cum"):
            assert np.array_equal(g[k], w[k]), (what, step, k)


@pytest.mark.parametrize("deg", [1, 3])
def test_k1_deals_on_cut_list_train_frames(dev, deg):
    """Step 1 seeds the view (complete lists), step 2 is the first cut frame and leaves the cut lists' table, steps 3 and 4 are cut frames
    on which K1 deals — with the near counts in the counter words' high halves.  Image, tile offsets, lists, order, scan, counts and loss of
    every step equal the three-launch run's."""
    want = _reference_frames(dev, deg)
    got = _train_frames(dev, deg, {"dsort_deal": 1})
    dealt = [f["dealt"] for f in got]
    assert dealt[:2] == [0, 0] and dealt[2:] == [1, 2] and got[-1]["fell_back"] == 0, (dealt, got[-1]["fell_back"])
    for f in got[1:]:   # cut frames: fewer listed splats than visible ones, fewer pairs than intersections, and a table with quantiles
        assert R.SPL_MIN_KEYS <= f["nl"] < f["nv"] and f["budget"] < f["ni"], (f["nl"], f["nv"], f["budget"], f["ni"])
    _assert_same_frames(got, want, "dealt, SH degree %d" % deg)


@pytest.mark.parametrize("options", [{}, {"event_waits": 1}], ids=["speculative-k5", "event-waits"])
def test_forward_recovers_from_a_bucket_overflow(dev, options):
    """64 slots per bucket for ~25 000 listed splats: every dealt frame overflows.  The bucket launch does nothing and tells the list
    builder queued behind it that nothing is listed, the host reads the overflow word with the counts, queues the three launches and the
    list builder again — and the frames equal the three-launch run's in everything."""
    want = _reference_frames(dev, 1)
    got = _train_frames(dev, 1, dict({"dsort_deal": 1}, **options), cap=64)
    assert [(f["dealt"], f["fell_back"]) for f in got] == [(0, 0), (0, 0), (1, 1), (2, 2)], [(f["dealt"], f["fell_back"]) for f in got]
    _assert_same_frames(got, want, "overflow recovery %r" % (options,))
