"""bh_train_set_features / SplatTrainer(feature_field=) (include/brush_hip_feature_train.h), test for test after
tests/test_gpu_distortion_train.py and on its scenes (restated here): nothing attached (no field, no target, weight 0 / NaN) changes
nothing; a step with the term is the hand-composed render -> feature map -> feature loss -> image loss -> ONE backward with a feature
term, and the field's update is the host adam_step on the captured v_features bit for bit; the row-marked single-GPU step equals the
zero-filled hook step bit for bit, rows that only the feature term writes included; a cut frame agrees with a complete one; the term
works beside the depth, normal and distortion terms (by linearity: the sum of two hand-composed backwards); what cannot work is
refused before anything runs; feature_loss_from_iter starts the term at that step; a field trains jointly with the splats through a
refine that prunes and splits.  No seed: the noise terms are zero.

Channel counts {3, 5, 19}: chunk widths 4, 8 and 16 with a remainder, at 19 a second pass with a tail.  The bit-for-bit comparison
of whole steps takes 13 in place of 19 (one chunk of 16 with a remainder): with two chunks two blocks race on v_combined's float
atomics and two runs of the SAME configuration differ in the last bit; 19 channels are compared row-marked against zero-filled
through the Adam moments of frozen steps, to the atomics-order bound (test_row_marked_step_with_two_chunks_agrees_...).

Measured on an MI355X: step vs hand-composed gradient blocks within 1.3e-7 and v_features within 7.6e-8 of each
block's largest entry (bound 1e-4); cut vs exact frame: loss 0 relative (bound 1e-6), gradient blocks within 1.5e-7 and v_features
within 1.1e-7 (bound 3e-5: v_features needs no more); four terms against the sum of two backwards within 4.2e-7 (bound 2e-4); joint
training (34 pruned, 54 added): cross-entropy 1.3863 -> 0.2236 (ratio 0.161), pixel accuracy 0.250 -> 0.963; 19 channels row-marked
against zero-filled through the frozen steps' moments: at most 3.5e-10 of a block's largest entry (bound 3e-5), most tensors equal."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import util

pytestmark = pytest.mark.gpu
BG = (0.1, 0.2, 0.3)
W, H = 64, 48
GRAD_TOL = 1e-4    # of each block's largest entry (README, "Correctness")
CUT_TOL = 3e-5     # cut frames against exact frames: the float atomics' order only (tests/test_gpu_depth_train.py)
FROZEN = dict(lr_mean=1e-30, lr_mean_end=1e-30, lr_coeffs_dc=0.0, lr_opac=0.0, lr_scale=0.0, lr_rotation=0.0)   # steps that move nothing
FIELD_KEYS = ("f_features", "f_m1", "f_m2")


def _scene(n=400, seed=0x3E):
    return synth.make_scene(n, seed, sh_degree=1, log_scale_range=(math.log(0.05), math.log(0.4)),
                            tan_half_fov=(math.tan(math.radians(50)), math.tan(math.radians(50))))


def _one_tile():
    return synth.make_scene(6000, 0xD0A, sh_degree=1, log_scale_range=(math.log(0.05), math.log(0.4)),
                            tan_half_fov=(math.tan(math.radians(50)), math.tan(math.radians(50))))


def _gt(dev, w=W, h=H):
    return torch.from_numpy(np.ascontiguousarray(synth.synthetic_gt_packed(w, h)).view(np.int32)).to(dev)


def _splats(ba, sc, dev):
    return ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _depth_gt(ba, ctx, sc, cam, w, h, dev, factor=1.07):
    """Expected depth of the scene with its means pushed along their viewing rays (the camera sits at the origin)."""
    moved = dict(sc, transforms=sc["transforms"].copy())
    moved["transforms"][:, :3] *= np.float32(factor)
    node = ba.render_splats_diff(_splats(ba, moved, dev), cam, (w, h), BG, ctx=ctx)
    d = node.depth("expected").clone()
    ctx.sync()
    return d


def _capture(tr, store):
    """An identity bh_grad_hook that copies what it is given: the exchange buffer, then (with a feature term) v_features."""
    from brush_amd import _ffi
    from brush_amd.host import _view

    def hook(_user, ptr, count):
        try:
            store.append(_view(ptr, (int(count),), torch.float32, torch.device("cuda", torch.cuda.current_device())).clone())
            return 0
        except Exception:
            return 1
    tr._hook = _ffi.GRAD_HOOK(hook)
    tr._world = 1
    tr.pg = object()   # (only its presence matters: the step takes the hook above, partition "cameras")
    tr.sparse_exchange = False


def _blocks(buf, n, c):
    pad4 = lambda x: (x + 3) & ~3   # noqa: E731
    o_tr = pad4(n)
    o_sh = o_tr + pad4(n * 10)
    o_op = o_sh + pad4(n * 3 * c)
    b = buf.cpu().numpy()
    return dict(v_transforms=b[o_tr:o_tr + n * 10].reshape(n, 10), v_sh_coeffs=b[o_sh:o_sh + n * 3 * c], v_raw_opacities=b[o_op:o_op + n])


def _close(got, want, tol, what):
    worst = {}
    for k, y in want.items():
        x, y = np.asarray(got[k], np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
        scale = max(float(np.abs(y).max()), 1e-20)
        worst[k] = float(np.abs(x - y).max()) / scale
        assert np.isfinite(x).all() and worst[k] <= tol, (what, k, worst[k])
    print(what, " ".join("%s %.2e" % kv for kv in worst.items()), "(bound %.0e)" % tol)


def _field(ba, ctx, n, ch, dev, lr=1e-2, seed=0xF1E1D):
    """A field with N(0, 0.5) features (a zero field would make the term's geometry gradient vanish) and zero moments."""
    f = ba.FeatureField(n, ch, lr=lr, device=dev, ctx=ctx)
    rows = np.random.default_rng(seed + ch).normal(0.0, 0.5, (n, ch)).astype(np.float32)
    f.features.copy_(torch.from_numpy(rows))
    return f, rows


def _target(kind, w, h, ch, dev, seed=0x7A6):
    """l1: f32 [H,W,C] from N(0, 1); cross_entropy: uint8 labels [H,W] in 0 .. C-1 with 255 (ignore) at every 11th pixel."""
    rng = np.random.default_rng(seed + ch)
    if kind == "l1":
        return torch.from_numpy(rng.normal(0.0, 1.0, (h, w, ch)).astype(np.float32)).to(dev)
    lab = rng.integers(0, ch, (h, w)).astype(np.uint8)
    lab.reshape(-1)[::11] = 255
    return torch.from_numpy(lab).to(dev)


def _state(spl, tr, field=None):
    out = {"transforms": spl.transforms.clone(), "sh": spl.sh_coeffs.clone(), "opac": spl.raw_opacities.clone()}
    out.update({k: v.clone() for k, v in tr.state.items()})
    if field is not None:
        out.update(f_features=field.features.clone(), f_m1=field.m1.clone(), f_m2=field.m2.clone())
    return out


def _run(dev, sc, w, h, steps, mode, ch=5, kind="l1", hook=False, weight=1.0, cfg_kw=None, store=None, per_step=None, gt=None, bg=BG, info=None, field_lr=1e-2):
    """mode: "plain" (no field), "no-target" (a field, batches without a target), "zero" / "nan" (field and target attached at that
    weight), "features" (the term)."""
    import brush_amd as ba
    from brush_amd import _ffi
    ctx = ba.Context(dev)
    try:
        cam = util.hip_camera(ba, synth.default_camera_params(w, h))
        gt = _gt(dev, w, h) if gt is None else gt
        spl = _splats(ba, sc, dev)
        n = spl.num_splats()
        field = None if mode == "plain" else _field(ba, ctx, n, ch, dev, lr=field_lr)[0]
        target = None if mode in ("plain", "no-target") else _target(kind, w, h, ch, dev)
        kw = dict(cfg_kw or {})
        kw.setdefault("feature_loss_weight", weight if mode in ("features", "no-target") else 0.0)
        cfg = ba.TrainConfig(background_color=bg, feature_loss_kind=kind, **kw)
        tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx, feature_field=field)
        if mode in ("zero", "nan"):   # (the trainer detaches at weight 0: attach such a term behind it)
            off = _ffi.BhFeatureTarget()
            off.target, off.h, off.w, off.channels, off.kind = target.data_ptr(), h, w, ch, ba.host.FEATURE_LOSS_KINDS[kind]
            off.weight = 0.0 if mode == "zero" else float("nan")
            tr.batch_patch = lambda b: ctx.check(ctx.lib.bh_train_set_features(ctx._h, C.byref(field.as_struct()), C.byref(off)))
        if hook:
            _capture(tr, store if store is not None else [])
        losses = []
        for _ in range(steps):
            _, st = tr.step(ba.SceneBatch(gt, cam, view_id=2, features=target if mode == "features" else None), spl)
            ctx.sync()
            losses.append(np.float32(st.loss))
            if per_step is not None:
                per_step.append(_state(spl, tr, field))
        if info is not None:
            info["t"] = None if field is None else field.t
        return losses, _state(spl, tr, field)
    finally:
        ctx.close()


def test_nothing_attached_changes_nothing(dev):
    """No field; a field with no target in the batch; weight 0; weight NaN: on ONE 16x16 tile whole steps repeat bit for bit, so three
    steps leave the loss bits and every splat and optimizer tensor of a plain run, and the field as it was."""
    one = _one_tile()
    n = one["transforms"].shape[0]
    lp, a = _run(dev, one, 16, 16, 3, "plain")
    runs = {}
    for mode in ("no-target", "zero", "nan"):
        info = {}
        runs[mode] = _run(dev, one, 16, 16, 3, mode, info=info) + (info,)
    ld, d = _run(dev, one, 16, 16, 3, "features")
    first = torch.from_numpy(np.random.default_rng(0xF1E1D + 5).normal(0.0, 0.5, (n, 5)).astype(np.float32))
    for mode, (losses, b, info) in runs.items():
        assert [v.tobytes() for v in lp] == [v.tobytes() for v in losses], mode
        for k in a:
            assert torch.equal(_bits(a[k]), _bits(b[k])), (mode, k)
        assert info["t"] == 0, mode
        assert torch.equal(_bits(b["f_features"].cpu()), _bits(first)), mode
        assert int(torch.count_nonzero(_bits(b["f_m1"]))) == 0 and int(torch.count_nonzero(_bits(b["f_m2"]))) == 0, mode
    # ... and a weight > 0 does change something (the comparison above is not vacuous)
    assert math.isfinite(lp[0]) and ld[0] > lp[0] and not torch.equal(_bits(a["transforms"]), _bits(d["transforms"]))
    assert not torch.equal(_bits(d["f_features"].cpu()), _bits(first))


@pytest.mark.parametrize("kind", ["l1", "cross_entropy"])
@pytest.mark.parametrize("ch", [3, 5, 19])
def test_step_equals_the_hand_composed_path(dev, ch, kind):
    import brush_amd as ba
    sc = _scene()
    n, c = sc["transforms"].shape[0], sc["sh"].shape[1]
    cam, gt = util.hip_camera(ba, synth.default_camera_params(W, H)), _gt(dev)
    wf = 1.0
    cfg = ba.TrainConfig(exact_lists=True, background_color=BG, feature_loss_weight=wf, feature_loss_kind=kind)
    ctx = ba.Context(dev)
    try:
        field, rows = _field(ba, ctx, n, ch, dev)
        target = _target(kind, W, H, ch, dev)
        feats = field.features.clone()
        # by hand on the untouched splats
        spl0 = _splats(ba, sc, dev)
        node = ba.render_splats_diff(spl0, cam, (W, H), BG, ctx=ctx)
        fmap = ba.render_features(node, feats)
        x = node.img.clone()
        fl, v_map = ba.feature_loss_value_and_grad(fmap, target, kind, wf, ctx=ctx)
        l_img, v = ba.image_loss_value_and_grad(x, gt, l1_weight=1.0 - cfg.ssim_weight, ssim_weight=-cfg.ssim_weight, ctx=ctx)
        want = node.backward(v, v_features=v_map, features=feats)
        ctx.sync()
        fl = fl.cpu().numpy()
        valid = int((target.cpu().numpy() < ch).sum()) if kind == "cross_entropy" else W * H
        assert fl[0] > 0 and fl[1] == valid and (kind == "l1" or valid < W * H), (fl, valid)
        want_loss = np.float32(np.float32(l_img.cpu().numpy()[0]) + np.float32(fl[0]))   # (image) + feature, in f32, in this order
        want = {k: want[k].cpu().numpy() for k in ("v_transforms", "v_sh_coeffs", "v_raw_opacities", "v_features")}
        only_colour = node.backward(v)["v_transforms"].cpu().numpy()
        assert np.abs(want["v_transforms"][:, :3] - only_colour[:, :3]).max() > 1e-3 * np.abs(only_colour[:, :3]).max()   # the term reaches the means
        # the step
        spl = _splats(ba, sc, dev)
        tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx, feature_field=field)
        store = []
        _capture(tr, store)
        _, st = tr.step(ba.SceneBatch(gt, cam, view_id=2, features=target), spl)
        ctx.sync()
        assert np.float32(st.loss).tobytes() == want_loss.tobytes(), (st.loss, want_loss, fl)
        assert len(store) == 2 and store[1].numel() == n * ch, [s.numel() for s in store]   # the exchange buffer, then v_features
        geometry = {k: want[k] for k in ("v_transforms", "v_sh_coeffs", "v_raw_opacities")}
        _close(_blocks(store[0], n, c), geometry, GRAD_TOL, "step vs hand-composed (C = %d, %s):" % (ch, kind))
        _close({"v_features": store[1].cpu().numpy()}, {"v_features": want["v_features"]}, GRAD_TOL, "... its v_features:")
        # the field's update: the host adam_step on the captured v_features, bit for bit (grad_scale is 1)
        p, m1, m2 = feats.clone(), torch.zeros_like(feats), torch.zeros_like(feats)
        ba.adam_step(p, store[1].view(n, ch).contiguous(), m1, m2, field.lr, 1, beta1=field.beta1, beta2=field.beta2, eps=field.eps, ctx=ctx)
        ctx.sync()
        assert field.t == 1
        assert torch.equal(_bits(field.features), _bits(p)) and torch.equal(_bits(field.m1), _bits(m1)) and torch.equal(_bits(field.m2), _bits(m2))
        assert not torch.equal(_bits(field.features), _bits(feats))
    finally:
        ctx.close()


def _assert_same_state(lm, a, lh, b):
    assert [v.tobytes() for v in lm] == [v.tobytes() for v in lh]
    for k in a:
        x, y = a[k], b[k]
        if k == "m2_sh":
            # the row-marked step's update keeps its "dormant" marks in the SIGN of a zero m2_sh (optim.hip; -0.0 where every moment
            # of the splat is zero), the zero-filled step keeps none: the sign of a zero is not part of the state
            assert bool((x[x == 0] == 0).all()) and bool((torch.signbit(y) == 0).all())
            x = torch.where(x == 0, torch.zeros_like(x), x)
        assert torch.equal(_bits(x), _bits(y)), k   # (the field's three tensors are among the keys)


@pytest.mark.parametrize("ch,kind", [(3, "cross_entropy"), (5, "l1"), (13, "cross_entropy")])
def test_row_marked_step_equals_the_zero_filled_step(dev, ch, kind):
    """Without a hook the step zero-fills nothing and K18 marks the rows it writes; with one the whole span is cleared.  The feature
    term's geometry gradient arrives through v_combined, so K18 writes and marks its rows like the colour term's: three steps either
    way leave the same bits, the field's included.

    Channel counts 3, 5 and 13: chunk widths 4, 8 and 16, each with a remainder, ONE chunk each.  The one-tile scene repeats bit for
    bit because one block owns every accumulator row; from 17 channels on the feature backward runs one block per chunk of 16 on
    the tile, and their float atomics into v_combined race: two runs of the SAME configuration then differ in the last bit (DESIGN.md
    §6s), so 19 channels cannot be compared bit for bit here: the next test compares them to the atomics-order bound."""
    one = _one_tile()
    n, c = one["transforms"].shape[0], one["sh"].shape[1]
    with_term, without = [], []
    lm, a = _run(dev, one, 16, 16, 3, "features", ch=ch, kind=kind)
    lh, b = _run(dev, one, 16, 16, 3, "features", ch=ch, kind=kind, hook=True, store=with_term)
    _run(dev, one, 16, 16, 1, "plain", hook=True, store=without)
    gn, gp = _blocks(with_term[0], n, c)["v_transforms"], _blocks(without[0], n, c)["v_transforms"]
    moved = np.abs(gn[:, :3] - gp[:, :3]).max(axis=1) > 0
    print("splats whose mean gradient the feature term changed: %d of %d" % (int(moved.sum()), n))
    assert moved.any() and all(k in a for k in FIELD_KEYS)
    _assert_same_state(lm, a, lh, b)


@pytest.mark.parametrize("kind", ["l1", "cross_entropy"])
def test_row_marked_step_with_two_chunks_agrees_with_the_zero_filled_step(dev, kind):
    """19 channels: two chunk blocks per tile, whose float atomics into v_combined race, so whole steps do not repeat bit for bit
    and the comparison above cannot be made.  What can: with every learning rate frozen (the field's too) nothing moves, and
    after three steps the Adam moments ARE the gradients — m1 = (1 - b1) (1 + b1 + b1^2) g is linear in them, m2 quadratic — so
    the row-marked step (no hook: the default single-GPU path, K18 marking the rows it writes) is compared with the zero-filled
    hook step through every optimizer tensor and the field's moments.

    Bounds.  The two runs differ by the order of float atomics only, for which this suite's bound is CUT_TOL of each block's
    largest entry.  First moments and the refine statistics: CUT_TOL.  Per-element second moments: g'^2 - g^2 = (g' - g)(g' + g)
    <= 2 CUT_TOL (1 + CUT_TOL) of the largest g^2.  m2_sh holds a row's MEAN of squares over row_len = 3 K entries, its largest
    entry may be as small as max g^2 / row_len: 2 CUT_TOL (1 + CUT_TOL) row_len.  The parameters and the features: unchanged,
    bit for bit, in both runs.  The loss of each step: the forward and the fused losses have no atomics and the state does not
    move, so the bits agree."""
    one = _one_tile()
    n, c = one["transforms"].shape[0], one["sh"].shape[1]
    ch = 19
    kw = dict(ch=ch, kind=kind, cfg_kw=FROZEN, field_lr=0.0)
    store = []
    lm, a = _run(dev, one, 16, 16, 3, "features", **kw)
    lh, b = _run(dev, one, 16, 16, 3, "features", hook=True, store=store, **kw)
    _, plain = _run(dev, one, 16, 16, 3, "plain", cfg_kw=FROZEN)
    assert len(store) == 6 and store[1].numel() == n * ch
    assert [v.tobytes() for v in lm] == [v.tobytes() for v in lh] and all(math.isfinite(v) for v in lm)
    first = torch.from_numpy(np.random.default_rng(0xF1E1D + ch).normal(0.0, 0.5, (n, ch)).astype(np.float32))
    for run in (a, b):   # nothing moved
        assert np.array_equal(run["transforms"].cpu().numpy(), one["transforms"]) and np.array_equal(run["sh"].cpu().numpy(), one["sh"])
        assert np.array_equal(run["opac"].cpu().numpy(), one["raw_opac"]) and torch.equal(_bits(run["f_features"].cpu()), _bits(first))
    quad = 2.0 * CUT_TOL * (1.0 + CUT_TOL)
    bounds = {"m2_t": quad, "m2_o": quad, "f_m2": quad, "m2_sh": quad * 3 * c}
    rest = [k for k in a if k not in ("transforms", "sh", "opac", "f_features")]
    assert set(bounds) < set(rest) and {"m1_t", "m1_sh", "m1_o", "f_m1", "refine_weight_norm"} < set(rest)
    for k in rest:
        _close({k: a[k].cpu().numpy()}, {k: b[k].cpu().numpy()}, bounds.get(k, CUT_TOL), "19 channels, row-marked vs zero-filled (%s):" % kind)
    assert float(a["f_m1"].abs().max()) > 0 and float(a["m1_t"].abs().max()) > 0
    # the term reaches the means: their first moments differ from a plain run's by more than 1e-3 of its largest entry
    gm, gp = a["m1_t"][:, :3].cpu().numpy(), plain["m1_t"][:, :3].cpu().numpy()
    assert np.abs(gm - gp).max() > 1e-3 * np.abs(gp).max()


def test_rows_that_only_the_feature_term_writes_are_marked(dev):
    """Black SH over a black background against a black target: the colour cotangent is exactly zero, so every row K18 writes comes
    from the feature term alone."""
    sc = {k: v.copy() for k, v in _one_tile().items()}
    sc["sh"][:] = 0.0
    sc["sh"][:, 0, :] = -4.0
    n, c = sc["transforms"].shape[0], sc["sh"].shape[1]
    gt = torch.zeros((16, 16), dtype=torch.int32, device=dev)
    kw = dict(gt=gt, bg=(0.0, 0.0, 0.0), ch=5, kind="l1")
    store, plain = [], []
    lm, a = _run(dev, sc, 16, 16, 3, "features", **kw)
    lh, b = _run(dev, sc, 16, 16, 3, "features", hook=True, store=store, **kw)
    _run(dev, sc, 16, 16, 1, "plain", hook=True, store=plain, gt=gt, bg=(0.0, 0.0, 0.0))
    g0 = _blocks(plain[0], n, c)
    assert all(not np.any(v) for v in g0.values()), "the colour term's cotangent is not exactly zero on the black scene"
    written = np.abs(_blocks(store[0], n, c)["v_transforms"]).max(axis=1) > 0
    print("rows written by the feature term alone: %d of %d" % (int(written.sum()), n))
    assert written.any()
    _assert_same_state(lm, a, lh, b)


def test_cut_frame_agrees_with_the_exact_frame(dev):
    """The same view twice with per-tile cuts: the second step's loss, gradients and v_features agree with the complete-list step of
    the same state (nothing moves: every lr 0, the field's too)."""
    import brush_amd as ba
    w, h, ch = 128, 96, 5
    cp = synth.default_camera_params(w, h)
    sc = synth.make_scene(20000, 0x57, log_scale_range=(math.log(0.03), math.log(0.3)), tan_half_fov=(math.tan(cp["fov_x"] / 2.0), math.tan(cp["fov_y"] / 2.0)))
    n, c = sc["transforms"].shape[0], sc["sh"].shape[1]
    res = {}
    for exact in (True, False):
        ctx = ba.Context(dev)
        try:
            cam, gt = util.hip_camera(ba, cp), _gt(dev, w, h)
            spl = _splats(ba, sc, dev)
            field, rows = _field(ba, ctx, n, ch, dev, lr=0.0)
            target = _target("l1", w, h, ch, dev)
            tr = ba.SplatTrainer(ba.TrainConfig(exact_lists=exact, background_color=BG, feature_loss_weight=1.0, **FROZEN), median_scene_scale=3.0, ctx=ctx,
                                 feature_field=field)
            store = []
            _capture(tr, store)
            for _ in range(2):
                _, st = tr.step(ba.SceneBatch(gt, cam, view_id=3, features=target), spl)
                ctx.sync()
            near, far = ba.last_list_counts(ctx)
            assert len(store) == 4
            res[exact] = (np.float32(st.loss), dict(_blocks(store[2], n, c), v_features=store[3].cpu().numpy()), near + far, st.num_intersections)
            assert np.array_equal(spl.transforms.cpu().numpy(), sc["transforms"]) and np.array_equal(field.features.cpu().numpy(), rows) and field.t == 2
        finally:
            ctx.close()
    print("pairs listed by the second frame: complete %d, cut %d of %d" % (res[True][2], res[False][2], res[False][3]))
    assert res[False][2] < res[False][3]   # the second frame did use cut lists
    rel = abs(float(res[True][0]) - float(res[False][0])) / max(1.0, abs(float(res[True][0])))
    print("cut frame vs exact frame: loss %.9g vs %.9g (relative %.2e, bound 1e-6)" % (res[False][0], res[True][0], rel))
    assert rel <= 1e-6
    _close(res[False][1], res[True][1], CUT_TOL, "cut frame vs exact frame:")


def test_step_beside_depth_normal_and_distortion_is_the_sum_of_two_backwards(dev):
    """RenderNode.backward refuses a feature cotangent beside the others, the step's ONE backward carries all of them: by linearity its
    gradient blocks are the sum of the three-term backward and the feature-only backward of one node (2 GRAD_TOL: the expectation is
    itself a sum of two results)."""
    import brush_amd as ba
    sc = _scene()
    n, c = sc["transforms"].shape[0], sc["sh"].shape[1]
    ch, kind = 19, "cross_entropy"
    cam, gt = util.hip_camera(ba, synth.default_camera_params(W, H)), _gt(dev)
    wn, wd, wx, wf = 0.4, 0.6, 0.5, 1.0
    cfg = ba.TrainConfig(exact_lists=True, background_color=BG, normal_loss_weight=wn, depth_loss_weight=wd, distortion_loss_weight=wx,
                         feature_loss_weight=wf, feature_loss_kind=kind)
    ctx = ba.Context(dev)
    try:
        dgt = _depth_gt(ba, ctx, sc, cam, W, H, dev)
        field, _ = _field(ba, ctx, n, ch, dev)
        target = _target(kind, W, H, ch, dev)
        feats = field.features.clone()
        spl0 = _splats(ba, sc, dev)
        node = ba.render_splats_diff(spl0, cam, (W, H), BG, ctx=ctx)
        e = node.depth("expected")
        nmap = node.normal("accumulated")
        mo = ba.render_distortion(node, "z", moments=True)
        fmap = ba.render_features(node, feats)
        x = node.img.clone()
        dl, v_depth = ba.depth_loss_value_and_grad(e, dgt, "l1", wd, ctx=ctx)
        nl, v_normal, v_depth = ba.normal_consistency_value_and_grad(nmap, e, x, cam, wn, v_depth=v_depth, ctx=ctx)
        xl = ba.distortion_loss(mo, wx, ctx=ctx)
        fl, v_map = ba.feature_loss_value_and_grad(fmap, target, kind, wf, ctx=ctx)
        l_img, v = ba.image_loss_value_and_grad(x, gt, l1_weight=1.0 - cfg.ssim_weight, ssim_weight=-cfg.ssim_weight, ctx=ctx)
        gain = np.float32(np.float64(np.float32(wx)) / np.float64(W * H))
        v_dist = torch.full((H, W), float(gain), dtype=torch.float32, device=dev)
        three = node.backward(v, v_depth=v_depth, depth_mode="expected", v_normal=v_normal, normal_mode="accumulated", v_distortion=v_dist)
        three = {k: three[k].cpu().numpy().astype(np.float64) for k in ("v_transforms", "v_sh_coeffs", "v_raw_opacities")}
        only = node.backward(None, v_features=v_map, features=feats)
        ctx.sync()
        want = {k: three[k].reshape(-1) + only[k].cpu().numpy().astype(np.float64).reshape(-1) for k in three}
        want_loss = np.float32(l_img.cpu().numpy()[0])
        for part in (dl, nl, xl, fl):   # (image) + depth + normal + distortion + feature, in f32, in this order
            want_loss = np.float32(want_loss + np.float32(part.cpu().numpy()[0]))
        spl = _splats(ba, sc, dev)
        tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx, feature_field=field)
        store = []
        _capture(tr, store)
        _, st = tr.step(ba.SceneBatch(gt, cam, view_id=2, depth=dgt, features=target), spl)
        ctx.sync()
        assert np.float32(st.loss).tobytes() == want_loss.tobytes(), (st.loss, want_loss)
        assert len(store) == 2
        got = {k: v.reshape(-1) for k, v in _blocks(store[0], n, c).items()}
        _close(got, want, 2 * GRAD_TOL, "step with four terms vs the sum of two hand-composed backwards:")
        _close({"v_features": store[1].cpu().numpy()}, {"v_features": only["v_features"].cpu().numpy()}, GRAD_TOL, "... its v_features:")
    finally:
        ctx.close()


@pytest.mark.parametrize("case", ["window", "pose", "rows", "size"])
def test_refusals_leave_the_step_unqueued(dev, case):
    import brush_amd as ba
    from brush_amd.host import _ptr
    sc = _scene()
    n, ch = sc["transforms"].shape[0], 5
    ctx = ba.Context(dev)
    try:
        cam, gt = util.hip_camera(ba, synth.default_camera_params(W, H)), _gt(dev)
        spl = _splats(ba, sc, dev)
        field, rows = _field(ba, ctx, n, ch, dev)
        good = _target("l1", W, H, ch, dev)
        target = good
        tr = ba.SplatTrainer(ba.TrainConfig(background_color=BG, feature_loss_weight=1.0), median_scene_scale=3.0, ctx=ctx, feature_field=field)
        keep = []
        if case == "window":
            def window(b):
                b.camera.tile_row_begin, b.camera.tile_row_end = 0, 2   # two of the frame's three tile rows
            tr.batch_patch = window
        elif case == "pose":
            buf = torch.zeros((12,), dtype=torch.float32, device=dev)
            keep.append(buf)
            ctx.check(ctx.lib.bh_train_set_pose_grad(ctx._h, _ptr(buf)))
        elif case == "rows":   # what a caller sees who forgot the carry after a refine
            tr.feature_field = _field(ba, ctx, n + 7, ch, dev)[0]
        elif case == "size":
            target = _target("l1", W, H + 16, ch, dev)
        torch.cuda.synchronize()
        with pytest.raises(ba.BrushHipError, match=r"brush_hip error -1: train_step: .*feature term"):
            tr.step(ba.SceneBatch(gt, cam, view_id=2, features=target), spl)
        ctx.check(ctx.lib.bh_train_set_pose_grad(ctx._h, None))
        ctx.sync()
        assert tr.step_count == 0 and tr.feature_field.t == 0 and field.t == 0
        assert np.array_equal(spl.transforms.cpu().numpy(), sc["transforms"]) and np.array_equal(spl.sh_coeffs.cpu().numpy(), sc["sh"])
        assert np.array_equal(spl.raw_opacities.cpu().numpy(), sc["raw_opac"])
        assert np.array_equal(field.features.cpu().numpy(), rows) and not bool(field.m1.any()) and not bool(field.m2.any())
        # the same trainer steps once the obstacle is gone
        tr.batch_patch = None
        tr.feature_field = field
        _, st = tr.step(ba.SceneBatch(gt, cam, view_id=2, features=good), spl)
        ctx.sync()
        assert tr.step_count == 1 and field.t == 1 and math.isfinite(st.loss)
        assert not np.array_equal(field.features.cpu().numpy(), rows)
    finally:
        ctx.close()


def test_set_features_argument_errors(dev):
    import brush_amd as ba
    from brush_amd import _ffi
    ctx = ba.Context(dev)
    try:
        field, _ = _field(ba, ctx, 10, 5, dev)
        target = _target("l1", 16, 16, 5, dev)

        def call(f, ch=5, kind=0, t_ch=5):
            t = _ffi.BhFeatureTarget()
            t.target, t.h, t.w, t.channels, t.kind, t.weight = target.data_ptr(), 16, 16, t_ch, kind, 1.0
            f.channels = ch
            return ctx.lib.bh_train_set_features(ctx._h, C.byref(f), C.byref(t))
        assert call(field.as_struct()) == 0
        no_m1 = field.as_struct()
        no_m1.m1 = None
        assert call(no_m1) == -1
        assert call(field.as_struct(), ch=0, t_ch=0) == -1 and call(field.as_struct(), ch=257, t_ch=257) == -1
        assert call(field.as_struct(), t_ch=4) == -1 and call(field.as_struct(), kind=2) == -1
        assert ctx.lib.bh_train_set_features(ctx._h, None, None) == 0
    finally:
        ctx.close()


def test_the_library_counts_the_updates_of_one_attachment(dev):
    """bh_train_set_features ONCE with step = 0, then two steps: the library's copy of `step` advances with every step that applied
    the term, so the second update is Adam's t = 2 (a count that stood still would re-initialise the moments: t = 1 does).  The
    trainer has no field of its own, so it makes no feature call around its steps; both updates against the host adam_step on the
    captured v_features, bit for bit."""
    import brush_amd as ba
    from brush_amd import _ffi
    sc = _scene()
    n, ch = sc["transforms"].shape[0], 5
    ctx = ba.Context(dev)
    try:
        cam, gt = util.hip_camera(ba, synth.default_camera_params(W, H)), _gt(dev)
        spl = _splats(ba, sc, dev)
        field, _ = _field(ba, ctx, n, ch, dev)
        target = _target("l1", W, H, ch, dev)
        tr = ba.SplatTrainer(ba.TrainConfig(background_color=BG), median_scene_scale=3.0, ctx=ctx)
        store = []
        _capture(tr, store)
        ft = _ffi.BhFeatureTarget()
        ft.target, ft.h, ft.w, ft.channels, ft.kind, ft.weight = target.data_ptr(), H, W, ch, _ffi.FEATURE_LOSS_L1, 1.0
        torch.cuda.synchronize()
        ctx.check(ctx.lib.bh_train_set_features(ctx._h, C.byref(field.as_struct()), C.byref(ft)))
        p, m1, m2 = field.features.clone(), field.m1.clone(), field.m2.clone()
        try:
            for t in (1, 2):
                tr.step(ba.SceneBatch(gt, cam, view_id=2), spl)
                ctx.sync()
                assert len(store) == 2 * t and store[-1].numel() == n * ch
                ba.adam_step(p, store[-1].view(n, ch).contiguous(), m1, m2, field.lr, t, beta1=field.beta1, beta2=field.beta2, eps=field.eps, ctx=ctx)
                ctx.sync()
                assert torch.equal(_bits(field.features), _bits(p)) and torch.equal(_bits(field.m1), _bits(m1)) and torch.equal(_bits(field.m2), _bits(m2)), t
        finally:
            ctx.lib.bh_train_set_features(ctx._h, None, None)
        assert field.t == 0   # (the host's count is the caller's to keep: nobody told it)
    finally:
        ctx.close()


def test_feature_loss_from_iter_starts_the_term_at_that_step(dev):
    one = _one_tile()
    plain, late, info = [], [], {}
    lp, _ = _run(dev, one, 16, 16, 2, "plain", per_step=plain)
    ll, _ = _run(dev, one, 16, 16, 2, "features", cfg_kw=dict(feature_loss_from_iter=2), per_step=late, info=info)
    assert lp[0].tobytes() == ll[0].tobytes()
    for k in plain[0]:
        assert torch.equal(_bits(plain[0][k]), _bits(late[0][k])), k   # step 1 is a plain step, bit for bit
    assert int(torch.count_nonzero(late[0]["f_m1"])) == 0
    assert ll[1] > lp[1] and not torch.equal(_bits(plain[1]["transforms"]), _bits(late[1]["transforms"]))   # step 2 carries the term
    assert info["t"] == 1 and int(torch.count_nonzero(late[1]["f_m1"])) > 0


def test_joint_training_through_a_refine(dev):
    """300 splats, two views, the argmax labels of a 4-channel teacher field, splats training at default rates, a refine in the middle
    that prunes and splits: the field follows the splats (FeatureField.carry inside SplatTrainer.refine), the next step is accepted,
    and the cross-entropy of the first view ends strictly below where it started."""
    import brush_amd as ba
    ch, steps = 4, 40
    cp = synth.default_camera_params(W, H)
    sc = synth.make_scene(300, 0x10A, sh_degree=0, log_scale_range=(math.log(0.1), math.log(0.5)), tan_half_fov=(math.tan(cp["fov_x"] / 2.0), math.tan(cp["fov_y"] / 2.0)))
    sc["raw_opac"][::9] = -7.0   # dead splats: the refine prunes them and refills the budget by splitting
    n = sc["transforms"].shape[0]
    teacher = np.zeros((n, ch), np.float32)
    quadrant = (sc["transforms"][:, 0] > 0).astype(np.int64) * 2 + (sc["transforms"][:, 1] > 0).astype(np.int64)
    teacher[np.arange(n), quadrant] = 4.0
    ctx = ba.Context(dev)
    try:
        cams = [util.hip_camera(ba, cp), util.hip_camera(ba, dict(cp, pos=(0.4, 0.1, -0.3)))]
        gt = _gt(dev)
        spl = _splats(ba, sc, dev)
        labels = []
        for cam in cams:
            node = ba.render_splats_diff(spl, cam, (W, H), BG, ctx=ctx)
            m = ba.render_features(node, torch.from_numpy(teacher).to(dev))
            lab = m.argmax(dim=2).to(torch.uint8)
            lab[m.sum(dim=2) < 0.5] = 255   # (barely covered pixels are ignored)
            labels.append(lab.contiguous())
        ctx.sync()
        assert all(int((lab < ch).sum()) > W * H // 8 for lab in labels)

        def value(spl, field):
            node = ba.render_splats_diff(spl, cams[0], (W, H), BG, ctx=ctx)
            m = ba.render_features(node, field.features)
            loss, _ = ba.feature_loss_value_and_grad(m, labels[0], "cross_entropy", 1.0, want_grad=False, ctx=ctx)
            ctx.sync()
            ok = labels[0] < ch
            acc = float((m.argmax(dim=2)[ok] == labels[0][ok].long()).float().mean())
            loss = loss.cpu().numpy()
            return float(loss[0]) * W * H / float(loss[1]), acc   # the mean over the valid pixels

        field = ba.FeatureField(n, ch, lr=5e-2, device=dev, ctx=ctx)
        first, acc0 = value(spl, field)
        cfg = ba.TrainConfig(background_color=BG, feature_loss_weight=1.0, feature_loss_kind="cross_entropy", total_train_iters=1000)
        tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx, feature_field=field)
        rs = None
        for s in range(steps):
            if s == steps // 2:
                spl, rs = tr.refine(s, spl, seed=77)
                assert rs.num_pruned > 0 and rs.num_added > 0, rs
                assert field.features.shape[0] == rs.total_splats == spl.num_splats() and field.m1.shape == field.m2.shape == field.features.shape
            tr.step(ba.SceneBatch(gt, cams[s % 2], view_id=1 + s % 2, features=labels[s % 2]), spl)   # (the step behind the refine is accepted)
        ctx.sync()
        assert field.t == steps and tr.step_count == steps
        last, acc1 = value(spl, field)
    finally:
        ctx.close()
    print("joint training through a refine (pruned %d, added %d): cross-entropy %.4f -> %.4f (ratio %.3f), pixel accuracy %.3f -> %.3f"
          % (rs.num_pruned, rs.num_added, first, last, last / first, acc0, acc1))
    assert math.isfinite(last) and last < first
