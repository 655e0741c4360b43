"""bh_train_set_bilagrid / SplatTrainer(bilagrid=) (include/brush_hip_bilagrid.h): an identity table at lr 0 and TV
weight 0 changes nothing, a step with a table is the hand-composed render -> slice -> loss [-> LPIPS] -> + tv -> bilagrid backward ->
render backward to the bit (row-marked and zero-filled gradients), a vignetted view learns corner gains below its centre gains, a
checkpointed table resumes to the same bits, and the step refuses a second colour table or an unknown view before it queues
anything.  No seed: the noise terms are zero."""
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import bilagrid_ref as br
import util

pytestmark = pytest.mark.gpu
BG = (0.1, 0.2, 0.3)
W, H = 64, 48
GRID = (16, 16, 8)
SHAPE = (16, 16, 8)


def _scene(n=400, seed=0x3E):
    return synth.make_scene(n, seed, sh_degree=1, log_scale_range=(math.log(0.05), math.log(0.4)),
                            tan_half_fov=(math.tan(math.radians(50)), math.tan(math.radians(50))))


def _gt(dev, w=W, h=H):
    return torch.from_numpy(np.ascontiguousarray(synth.synthetic_gt_packed(w, h)).view(np.int32)).to(dev)


def _splats(ba, sc, dev):
    return ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _g(seed=9):
    return (br.identity_grid(*SHAPE) + np.random.default_rng(seed).uniform(-0.3, 0.3, SHAPE + (12,))).astype(np.float32)


def _run(dev, sc, w, h, steps, with_table):
    import brush_amd as ba
    ctx = ba.Context(dev)
    try:
        spl = _splats(ba, sc, dev)
        tab = ba.BilateralGridTable(2, grid=GRID, lr=0.0, ctx=ctx) if with_table else None
        tr = ba.SplatTrainer(ba.TrainConfig(background_color=BG), median_scene_scale=3.0, ctx=ctx, bilagrid=tab, bilagrid_tv_weight=0.0)
        cam, gt, losses = util.hip_camera(ba, synth.default_camera_params(w, h)), _gt(dev, w, h), []
        for _ in range(steps):
            _, st = tr.step(ba.SceneBatch(gt, cam, view_id=2), spl)
            ctx.sync()
            losses.append(np.float32(st.loss))
        out = {"transforms": spl.transforms.clone(), "sh": spl.sh_coeffs.clone(), "opac": spl.raw_opacities.clone()}
        out.update({k: v.clone() for k, v in tr.state.items()})
        if tab is not None:
            ident = br.identity_grid(*SHAPE).astype(np.float32)
            assert np.array_equal(tab.params[0], ident) and np.array_equal(tab.params[1], ident)
            assert tab.state(2)[2] == steps and tab.state(1)[2] == 0
        return losses, out
    finally:
        ctx.close()


def test_identity_table_at_lr_zero_changes_nothing(dev):
    sc = _scene()
    plain, _ = _run(dev, sc, W, H, 1, False)
    on, _ = _run(dev, sc, W, H, 1, True)
    assert math.isfinite(plain[0]) and plain[0].tobytes() == on[0].tobytes(), (plain, on)
    # ONE 16x16 tile (tests/test_gpu_pose_train.py): whole steps repeat bit for bit, so the splats can be compared too
    one = synth.make_scene(6000, 0xD0A, sh_degree=1, log_scale_range=(math.log(0.05), math.log(0.4)),
                           tan_half_fov=(math.tan(math.radians(50)), math.tan(math.radians(50))))
    lp, a = _run(dev, one, 16, 16, 3, False)
    lo, b = _run(dev, one, 16, 16, 3, True)
    assert [v.tobytes() for v in lp] == [v.tobytes() for v in lo]
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


@pytest.fixture(scope="module")
def lpips_model(dev):
    import brush_amd as ba
    m = ba.Lpips.from_params(ba.Lpips.random_params(seed=5), ctx=ba.get_context(dev))
    yield m
    m.close()


@pytest.mark.parametrize("mode", ["plain", "zero_grads", "lpips", "pose"])
def test_step_equals_the_hand_composed_path(dev, mode, lpips_model):
    import brush_amd as ba
    from brush_amd.host import _ptr
    sc = _scene()
    cam = util.hip_camera(ba, synth.default_camera_params(W, H))
    gt = _gt(dev)
    lw = 0.2 if mode == "lpips" else 0.0
    tvw = 10.0
    cfg = ba.TrainConfig(exact_lists=True, background_color=BG, lpips_loss_weight=lw)
    ctx = ba.Context(dev, options={"zero_grads": 1} if mode == "zero_grads" else {})
    try:
        # by hand on the untouched splats: render, slice, the step's loss and its gradient, [LPIPS on the sliced image,] the TV term,
        # the bilagrid backward with its update on a second table in the same state, [the pose backward of v_img]
        hand = ba.BilateralGridTable(2, grid=GRID, lr=0.01, ctx=ctx)
        hand.set_view(2, _g())
        spl0 = _splats(ba, sc, dev)
        node = ba.render_splats_diff(spl0, cam, (W, H), BG, ctx=ctx)
        x = node.img.clone()
        y = hand.slice(2, x)
        l_img, v = ba.image_loss_value_and_grad(y, gt, l1_weight=1.0 - cfg.ssim_weight, ssim_weight=-cfg.ssim_weight, ctx=ctx)
        want_loss = np.float32(l_img.cpu().numpy()[0])
        if mode == "lpips":
            lv, v = ba.lpips_value_and_grad(y, gt, lpips_model, weight=lw, v_output=v, ctx=ctx)
            want_loss = np.float32(want_loss + np.float32(lv.cpu().numpy()[0]) * np.float32(lw))
        tv = np.float32(hand.tv(2).cpu().numpy()[0])
        want_loss = np.float32(want_loss + np.float32(np.float32(tvw) * tv))
        v_img = hand.backward(2, x, v, tv_weight=tvw, update=True)
        want_pose = None
        if mode == "pose":
            want_pose = node.backward(v_img, pose=True)["v_viewmat"].cpu().numpy().astype(np.float64)
        # the step
        tab = ba.BilateralGridTable(2, grid=GRID, lr=0.01, ctx=ctx)
        tab.set_view(2, _g())
        spl = _splats(ba, sc, dev)
        tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx, bilagrid=tab, bilagrid_tv_weight=tvw, lpips=lpips_model if mode == "lpips" else None)
        buf = torch.full((12,), float("nan"), device=dev)
        if mode == "pose":
            ctx.check(ctx.lib.bh_train_set_pose_grad(ctx._h, _ptr(buf)))
        _, st = tr.step(ba.SceneBatch(gt, cam, view_id=2), spl)
        ctx.check(ctx.lib.bh_train_set_pose_grad(ctx._h, None))
        ctx.sync()
        assert tv > 0 and np.float32(st.loss).tobytes() == want_loss.tobytes(), (st.loss, want_loss)
        assert np.array_equal(tab.grads.view(np.int32), hand.grads.view(np.int32)) and tab.grads[1].any()
        assert np.array_equal(tab.params.view(np.int32), hand.params.view(np.int32))
        assert not np.array_equal(tab.params[1], _g()) and np.array_equal(tab.params[0], br.identity_grid(*SHAPE).astype(np.float32))
        for a, b in zip(tab.state(2), hand.state(2)):
            assert np.array_equal(a, b)
        assert tab.state(1)[2] == 0 and not tab.grads[0].any()
        if mode == "pose":
            import pose_ref
            got = buf.cpu().numpy().astype(np.float64)
            with torch.enable_grad():
                mass = pose_ref.pose_gradients(sc, synth.default_camera_params(W, H), W, H, v_img.cpu().numpy(), bg=BG)["S"]
            ratio = np.abs(got - want_pose) / mass
            print("pose buffer vs hand-composed v_img: max |delta_k| / S_k = %.3e (bound 1e-4)" % ratio.max())
            assert np.isfinite(got).all() and np.abs(want_pose).max() > 0 and (np.abs(got - want_pose) <= 1e-4 * mass).all(), ratio
    finally:
        ctx.close()


def _vignetted(gt_packed, w, h, depth=0.5):
    """The packed rgba8 image with its rgb darkened towards the corners: x (1 - depth r^2), r = 1 in the corners; alpha kept."""
    b = gt_packed.cpu().numpy().view(np.uint8).reshape(h, w, 4).astype(np.float64)
    yy, xx = np.mgrid[0:h, 0:w]
    r2 = 0.5 * (((xx + 0.5) / w * 2 - 1) ** 2 + ((yy + 0.5) / h * 2 - 1) ** 2)
    b[..., :3] = np.clip(np.rint(b[..., :3] * (1.0 - depth * r2)[..., None]), 0, 255)
    return torch.from_numpy(np.ascontiguousarray(b.astype(np.uint8)).view(np.int32).reshape(gt_packed.shape)).to(gt_packed.device)


VIGNETTE_STEPS = 120


def test_a_vignetted_view_learns_darker_corners(dev):
    import brush_amd as ba
    sc = _scene()
    cams = [util.hip_camera(ba, synth.default_camera_params(W, H)), util.hip_camera(ba, dict(synth.default_camera_params(W, H), pos=(0.4, 0.1, synth.default_camera_params(W, H)["pos"][2])))]
    ctx = ba.Context(dev)
    try:
        teacher = _splats(ba, sc, dev)
        gts = [ba.render_splats(teacher, c, (W, H), BG, ctx=ctx)[0] for c in cams]
        gts[1] = _vignetted(gts[1], W, H)
        spl = _splats(ba, sc, dev)
        tab = ba.BilateralGridTable(2, grid=GRID, lr=0.01, ctx=ctx)
        tr = ba.SplatTrainer(ba.TrainConfig(background_color=BG), median_scene_scale=3.0, ctx=ctx, bilagrid=tab)
        for s in range(VIGNETTE_STEPS):
            tr.step(ba.SceneBatch(gts[s % 2], cams[s % 2], view_id=1 + s % 2), spl)
        p = tab.params.astype(np.float64)

        def gain(view, js, is_):
            cells = p[view][np.ix_(js, is_)]   # [.., .., L, 12]
            return float(np.mean([cells[..., 0], cells[..., 5], cells[..., 10]]))

        corner = gain(1, [0, 15], [0, 15])
        centre = gain(1, [7, 8], [7, 8])
        print("mean diagonal gain of view 2 (vignetted GT) after %d alternating steps: corner cells %.4f, centre cells %.4f; view 1 corner %.4f"
              % (VIGNETTE_STEPS, corner, centre, gain(0, [0, 15], [0, 15])))
        assert tab.state(1)[2] == tab.state(2)[2] == VIGNETTE_STEPS // 2
        assert corner < centre and corner < 1.0, (corner, centre)
    finally:
        ctx.close()


def test_checkpoint_round_trip_resumes_to_the_same_bits(dev):
    import brush_amd as ba
    rng = np.random.default_rng(4)
    x = torch.from_numpy(rng.uniform(0.0, 1.0, (H, W, 4)).astype(np.float32)).to(dev)
    vs = [torch.from_numpy(rng.uniform(-1.0, 1.0, (H, W, 4)).astype(np.float32)).to(dev) for _ in range(5)]
    ctx = ba.Context(dev)
    try:
        a = ba.BilateralGridTable(3, grid=GRID, lr=0.02, ctx=ctx)
        a.set_view(3, _g(2))
        for v in vs[:3]:
            a.backward(3, x, v, tv_weight=10.0, update=True)
        b = ba.BilateralGridTable(3, grid=GRID, lr=0.02, ctx=ctx)
        b.params = a.params
        for k in (1, 2, 3):
            b.set_state(k, *a.state(k))
        assert b.state(3)[2] == 3 and b.state(1)[2] == 0
        for v in vs[3:]:
            a.backward(3, x, v, tv_weight=10.0, update=True)
            b.backward(3, x, v, tv_weight=10.0, update=True)
        assert np.array_equal(a.params.view(np.int32), b.params.view(np.int32)) and not np.array_equal(a.params[2], _g(2))
        for k in (1, 2, 3):
            for p, q in zip(a.state(k), b.state(k)):
                assert np.array_equal(p, q)
    finally:
        ctx.close()


def _corrected_step(ba, ctx, sc, dev, w, h, kind):
    """One train step of the untouched scene `sc` with a colour table of `kind` on `ctx`: the loss, the splats and the table afterwards."""
    spl = _splats(ba, sc, dev)
    if kind == "exposure":
        tab = ba.ExposureTable(2, lr=0.01, ctx=ctx)
        tab.set_view(2, (np.eye(3, 4).reshape(12) + np.random.default_rng(5).uniform(-0.2, 0.2, 12)).astype(np.float32))
        tr = ba.SplatTrainer(ba.TrainConfig(background_color=BG), median_scene_scale=3.0, ctx=ctx, exposure=tab)
    else:
        tab = ba.BilateralGridTable(2, grid=GRID, lr=0.01, ctx=ctx)
        tab.set_view(2, _g())
        tr = ba.SplatTrainer(ba.TrainConfig(background_color=BG), median_scene_scale=3.0, ctx=ctx, bilagrid=tab, bilagrid_tv_weight=10.0)
    _, st = tr.step(ba.SceneBatch(_gt(dev, w, h), util.hip_camera(ba, synth.default_camera_params(w, h)), view_id=2), spl)
    ctx.sync()
    out = dict(loss=np.float32(st.loss), params=tab.params, grads=tab.grads, transforms=spl.transforms.cpu().numpy(),
               sh=spl.sh_coeffs.cpu().numpy(), opac=spl.raw_opacities.cpu().numpy())
    assert tab.state(2)[2] == 1 and out["grads"][1].any()
    tab.close()
    return out


@pytest.mark.parametrize("w,h", [(W, H), (16, 16)])
def test_both_colour_tables_take_turns_on_one_context(dev, w, h):
    """The exposed frame and the sliced frame share one scratch slot of the context: a step with an exposure table, then a step with a
    bilateral-grid table on the SAME context (the trainer detaches its table after every step) give what each gives on a context of its
    own — the loss, the table's gradient and its updated parameters bit for bit.  Both steps start from the untouched scene, so that
    the second does not inherit the first one's splats: at 64x48 (twelve tiles) an updated splat is reproducible only up to the order of
    the blend backward's float atomics (tests/test_gpu_options.py), so there the splats are held to util.assert_adam_close, and to the
    bit on the one-tile frame, where whole steps repeat (tests/test_gpu_pose_train.py)."""
    import brush_amd as ba
    one_tile = (w, h) == (16, 16)
    sc = synth.make_scene(6000, 0xD0A, sh_degree=1, log_scale_range=(math.log(0.05), math.log(0.4)),
                          tan_half_fov=(math.tan(math.radians(50)), math.tan(math.radians(50)))) if one_tile else _scene()
    shared = ba.Context(dev)
    try:
        got = [_corrected_step(ba, shared, sc, dev, w, h, kind) for kind in ("exposure", "bilagrid")]
    finally:
        shared.close()
    cfg = ba.TrainConfig()
    for kind, a in zip(("exposure", "bilagrid"), got):
        fresh = ba.Context(dev)
        try:
            b = _corrected_step(ba, fresh, sc, dev, w, h, kind)
        finally:
            fresh.close()
        assert math.isfinite(a["loss"]) and a["loss"].tobytes() == b["loss"].tobytes(), (kind, a["loss"], b["loss"])
        assert np.array_equal(a["params"].view(np.int32), b["params"].view(np.int32)), kind
        assert np.array_equal(a["grads"].view(np.int32), b["grads"].view(np.int32)), kind
        if one_tile:
            for k in ("transforms", "sh", "opac"):
                assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), (kind, k)
        else:
            util.assert_adam_close(a["transforms"][:, 3:7], b["transforms"][:, 3:7], cfg.lr_rotation, 1, kind + " rotation")
            util.assert_adam_close(a["transforms"][:, 7:10], b["transforms"][:, 7:10], cfg.lr_scale, 1, kind + " scale")
            util.assert_adam_close(a["opac"], b["opac"], cfg.lr_opac, 1, kind + " opacity")


def test_step_refuses_a_second_colour_table_and_an_unknown_view(dev):
    import brush_amd as ba
    sc = _scene()
    cam, gt = util.hip_camera(ba, synth.default_camera_params(W, H)), _gt(dev)
    ctx = ba.Context(dev)
    try:
        spl = _splats(ba, sc, dev)
        kept = {"transforms": spl.transforms.clone(), "sh": spl.sh_coeffs.clone(), "opac": spl.raw_opacities.clone()}
        tab = ba.BilateralGridTable(2, grid=GRID, lr=0.01, ctx=ctx)
        tab.set_view(2, _g())
        exp = ba.ExposureTable(2, ctx=ctx)
        tr = ba.SplatTrainer(ba.TrainConfig(background_color=BG), median_scene_scale=3.0, ctx=ctx, bilagrid=tab)
        ctx.check(ctx.lib.bh_train_set_exposure(ctx._h, exp._h))
        with pytest.raises(ba.BrushHipError, match="alternatives"):
            tr.step(ba.SceneBatch(gt, cam, view_id=2), spl)
        ctx.check(ctx.lib.bh_train_set_exposure(ctx._h, None))
        for view in (0, 3):
            with pytest.raises(ba.BrushHipError, match="view_id must be 1 .. n_views"):
                tr.step(ba.SceneBatch(gt, cam, view_id=view), spl)
        ctx.sync()
        assert tr.step_count == 0 and tab.state(2)[2] == 0 and tab.state(1)[2] == 0 and not tab.grads.any()
        assert np.array_equal(tab.params[1], _g()) and not exp.grads.any()
        for k, v in kept.items():
            assert torch.equal(_bits(v), _bits({"transforms": spl.transforms, "sh": spl.sh_coeffs, "opac": spl.raw_opacities}[k])), k
        _, st = tr.step(ba.SceneBatch(gt, cam, view_id=2), spl)   # and the trainer still works
        ctx.sync()
        assert math.isfinite(st.loss) and tab.state(2)[2] == 1
    finally:
        ctx.close()
