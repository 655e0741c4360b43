"""bh_train_set_exposure / SplatTrainer(exposure=) (include/brush_hip_exposure.h): an identity table at lr 0 changes
nothing, a step with a table is the hand-composed render -> apply -> loss [-> LPIPS] -> exposure backward -> render backward to the
bit, a darker view learns a gain below 1, and a checkpointed table resumes to the same bits.  No seed: the noise terms are zero."""
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import exposure_ref as er
import util

pytestmark = pytest.mark.gpu
BG = (0.1, 0.2, 0.3)
W, H = 64, 48


def _scene(n=400, seed=0x3E):
    return synth.make_scene(n, seed, sh_degree=1, log_scale_range=(math.log(0.05), math.log(0.4)),
                            tan_half_fov=(math.tan(math.radians(50)), math.tan(math.radians(50))))


def _gt(dev, w=W, h=H):
    return torch.from_numpy(np.ascontiguousarray(synth.synthetic_gt_packed(w, h)).view(np.int32)).to(dev)


def _splats(ba, sc, dev):
    return ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _m(seed=9):
    return (er.IDENTITY + np.random.default_rng(seed).uniform(-0.3, 0.3, 12)).astype(np.float32)


def _run(dev, sc, w, h, steps, with_table):
    import brush_amd as ba
    ctx = ba.Context(dev)
    try:
        spl = _splats(ba, sc, dev)
        tab = ba.ExposureTable(2, lr=0.0, ctx=ctx) if with_table else None
        tr = ba.SplatTrainer(ba.TrainConfig(background_color=BG), median_scene_scale=3.0, ctx=ctx, exposure=tab)
        cam, gt, losses = util.hip_camera(ba, synth.default_camera_params(w, h)), _gt(dev, w, h), []
        for _ in range(steps):
            _, st = tr.step(ba.SceneBatch(gt, cam, view_id=2), spl)
            ctx.sync()
            losses.append(np.float32(st.loss))
        out = {"transforms": spl.transforms.clone(), "sh": spl.sh_coeffs.clone(), "opac": spl.raw_opacities.clone()}
        out.update({k: v.clone() for k, v in tr.state.items()})
        if tab is not None:
            assert np.array_equal(tab.params, np.tile(er.IDENTITY.astype(np.float32), (2, 1))) and tab.state(2)[2] == steps and tab.state(1)[2] == 0
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


@pytest.mark.parametrize("mode", ["plain", "lpips", "pose"])
def test_step_equals_the_hand_composed_path(dev, mode, lpips_model):
    import brush_amd as ba
    from brush_amd.host import _ptr
    sc = _scene()
    cam = util.hip_camera(ba, synth.default_camera_params(W, H))
    gt = _gt(dev)
    lw = 0.2 if mode == "lpips" else 0.0
    cfg = ba.TrainConfig(exact_lists=True, background_color=BG, lpips_loss_weight=lw)
    ctx = ba.Context(dev)
    try:
        # by hand on the untouched splats: render, apply, the step's loss and its gradient, [LPIPS on the exposed image,] the
        # exposure backward with its update on a second table in the same state, [the pose backward of A^T v']
        hand = ba.ExposureTable(2, lr=0.01, ctx=ctx)
        hand.set_view(2, _m())
        spl0 = _splats(ba, sc, dev)
        node = ba.render_splats_diff(spl0, cam, (W, H), BG, ctx=ctx)
        x = node.img.clone()
        y = hand.apply(2, x)
        l_img, v = ba.image_loss_value_and_grad(y, gt, l1_weight=1.0 - cfg.ssim_weight, ssim_weight=-cfg.ssim_weight, ctx=ctx)
        want_loss = np.float32(l_img.cpu().numpy()[0])
        if mode == "lpips":
            lv, v = ba.lpips_value_and_grad(y, gt, lpips_model, weight=lw, v_output=v, ctx=ctx)
            want_loss = np.float32(want_loss + np.float32(lv.cpu().numpy()[0]) * np.float32(lw))
        v_img = hand.backward(2, x, v, update=True)
        want_pose = None
        if mode == "pose":
            want_pose = node.backward(v_img, pose=True)["v_viewmat"].cpu().numpy().astype(np.float64)
        # the step
        tab = ba.ExposureTable(2, lr=0.01, ctx=ctx)
        tab.set_view(2, _m())
        spl = _splats(ba, sc, dev)
        tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx, exposure=tab, lpips=lpips_model if mode == "lpips" else None)
        buf = torch.full((12,), float("nan"), device=dev)
        if mode == "pose":
            ctx.check(ctx.lib.bh_train_set_pose_grad(ctx._h, _ptr(buf)))
        _, st = tr.step(ba.SceneBatch(gt, cam, view_id=2), spl)
        ctx.check(ctx.lib.bh_train_set_pose_grad(ctx._h, None))
        ctx.sync()
        assert np.float32(st.loss).tobytes() == want_loss.tobytes(), (st.loss, want_loss)
        assert np.array_equal(tab.grads.view(np.int32), hand.grads.view(np.int32)) and tab.grads[1].any()
        assert np.array_equal(tab.params.view(np.int32), hand.params.view(np.int32))
        assert not np.array_equal(tab.params[1], _m()) and np.array_equal(tab.params[0], er.IDENTITY.astype(np.float32))
        for a, b in zip(tab.state(2), hand.state(2)):
            assert np.array_equal(a, b)
        assert tab.state(1)[2] == 0 and not tab.grads[0].any()
        if mode == "pose":
            import pose_ref
            got = buf.cpu().numpy().astype(np.float64)
            with torch.enable_grad():
                mass = pose_ref.pose_gradients(sc, synth.default_camera_params(W, H), W, H, v_img.cpu().numpy(), bg=BG)["S"]
            ratio = np.abs(got - want_pose) / mass
            print("pose buffer vs hand-composed A^T v': max |delta_k| / S_k = %.3e (bound 1e-4)" % ratio.max())
            assert np.isfinite(got).all() and np.abs(want_pose).max() > 0 and (np.abs(got - want_pose) <= 1e-4 * mass).all(), ratio
    finally:
        ctx.close()


def _darker(gt_packed, gain):
    """The packed rgba8 image with its rgb multiplied by `gain` (rounded to bytes), alpha kept."""
    b = gt_packed.cpu().numpy().view(np.uint8).reshape(-1, 4).astype(np.float64)
    b[:, :3] = np.clip(np.rint(b[:, :3] * gain), 0, 255)
    return torch.from_numpy(np.ascontiguousarray(b.astype(np.uint8)).view(np.int32).reshape(gt_packed.shape)).to(gt_packed.device)


# The same loop on the CPU (exposure_ref.darker_view_loop: the oracle's train step with exposure_ref around its loss, GT bytes from
# the oracle's render, 120 alternating steps at lr 0.01) ends with mean diagonal gains of 1.0619 (view 1) and 0.8558 (view 2, GT x 0.7)
# — the cross terms, the offsets and the splats take the rest of the 0.7.  The test asks for half that movement.
DARK_STEPS = 120
DARK_RECORDED_GAIN = 0.8558


def test_a_darker_view_learns_a_gain_below_one(dev):
    import brush_amd as ba
    sc = _scene()
    cams = [util.hip_camera(ba, synth.default_camera_params(W, H)), util.hip_camera(ba, dict(synth.default_camera_params(W, H), pos=(0.4, 0.1, synth.default_camera_params(W, H)["pos"][2])))]
    ctx = ba.Context(dev)
    try:
        teacher = _splats(ba, sc, dev)
        gts = [ba.render_splats(teacher, c, (W, H), BG, ctx=ctx)[0] for c in cams]
        gts[1] = _darker(gts[1], 0.7)
        spl = _splats(ba, sc, dev)
        tab = ba.ExposureTable(2, lr=0.01, ctx=ctx)
        tr = ba.SplatTrainer(ba.TrainConfig(background_color=BG), median_scene_scale=3.0, ctx=ctx, exposure=tab)
        for s in range(DARK_STEPS):
            tr.step(ba.SceneBatch(gts[s % 2], cams[s % 2], view_id=1 + s % 2), spl)
        p = tab.params.astype(np.float64)
        gain = [float(np.mean([p[k][0], p[k][5], p[k][10]])) for k in (0, 1)]
        print("mean diagonal gain after %d alternating steps: view 1 %.4f, view 2 (GT x 0.7) %.4f" % (DARK_STEPS, gain[0], gain[1]))
        assert tab.state(1)[2] == tab.state(2)[2] == DARK_STEPS // 2
        assert gain[1] < gain[0] and gain[1] < 1.0 - 0.5 * (1.0 - DARK_RECORDED_GAIN), gain
    finally:
        ctx.close()


def test_checkpoint_round_trip_resumes_to_the_same_bits(dev):
    import brush_amd as ba
    rng = np.random.default_rng(4)
    x = torch.from_numpy(rng.uniform(0.0, 1.0, (H, W, 4)).astype(np.float32)).to(dev)
    vs = [torch.from_numpy((rng.uniform(-1.0, 1.0, (H, W, 4)) + 0.25).astype(np.float32)).to(dev) for _ in range(5)]
    ctx = ba.Context(dev)
    try:
        a = ba.ExposureTable(3, lr=0.02, ctx=ctx)
        a.set_view(3, _m(2))
        for v in vs[:3]:
            a.backward(3, x, v, update=True)
        b = ba.ExposureTable(3, lr=0.02, ctx=ctx)
        b.params = a.params
        for k in (1, 2, 3):
            b.set_state(k, *a.state(k))
        assert b.state(3)[2] == 3 and b.state(1)[2] == 0
        for v in vs[3:]:
            a.backward(3, x, v, update=True)
            b.backward(3, x, v, update=True)
        assert np.array_equal(a.params.view(np.int32), b.params.view(np.int32)) and not np.array_equal(a.params[2], _m(2))
        for k in (1, 2, 3):
            for p, q in zip(a.state(k), b.state(k)):
                assert np.array_equal(p, q)
    finally:
        ctx.close()
