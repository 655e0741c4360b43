"""bh_train_set_envmap / SplatTrainer(envmap=) (include/brush_hip_envmap.h): a black map at lr 0 changes nothing, a step
with a map is the hand-composed render -> composite -> loss [-> LPIPS] [-> exposure | bilagrid] -> their backward -> map backward ->
render backward to the bit, an identity gradient hook is handed v_E once, every refusal of the term is met before anything is queued,
and a map learns a teacher's sky behind frozen splats.  No seed: the noise terms are zero.  Scenes and sizes are those of
tests/test_gpu_exposure_train.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import bilagrid_ref as br
import envmap_ref as vr
import exposure_ref as er
import util

pytestmark = pytest.mark.gpu
BLACK = (0.0, 0.0, 0.0)
W, H = 64, 48
RES = 8
GRID = (16, 16, 8)


def _scene(n=400, seed=0x3E):
    return synth.make_scene(n, seed, sh_degree=1, log_scale_range=(math.log(0.05), math.log(0.4)),
                            tan_half_fov=(math.tan(math.radians(50)), math.tan(math.radians(50))))


def _gt(dev, w=W, h=H):
    return torch.from_numpy(np.ascontiguousarray(synth.synthetic_gt_packed(w, h)).view(np.int32)).to(dev)


def _splats(ba, sc, dev):
    return ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))


def _table(res=RES, seed=11, lo=0.2, hi=0.8):
    return np.random.default_rng(seed).uniform(lo, hi, (6, res, res, 3)).astype(np.float32)


def _run(dev, sc, w, h, steps, with_map):
    import brush_amd as ba
    ctx = ba.Context(dev)
    try:
        spl = _splats(ba, sc, dev)
        env = ba.EnvironmentMap(RES, lr=0.0, ctx=ctx) if with_map else None
        tr = ba.SplatTrainer(ba.TrainConfig(background_color=BLACK), median_scene_scale=3.0, ctx=ctx, envmap=env)
        cam, gt, losses = util.hip_camera(ba, synth.default_camera_params(w, h)), _gt(dev, w, h), []
        for _ in range(steps):
            _, st = tr.step(ba.SceneBatch(gt, cam, view_id=2), spl)
            ctx.sync()
            losses.append(np.float32(st.loss))
        out = {"transforms": spl.transforms.clone(), "sh": spl.sh_coeffs.clone(), "opac": spl.raw_opacities.clone()}
        out.update({k: v.clone() for k, v in tr.state.items()})
        if env is not None:
            assert not env.params.any() and env.state()[2] == steps and env.grads.any()
        return losses, out
    finally:
        ctx.close()


def test_black_map_at_lr_zero_changes_nothing(dev):
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


def _colour_table(ba, mode, ctx):
    if mode == "exposure":
        t = ba.ExposureTable(2, lr=0.01, ctx=ctx)
        t.set_view(2, (er.IDENTITY + np.random.default_rng(9).uniform(-0.3, 0.3, 12)).astype(np.float32))
        return t
    if mode == "bilagrid":
        t = ba.BilateralGridTable(2, grid=GRID, lr=0.01, ctx=ctx)
        t.set_view(2, (br.identity_grid(*GRID) + np.random.default_rng(9).uniform(-0.3, 0.3, GRID + (12,))).astype(np.float32))
        return t
    return None


@pytest.mark.parametrize("mode", ["plain", "lpips", "exposure", "bilagrid"])
def test_step_equals_the_hand_composed_path(dev, mode, lpips_model):
    import brush_amd as ba
    sc = _scene()
    cam = util.hip_camera(ba, synth.default_camera_params(W, H))
    gt = _gt(dev)
    lw = 0.2 if mode == "lpips" else 0.0
    tvw = 10.0
    cfg = ba.TrainConfig(exact_lists=True, background_color=BLACK, lpips_loss_weight=lw)
    ctx = ba.Context(dev)
    try:
        # by hand on the untouched splats: render on black, composite, [expose | slice the composited frame,] the step's loss and its
        # gradient, [LPIPS,] [the colour table's backward with x = the composited frame,] the map's backward with its update
        hand, hand_tab = ba.EnvironmentMap(RES, lr=0.01, ctx=ctx), _colour_table(ba, mode, ctx)
        hand.params = _table()
        spl0 = _splats(ba, sc, dev)
        node = ba.render_splats_diff(spl0, cam, (W, H), BLACK, ctx=ctx)
        x = node.img.clone()
        y = hand.composite(x, cam)
        assert not torch.equal(y, x)
        z = y if hand_tab is None else (hand_tab.apply(2, y) if mode == "exposure" else hand_tab.slice(2, y))
        l_img, v = ba.image_loss_value_and_grad(z, gt, l1_weight=1.0 - cfg.ssim_weight, ssim_weight=-cfg.ssim_weight, ctx=ctx)
        want_loss = np.float32(l_img.cpu().numpy()[0])
        if mode == "lpips":
            lv, v = ba.lpips_value_and_grad(z, gt, lpips_model, weight=lw, v_output=v, ctx=ctx)
            want_loss = np.float32(want_loss + np.float32(lv.cpu().numpy()[0]) * np.float32(lw))
        if mode == "exposure":
            v = hand_tab.backward(2, y, v, update=True)
        if mode == "bilagrid":
            want_loss = np.float32(want_loss + np.float32(np.float32(tvw) * np.float32(hand_tab.tv(2).cpu().numpy()[0])))
            v = hand_tab.backward(2, y, v, tv_weight=tvw, update=True)
        v_img = hand.backward(x, cam, v, update=True)
        assert bool((v_img[..., 3] != v[..., 3]).any())   # the sky pulls on alpha
        # the step
        env, tab = ba.EnvironmentMap(RES, lr=0.01, ctx=ctx), _colour_table(ba, mode, ctx)
        env.params = _table()
        spl = _splats(ba, sc, dev)
        tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx, envmap=env, lpips=lpips_model if mode == "lpips" else None,
                             exposure=tab if mode == "exposure" else None, bilagrid=tab if mode == "bilagrid" else None, bilagrid_tv_weight=tvw)
        _, st = tr.step(ba.SceneBatch(gt, cam, view_id=2), spl)
        ctx.sync()
        assert np.float32(st.loss).tobytes() == want_loss.tobytes(), (st.loss, want_loss)
        assert _same(env.grads, hand.grads) and env.grads.any()
        assert _same(env.params, hand.params) and not _same(env.params, _table())
        for a, b in zip(env.state(), hand.state()):
            assert np.array_equal(a, b)
        assert env.state()[2] == 1
        if tab is not None:
            assert np.array_equal(tab.grads.view(np.int32), hand_tab.grads.view(np.int32)) and tab.grads[1].any()
            assert np.array_equal(tab.params.view(np.int32), hand_tab.params.view(np.int32))
    finally:
        ctx.close()


def test_an_identity_hook_is_handed_the_table_gradient_once(dev):
    import brush_amd as ba
    from brush_amd import _ffi
    from brush_amd.host import _view
    sc = _scene()
    cam, gt = util.hip_camera(ba, synth.default_camera_params(W, H)), _gt(dev)
    ctx = ba.Context(dev)
    try:
        env = ba.EnvironmentMap(RES, lr=0.01, ctx=ctx)
        env.params = _table()
        spl = _splats(ba, sc, dev)
        tr = ba.SplatTrainer(ba.TrainConfig(exact_lists=True, background_color=BLACK), median_scene_scale=3.0, ctx=ctx, envmap=env)
        store = []

        def hook(_user, ptr, count):
            try:
                store.append(_view(ptr, (int(count),), torch.float32, dev).clone())
                return 0
            except Exception:
                return 1
        tr._hook = _ffi.GRAD_HOOK(hook)
        tr._world = 1
        tr.pg = object()   # (only its presence matters: the step takes the hook above, partition "cameras")
        tr.sparse_exchange = False
        tr.step(ba.SceneBatch(gt, cam, view_id=2), spl)
        ctx.sync()
        cells = 6 * RES * RES * 3
        assert [int(t.numel()) for t in store].count(cells) == 1 and len(store) == 2 and int(store[1].numel()) == cells
        grads = env.grads
        assert _same(store[1].cpu().numpy().reshape(grads.shape), grads) and grads.any()
        # the update came behind the hook, on the summed gradient
        want, m1, m2, t = vr.adam_step(_table(), np.zeros_like(grads), np.zeros_like(grads), 0, grads, 0.01)
        got_m1, got_m2, got_t = env.state()
        assert got_t == t == 1 and _same(env.params, want) and _same(got_m1, m1) and _same(got_m2, m2)
    finally:
        ctx.close()


@pytest.mark.parametrize("case", ["fisheye", "window", "image_hook", "pose", "alpha"])
def test_refusals_queue_nothing(dev, case):
    import brush_amd as ba
    from brush_amd import _ffi
    from brush_amd.host import _ptr
    sc = _scene()
    ctx = ba.Context(dev)
    try:
        params = synth.default_camera_params(W, H)
        good_cam = util.hip_camera(ba, params)
        cam = util.hip_camera(ba, dict(params, model=util.REF_LENSES["kb4"][0], dist=util.REF_LENSES["kb4"][1])) if case == "fisheye" else good_cam
        gt = _gt(dev)
        spl = _splats(ba, sc, dev)
        env = ba.EnvironmentMap(RES, lr=0.01, ctx=ctx)
        env.params = _table()
        tr = ba.SplatTrainer(ba.TrainConfig(background_color=BLACK), median_scene_scale=3.0, ctx=ctx, envmap=env)
        keep, batch = [], ba.SceneBatch(gt, cam, view_id=2)
        if case == "window":
            def window(b):
                b.camera.tile_row_begin, b.camera.tile_row_end = 0, 2   # two of the frame's three tile rows
            tr.batch_patch = window
        elif case == "image_hook":
            cb = _ffi.IMAGE_HOOK(lambda *a: 0)
            keep.append(cb)

            def hooked(b):
                b.image_hook = C.cast(cb, C.c_void_p)
            tr.batch_patch = hooked
        elif case == "pose":
            buf = torch.zeros((12,), dtype=torch.float32, device=dev)
            keep.append(buf)
            ctx.check(ctx.lib.bh_train_set_pose_grad(ctx._h, _ptr(buf)))
        elif case == "alpha":
            batch = ba.SceneBatch(gt, cam, has_alpha=True, alpha_is_mask=False, view_id=2)
        torch.cuda.synchronize()
        pattern = {"fisheye": "pinhole", "window": "whole frame", "image_hook": "whole frame", "pose": "pose-gradient", "alpha": "real alpha"}[case]
        with pytest.raises(ba.BrushHipError, match=r"brush_hip error -1: train_step: .*environment map.*" + pattern):
            tr.step(batch, spl)
        ctx.check(ctx.lib.bh_train_set_pose_grad(ctx._h, None))
        ctx.sync()
        assert tr.step_count == 0 and env.state()[2] == 0 and _same(env.params, _table()) and not env.grads.any()
        assert np.array_equal(spl.transforms.cpu().numpy(), sc["transforms"]) and np.array_equal(spl.raw_opacities.cpu().numpy(), sc["raw_opac"])
        # the same trainer steps once the obstacle is gone; a mask is fine
        tr.batch_patch = None
        _, st = tr.step(ba.SceneBatch(gt, good_cam, has_alpha=True, alpha_is_mask=True, view_id=2), spl)
        ctx.sync()
        assert math.isfinite(st.loss) and tr.step_count == 1 and env.state()[2] == 1
    finally:
        ctx.close()


def _pack(rgb):
    """[H,W,3] f32 in 0 .. 1 -> rgba8 [H,W] as int32, opaque."""
    b = np.clip(np.rint(rgb.astype(np.float64) * 255.0), 0, 255).astype(np.uint32)
    return np.ascontiguousarray(b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16) | (np.uint32(255) << 24)).view(np.int32)


def test_a_map_learns_the_teachers_sky_behind_frozen_splats(dev):
    """GT is the scene over a teacher map (0.2 .. 0.8) of the same R; the student starts at 0.5 with every splat rate at 0 (lr_mean keeps
    1e-30: its exponential schedule divides by it), no SSIM, 60 steps at lr 0.01: Adam can move a texel 0.6 and needs at most 0.3, the
    residual oscillation is of order lr.  The loss falls below a quarter of its start; texels no pixel reaches keep their bits."""
    import brush_amd as ba
    sc = _scene()
    cam = util.hip_camera(ba, synth.default_camera_params(W, H))
    ctx = ba.Context(dev)
    try:
        spl = _splats(ba, sc, dev)
        teacher = ba.EnvironmentMap(RES, ctx=ctx)
        teacher.params = _table(seed=21)
        frame, _ = ba.render_splats(spl, cam, (W, H), BLACK, ba.RasterPass.Backward, ctx=ctx)
        gt_rgb = teacher.composite(frame, cam).cpu().numpy()[..., :3]
        assert float((frame[..., 3] < 0.5).float().mean()) > 0.1          # there is sky to learn
        gt = torch.from_numpy(_pack(gt_rgb)).to(dev)
        start = np.full((6, RES, RES, 3), 0.5, np.float32)
        env = ba.EnvironmentMap(RES, lr=0.01, ctx=ctx)
        env.params = start
        cfg = ba.TrainConfig(background_color=BLACK, ssim_weight=0.0, lr_mean=1e-30, lr_mean_end=1e-30, lr_coeffs_dc=0.0, lr_opac=0.0, lr_scale=0.0,
                             lr_rotation=0.0, mean_noise_weight=0.0)
        tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx, envmap=env)
        losses = []
        for _ in range(60):
            _, st = tr.step(ba.SceneBatch(gt, cam, view_id=1), spl)
            ctx.sync()
            losses.append(float(st.loss))
        print("loss %.5f -> %.5f (ratio %.3f, bound 0.25)" % (losses[0], losses[-1], losses[-1] / losses[0]))
        assert losses[-1] < 0.25 * losses[0], losses
        assert np.array_equal(spl.transforms.cpu().numpy(), sc["transforms"]) and np.array_equal(spl.sh_coeffs.cpu().numpy(), sc["sh"])
        h_cam = cam.uniforms((W, H))
        ref_cam = dict(vm=np.array(list(h_cam.vm), np.float32), fx=np.float32(h_cam.fx), fy=np.float32(h_cam.fy), cx=np.float32(h_cam.cx), cy=np.float32(h_cam.cy))
        texel, _ = vr.taps(ref_cam, H, W, RES)
        reached = np.zeros(6 * RES * RES, bool)
        reached[texel.reshape(-1)] = True
        reached = reached.reshape(6, RES, RES)
        got = env.params
        assert (~reached).any() and _same(got[~reached], start[~reached])
        assert np.abs(got[reached] - 0.5).max() > 0.05
    finally:
        ctx.close()
