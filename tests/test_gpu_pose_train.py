"""bh_train_set_pose_grad (include/brush_hip_pose.h): the attached buffer changes nothing else about the step, holds
what the hand-composed forward / loss / pose backward gives, and is left alone once detached.  Noise terms are zero (no seed), as
the parity suite sets them."""
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import pose_ref
import util

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _setup(n=6000, w=16, h=16, seed=0xD0A):
    """ONE 16x16 tile (tests/test_gpu_masked_grads.py): every splat has at most one (splat, tile) pair, so whole steps repeat bit for bit."""
    sc = synth.make_scene(n, seed, sh_degree=1, log_scale_range=(math.log(0.05), math.log(0.4)),
                          tan_half_fov=(math.tan(math.radians(50)), math.tan(math.radians(50))))
    return sc, synth.default_camera_params(w, h)


def _gt(dev, w=16, h=16):
    return torch.from_numpy(np.ascontiguousarray(synth.synthetic_gt_packed(w, h)).view(np.int32)).to(dev)


def _steps(dev, mode, steps=3):
    import brush_amd as ba
    from brush_amd.host import _ptr
    sc, cp = _setup()
    ctx = ba.Context(dev)
    try:
        spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
        tr = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=3.0, ctx=ctx)
        buf = torch.full((12,), -7.0, device=dev)
        seen = []
        for s in range(steps):
            if mode == "attached" or (mode == "detached" and s == 0):
                ctx.check(ctx.lib.bh_train_set_pose_grad(ctx._h, _ptr(buf)))
            if mode == "detached" and s == 1:
                ctx.check(ctx.lib.bh_train_set_pose_grad(ctx._h, None))
                buf.fill_(-7.0)
            tr.step(ba.SceneBatch(_gt(dev), util.hip_camera(ba, cp)), spl)
            seen.append(buf.clone())
        ctx.sync()
        out = {"transforms": spl.transforms.clone(), "sh": spl.sh_coeffs.clone(), "opac": spl.raw_opacities.clone()}
        out.update({k: v.clone() for k, v in tr.state.items()})
        return out, seen
    finally:
        ctx.close()


def test_attached_buffer_changes_nothing_else_and_detaching_stops_the_writes(dev):
    plain, untouched = _steps(dev, None)
    on, seen = _steps(dev, "attached")
    for k in plain:
        assert torch.equal(plain[k].view(torch.int32), on[k].view(torch.int32)), k
    assert all(torch.equal(b, torch.full((12,), -7.0, device=dev)) for b in untouched)
    assert all(torch.isfinite(b).all() and float(b.abs().max()) > 0 and not (b == -7.0).any() for b in seen)
    assert not torch.equal(seen[0], seen[1])   # each step's own gradient
    off, seen = _steps(dev, "detached")
    for k in plain:
        assert torch.equal(plain[k].view(torch.int32), off[k].view(torch.int32)), k
    assert not (seen[0] == -7.0).any()
    assert torch.equal(seen[1], torch.full((12,), -7.0, device=dev)) and torch.equal(seen[2], seen[1])   # the sentinel stays


def test_buffer_is_the_hand_composed_pose_gradient(dev):
    import brush_amd as ba
    from brush_amd.host import _ptr
    sc, cp = _setup(n=2000)   # (what the float64 reference below walks through in about two seconds)
    w = h = 16
    cam = util.hip_camera(ba, cp)
    ctx = ba.Context(dev)
    try:
        cfg = ba.TrainConfig()
        spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
        # by hand, on the untouched inputs: forward, the step's loss and its gradient, the pose backward
        node = ba.render_splats_diff(spl, cam, (w, h), cfg.background_color, ctx=ctx)
        _, v_out = ba.image_loss_value_and_grad(node.img, _gt(dev), l1_weight=1.0 - cfg.ssim_weight, ssim_weight=-cfg.ssim_weight, ctx=ctx)
        g = node.backward(v_out, pose=True)
        want = g["v_viewmat"].cpu().numpy().astype(np.float64)
        vt = g["v_transforms"].cpu().numpy().astype(np.float64)
        tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx)
        buf = torch.full((12,), float("nan"), device=dev)
        ctx.check(ctx.lib.bh_train_set_pose_grad(ctx._h, _ptr(buf)))
        tr.step(ba.SceneBatch(_gt(dev), cam), spl)
        ctx.check(ctx.lib.bh_train_set_pose_grad(ctx._h, None))
        got = buf.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all() and np.abs(want).max() > 0
        # The L1 masses S_k of all twelve entries: the float64 reference's per-splat contributions for the same v_output
        # (tests/pose_ref.py).  W = I here (the default camera), so the translation entries' S_k is also sum |v_mean| of the
        # hand-composed rows: the two must tell the same scale
        with torch.enable_grad():
            ref = pose_ref.pose_gradients(sc, cp, w, h, v_out.cpu().numpy(), bg=tuple(cfg.background_color))
        mass = ref["S"]
        own = np.abs(vt[:, 0:3]).sum(0)
        assert (mass > 0).all() and (np.abs(mass[9:] - own) <= 1e-2 * own).all(), (mass[9:], own)
        ratio = np.abs(got - want) / mass
        print("train step vs hand-composed: max |delta_k| / S_k = %.3e" % ratio.max())
        assert (np.abs(got - want) <= TOL * mass).all(), ratio
    finally:
        ctx.close()


def test_trainer_with_a_pose_optimizer_keeps_one_view_table(dev):
    import brush_amd as ba
    sc, cp = _setup(n=3000, w=64, h=48, seed=0x3E)
    ctx = ba.Context(dev)
    try:
        spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
        po = ba.PoseOptimizer(lr_rotation=1e-4, lr_translation=1e-3)
        tr = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=3.0, ctx=ctx, pose_optimizer=po)
        gt = _gt(dev, 64, 48)
        counts = []
        for _ in range(6):
            tr.step(ba.SceneBatch(gt, util.hip_camera(ba, cp), view_id=5), spl)
            counts.append(ctx.view_table_count())
        assert np.abs(po.twist(5)).min() > 0 and np.isfinite(po.twist(5)).all()
        assert counts[-1] == counts[1] and counts[-1] <= 1, counts   # the camera moved every step; the view is still one
        with pytest.raises(ValueError):
            tr.step(ba.SceneBatch(gt, util.hip_camera(ba, cp)), spl)   # a moving camera needs a view id
    finally:
        ctx.close()


def test_trainer_with_a_pose_optimizer_on_a_context_with_its_own_stream(dev):
    """Context(use_torch_stream=False): the step runs on the ctx's stream, the readback on torch's.  The optimizer must see each
    step's gradient: the twists of a run on an own-stream context are those of a run on torch's stream, step for step (one 16x16
    tile: whole steps repeat bit for bit)."""
    import brush_amd as ba

    def run(own):
        sc, cp = _setup()
        ctx = ba.Context(dev, use_torch_stream=not own)
        try:
            spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
            torch.cuda.synchronize()
            po = ba.PoseOptimizer(lr_rotation=1e-4, lr_translation=1e-3)
            tr = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=3.0, ctx=ctx, pose_optimizer=po)
            gt = _gt(dev)
            torch.cuda.synchronize()
            twists = []
            for _ in range(4):
                tr.step(ba.SceneBatch(gt, util.hip_camera(ba, cp), view_id=3), spl)
                twists.append((po.twist(3), po.views[3]["m1"].copy()))
            ctx.sync()
            return twists
        finally:
            ctx.close()

    a, b = run(False), run(True)
    for (ta, ma), (tb, mb) in zip(a, b):
        assert np.abs(ma).max() > 0 and np.array_equal(ta, tb) and np.array_equal(ma, mb), (ta, tb)
