"""bh_train_set_intrinsics_grad (include/brush_hip_intrinsics.h): the attached buffer changes nothing else about the
step, holds what the hand-composed forward / loss / intrinsics backward gives, is left alone once detached, the step refuses an
environment map and the normal term beside it, and IntrinsicsOptimizer recovers a perturbed lens.  Noise terms are zero (no seed),
as the parity suite sets them."""
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import intrinsics_ref
import util

TOL = 1e-4
gpu = pytest.mark.gpu


def _setup(n=6000, w=16, h=16, seed=0xD0A):
    """ONE 16x16 tile (tests/test_gpu_pose_train.py): every splat has at most one (splat, tile) pair, so whole steps repeat bit for bit."""
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
        buf = torch.full((4,), -7.0, device=dev)
        seen = []
        for s in range(steps):
            if mode == "attached" or (mode == "detached" and s == 0):
                ctx.check(ctx.lib.bh_train_set_intrinsics_grad(ctx._h, _ptr(buf)))
            if mode == "detached" and s == 1:
                ctx.check(ctx.lib.bh_train_set_intrinsics_grad(ctx._h, None))
                buf.fill_(-7.0)
            tr.step(ba.SceneBatch(_gt(dev), util.hip_camera(ba, cp)), spl)
            seen.append(buf.clone())
        ctx.sync()
        out = {"transforms": spl.transforms.clone(), "sh": spl.sh_coeffs.clone(), "opac": spl.raw_opacities.clone()}
        out.update({k: v.clone() for k, v in tr.state.items()})
        return out, seen
    finally:
        ctx.close()


@gpu
def test_attached_buffer_changes_nothing_else_and_detaching_stops_the_writes(dev):
    plain, untouched = _steps(dev, None)
    on, seen = _steps(dev, "attached")
    for k in plain:
        assert torch.equal(plain[k].view(torch.int32), on[k].view(torch.int32)), k
    assert all(torch.equal(b, torch.full((4,), -7.0, device=dev)) for b in untouched)
    assert all(torch.isfinite(b).all() and float(b.abs().max()) > 0 and not (b == -7.0).any() for b in seen)
    assert not torch.equal(seen[0], seen[1])   # each step's own gradient
    off, seen = _steps(dev, "detached")
    for k in plain:
        assert torch.equal(plain[k].view(torch.int32), off[k].view(torch.int32)), k
    assert not (seen[0] == -7.0).any()
    assert torch.equal(seen[1], torch.full((4,), -7.0, device=dev)) and torch.equal(seen[2], seen[1])   # the sentinel stays


@gpu
def test_buffer_is_the_hand_composed_intrinsics_gradient(dev):
    import brush_amd as ba
    from brush_amd.host import _ptr
    sc, cp = _setup(n=2000)   # (what the float64 reference below walks through in about two seconds)
    w = h = 16
    cam = util.hip_camera(ba, cp)
    ctx = ba.Context(dev)
    try:
        cfg = ba.TrainConfig()
        spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
        # by hand, on the untouched inputs: forward, the step's loss and its gradient, the intrinsics backward
        node = ba.render_splats_diff(spl, cam, (w, h), cfg.background_color, ctx=ctx)
        _, v_out = ba.image_loss_value_and_grad(node.img, _gt(dev), l1_weight=1.0 - cfg.ssim_weight, ssim_weight=-cfg.ssim_weight, ctx=ctx)
        want = node.backward(v_out, intrinsics=True)["v_intrinsics"].cpu().numpy().astype(np.float64)
        tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx)
        buf = torch.full((4,), float("nan"), device=dev)
        ctx.check(ctx.lib.bh_train_set_intrinsics_grad(ctx._h, _ptr(buf)))
        tr.step(ba.SceneBatch(_gt(dev), cam), spl)
        ctx.check(ctx.lib.bh_train_set_intrinsics_grad(ctx._h, None))
        got = buf.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all() and np.abs(want).max() > 0
        # the L1 masses S_k: the float64 reference's per-splat contributions for the same v_output (tests/intrinsics_ref.py)
        with torch.enable_grad():
            ref = intrinsics_ref.intrinsics_gradients(sc, cp, w, h, v_out.cpu().numpy(), bg=tuple(cfg.background_color))
        mass = ref["S"]
        assert (mass > 0).all()
        ratio = np.abs(got - want) / mass
        print("train step vs hand-composed: max |delta_k| / S_k = %.3e" % ratio.max())
        assert (np.abs(got - want) <= TOL * mass).all(), ratio
    finally:
        ctx.close()


@gpu
@pytest.mark.parametrize("case", ["envmap", "normal"])
def test_step_refuses_what_the_pass_does_not_carry(dev, case):
    """BH_ERR_STATE (-4) from the library itself, with the buffer attached behind the trainer's back; the same step runs once the
    buffer is detached."""
    import brush_amd as ba
    from brush_amd.host import _ptr
    sc, cp = _setup(n=500)
    ctx = ba.Context(dev)
    try:
        spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
        env = ba.EnvironmentMap(8, lr=0.0, ctx=ctx) if case == "envmap" else None
        cfg = ba.TrainConfig(background_color=(0.0, 0.0, 0.0)) if case == "envmap" else ba.TrainConfig(normal_loss_weight=0.05, normal_loss_from_iter=0)
        tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx, envmap=env)
        buf = torch.full((4,), -7.0, device=dev)
        batch = ba.SceneBatch(_gt(dev), util.hip_camera(ba, cp), view_id=2)
        ctx.check(ctx.lib.bh_train_set_intrinsics_grad(ctx._h, _ptr(buf)))
        with pytest.raises(ba.BrushHipError, match=r"error -4: train_step: .* intrinsics-gradient buffer"):
            tr.step(batch, spl)
        ctx.sync()
        assert torch.equal(buf, torch.full((4,), -7.0, device=dev)) and tr.step_count == 0
        ctx.check(ctx.lib.bh_train_set_intrinsics_grad(ctx._h, None))
        tr.step(batch, spl)
        assert tr.step_count == 1
    finally:
        ctx.close()


@gpu
def test_trainer_with_both_optimizers_reads_both_gradients_back(dev):
    """SplatTrainer(pose_optimizer=, intrinsics_optimizer=): every step moves the view's twist and the sensor's four, the view stays
    one table, and a run on a context with its own stream sees the gradients a run on torch's stream sees (one 16x16 tile: whole
    steps repeat bit for bit)."""
    import brush_amd as ba

    def run(own):
        sc, cp = _setup()
        ctx = ba.Context(dev, use_torch_stream=not own)
        try:
            spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
            torch.cuda.synchronize()
            po, io = ba.PoseOptimizer(lr_rotation=1e-4, lr_translation=1e-3), ba.IntrinsicsOptimizer()
            tr = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=3.0, ctx=ctx, pose_optimizer=po, intrinsics_optimizer=io)
            gt = _gt(dev)
            torch.cuda.synchronize()
            seen = []
            for _ in range(4):
                tr.step(ba.SceneBatch(gt, util.hip_camera(ba, cp), view_id=3), spl)
                seen.append((po.twist(3), io.params(3), io.sensors[0]["m1"].copy(), ctx.view_table_count()))
            ctx.sync()
            return seen
        finally:
            ctx.close()

    a, b = run(False), run(True)
    assert a[-1][3] == a[1][3] <= 1
    for (ta, pa, ma, _), (tb, pb, mb, _) in zip(a, b):
        assert np.abs(ma).min() > 0 and np.abs(ta).min() > 0
        assert np.array_equal(ta, tb) and np.array_equal(pa, pb) and np.array_equal(ma, mb), (pa, pb)
    assert not np.array_equal(a[0][1], a[1][1])


# ---- recovery -----------------------------------------------------------------------------------------------------------------
# Eight orbit views of 1500 fixed splats at 64x64, the lens scaled by 1.03 in focal length and its principal point shifted by 1.5 px
# in x and y; 150 IntrinsicsOptimizer steps cycling the views on the mean squared error against the true lens's frames.  The learning
# rates: log f has 0.03 to travel and Adam moves at most lr per step, so the default lr_focal = 1e-3 gets there in 150 steps with
# room; the centre has 1.5 / 64 = 0.023 to travel, out of reach of the default 1e-4 in 150 steps, hence 5e-4.
RECOVERY = dict(n=1500, size=64, views=8, seed=0xC9, focal_scale=1.03, shift_px=1.5, iters=150, lr_focal=1e-3, lr_center=5e-4, radius=4.5)


def _recovery_scene():
    """(scene, [camera dicts], student camera dicts): a blob of splats around the origin and cameras on a circle looking at it."""
    r = RECOVERY
    w = h = r["size"]
    cp0 = synth.default_camera_params(w, h)
    sc = synth.make_scene(r["n"], r["seed"], sh_degree=0, log_scale_range=(math.log(0.05), math.log(0.25)), z_range=(3.0, 6.0),
                          tan_half_fov=(0.35, 0.35))
    sc["transforms"][:, 2] -= 4.5   # the frustum's splats, moved around the origin
    cams = []
    for i in range(r["views"]):
        a = 2.0 * math.pi * i / r["views"]
        pos = np.array([r["radius"] * math.sin(a), 0.6 * math.sin(2.0 * a + 0.3), -r["radius"] * math.cos(a)])
        f = -pos / np.linalg.norm(pos)
        right = np.cross(np.array([0.0, 1.0, 0.0]), f)
        right /= np.linalg.norm(right)
        c2w = np.stack([right, np.cross(f, right), f], axis=1)
        qw = 0.5 * math.sqrt(max(1.0 + c2w[0, 0] + c2w[1, 1] + c2w[2, 2], 1e-12))
        if qw > 1e-3:
            q = (float((c2w[2, 1] - c2w[1, 2]) / (4 * qw)), float((c2w[0, 2] - c2w[2, 0]) / (4 * qw)), float((c2w[1, 0] - c2w[0, 1]) / (4 * qw)), float(qw))
        else:   # the half turn about y (the view opposite the first)
            q = (0.0, 1.0, 0.0, 0.0)
        cams.append(dict(pos=tuple(float(v) for v in pos), rot_xyzw=q, fov_x=cp0["fov_x"], fov_y=cp0["fov_y"], center_uv=(0.5, 0.5)))
    return sc, cams


def _recovery_loop(ba, grad_of):
    """The loop both the device test and the float64 run take: grad_of(view index, BhCamera) -> v_intrinsics [4] of the mean squared
    error against that view's target.  Returns (initial, final) = (|log(f / f*)| of the worse axis, principal-point error in px)."""
    r = RECOVERY
    w = h = r["size"]
    _, cams = _recovery_scene()
    true = [util.hip_camera(ba, c) for c in cams]
    u0 = true[0].uniforms((w, h))
    students = [c.with_intrinsics(r["focal_scale"] * u0.fx, r["focal_scale"] * u0.fy, u0.cx + r["shift_px"], u0.cy + r["shift_px"], (w, h)) for c in true]
    io = ba.IntrinsicsOptimizer(lr_focal=r["lr_focal"], lr_center=r["lr_center"])

    def errs():
        u = io.camera(1, students[0], (w, h))
        return (max(abs(math.log(u.fx / u0.fx)), abs(math.log(u.fy / u0.fy))), math.hypot(u.cx - u0.cx, u.cy - u0.cy))

    e0 = errs()
    for it in range(r["iters"]):
        v = it % r["views"]
        cam = io.camera(v + 1, students[v], (w, h))
        io.update(v + 1, cam, grad_of(v, cam))
    return e0, errs()


@gpu
def test_intrinsics_optimizer_recovers_a_perturbed_lens(dev):
    """Frozen splats, the targets rendered with the true lens, the student's focal lengths 3 % long and its principal point 1.5 px
    off in x and y; IntrinsicsOptimizer alone through RenderNode.backward(intrinsics=True), one sensor for the eight views.  Both
    errors end below a third of their initial value.

    The same loop in float64 on the CPU through tests/intrinsics_ref.py (recovery_reference() below, four minutes) ends at
    |log(f / f*)| = 1.776e-05 and a principal-point error of 0.00139 px, from 2.956e-02 and 2.121 px: far below a sixth of both, so
    the scene, the seed and the step count were kept as first chosen."""
    import brush_amd as ba
    r = RECOVERY
    w = h = r["size"]
    sc, cams = _recovery_scene()
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    ctx = ba.Context(dev)
    try:
        smooth = ba.RasterPass.BackwardSmoothCutoff
        targets = [ba.render_splats_diff(spl, util.hip_camera(ba, c), (w, h), pass_=smooth, ctx=ctx).img.clone() for c in cams]
        assert all(float(t[..., 3].mean()) > 0.2 for t in targets)   # every view sees the blob

        def grad_of(v, cam):
            ctx.check(ctx.lib.bh_set_view_id(ctx._h, v + 1))
            node = ba.render_splats_diff(spl, cam, (w, h), pass_=smooth, ctx=ctx)
            g = node.backward((node.img - targets[v]) * (2.0 / (h * w * 4)), intrinsics=True)
            return g["v_intrinsics"].cpu().numpy().astype(np.float64)

        e0, e1 = _recovery_loop(ba, grad_of)
        print("|log f/f*| %.4e -> %.4e, principal point %.4f -> %.4f px" % (e0[0], e1[0], e0[1], e1[1]))
        assert e1[0] < e0[0] / 3.0 and e1[1] < e0[1] / 3.0, (e0, e1)
    finally:
        ctx.close()


def recovery_reference():
    """The recovery loop in float64 on the CPU (tests/intrinsics_ref.py): what the docstring above records.  Not a test: minutes."""
    import brush_amd as ba
    r = RECOVERY
    w = h = r["size"]
    sc, cams = _recovery_scene()
    tr, sh, op = [torch.tensor(np.asarray(sc[k], np.float64)) for k in ("transforms", "sh", "raw_opac")]
    with torch.no_grad():
        targets = [intrinsics_ref.render(tr, sh, op, c, w, h, smooth=True)["img"] for c in cams]

    def grad_of(v, cam):
        k = torch.tensor([cam.fx, cam.fy, cam.cx, cam.cy], dtype=torch.float64, requires_grad=True)
        with torch.enable_grad():
            img = intrinsics_ref.render(tr, sh, op, cams[v], w, h, smooth=True, k=k)["img"]
            ((img - targets[v]) ** 2).mean().backward()
        return k.grad.numpy()

    return _recovery_loop(ba, grad_of)
