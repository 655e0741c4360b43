"""bh_train_set_distortion / TrainConfig.distortion_loss_weight (include/brush_hip_distortion.h), test for test after
tests/test_gpu_normal_train.py and on its scenes: nothing attached (or weight 0 / NaN) changes nothing; a step with the term is the
hand-composed render -> moment map -> distortion loss -> image loss -> ONE backward with a distortion term; the row-marked single-GPU
step equals the zero-filled hook step bit for bit, a splat that receives only v_z included; a cut frame agrees with a complete one;
the term works beside the depth and normal terms; it lowers the mean distortion of the frame; what cannot work is refused before
anything runs; distortion_loss_from_iter starts the term at that step.  No seed: the noise terms are zero."""
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
    """An identity bh_grad_hook that copies what it is given: visible | v_transforms | v_sh | v_raw_opac of the exchange buffer."""
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


def _state(spl, tr):
    out = {"transforms": spl.transforms.clone(), "sh": spl.sh_coeffs.clone(), "opac": spl.raw_opacities.clone()}
    out.update({k: v.clone() for k, v in tr.state.items()})
    return out


NDC = dict(distortion_kind="ndc", distortion_near=0.5, distortion_far=30.0)


def _run(dev, sc, w, h, steps, mode, hook=False, weight=0.5, cfg_kw=None, store=None, depth=False, normal=False, per_step=None, gt=None, bg=BG):
    """mode: "plain" (nothing attached), "zero" / "nan" (the term attached at that weight), "distortion" (the term).  depth: an L1 depth
    target too; normal: the normal-consistency term too."""
    import brush_amd as ba
    from brush_amd import _ffi
    ctx = ba.Context(dev)
    try:
        cam = util.hip_camera(ba, synth.default_camera_params(w, h))
        gt = _gt(dev, w, h) if gt is None else gt
        dmap = _depth_gt(ba, ctx, sc, cam, w, h, dev) if depth else None
        spl = _splats(ba, sc, dev)
        kw = dict(cfg_kw or {})
        kw.setdefault("distortion_loss_weight", weight if mode == "distortion" else 0.0)
        cfg = ba.TrainConfig(background_color=bg, depth_loss_weight=0.5 if depth else 0.0, normal_loss_weight=0.3 if normal else 0.0, **kw)
        tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx)
        if mode in ("zero", "nan"):   # (the trainer detaches at weight 0: attach such a term behind it)
            off = _ffi.BhDistortionTermConfig(weight=0.0 if mode == "zero" else float("nan"), kind=0)
            tr.batch_patch = lambda b: ctx.check(ctx.lib.bh_train_set_distortion(ctx._h, C.byref(off)))
        if hook:
            _capture(tr, store if store is not None else [])
        losses = []
        for _ in range(steps):
            _, st = tr.step(ba.SceneBatch(gt, cam, view_id=2, depth=dmap), spl)
            ctx.sync()
            losses.append(np.float32(st.loss))
            if per_step is not None:
                per_step.append(_state(spl, tr))
        return losses, _state(spl, tr)
    finally:
        ctx.close()


def test_nothing_attached_changes_nothing(dev):
    sc = _scene()
    plain, _ = _run(dev, sc, W, H, 1, "plain")
    zero, _ = _run(dev, sc, W, H, 1, "zero")
    nan, _ = _run(dev, sc, W, H, 1, "nan")
    assert math.isfinite(plain[0]) and plain[0].tobytes() == zero[0].tobytes() == nan[0].tobytes(), (plain, zero, nan)
    one = _one_tile()   # ONE 16x16 tile: whole steps repeat bit for bit, so the splats can be compared too
    lp, a = _run(dev, one, 16, 16, 3, "plain")
    lp2, a2 = _run(dev, one, 16, 16, 3, "plain")
    lz, b = _run(dev, one, 16, 16, 3, "zero")
    ln, b2 = _run(dev, one, 16, 16, 3, "nan")
    ld, d = _run(dev, one, 16, 16, 3, "distortion")
    assert [v.tobytes() for v in lp] == [v.tobytes() for v in lp2] == [v.tobytes() for v in lz] == [v.tobytes() for v in ln]
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(a2[k])) and torch.equal(_bits(a[k]), _bits(b[k])) and torch.equal(_bits(a[k]), _bits(b2[k])), k
    # ... and a weight > 0 does change something (the comparison above is not vacuous)
    assert ld[0] > lp[0] and not torch.equal(_bits(a["transforms"]), _bits(d["transforms"]))


@pytest.mark.parametrize("kind", ["z", "ndc"])
def test_step_equals_the_hand_composed_path(dev, kind):
    import brush_amd as ba
    sc = _scene()
    n, c = sc["transforms"].shape[0], sc["sh"].shape[1]
    cam, gt = util.hip_camera(ba, synth.default_camera_params(W, H)), _gt(dev)
    wx = 0.4
    kw = NDC if kind == "ndc" else {}
    near, far = kw.get("distortion_near", 0.2), kw.get("distortion_far", 1000.0)
    cfg = ba.TrainConfig(exact_lists=True, background_color=BG, distortion_loss_weight=wx, **kw)
    ctx = ba.Context(dev)
    try:
        # by hand on the untouched splats
        spl0 = _splats(ba, sc, dev)
        node = ba.render_splats_diff(spl0, cam, (W, H), BG, ctx=ctx)
        mo = ba.render_distortion(node, kind, near, far, moments=True)
        x = node.img.clone()
        xl = ba.distortion_loss(mo, wx, ctx=ctx)
        l_img, v = ba.image_loss_value_and_grad(x, gt, l1_weight=1.0 - cfg.ssim_weight, ssim_weight=-cfg.ssim_weight, ctx=ctx)
        gain = np.float32(np.float64(np.float32(wx)) / np.float64(W * H))   # the constant cotangent, rounded once
        v_dist = torch.full((H, W), float(gain), dtype=torch.float32, device=dev)
        want = node.backward(v, v_distortion=v_dist, distortion=kind, distortion_near=near, distortion_far=far)
        ctx.sync()
        xl = xl.cpu().numpy()
        assert xl[0] > 0 and xl[1] == W * H
        want_loss = np.float32(np.float32(l_img.cpu().numpy()[0]) + np.float32(xl[0]))   # (image) + distortion, in f32, in this order
        want = {k: want[k].cpu().numpy() for k in ("v_transforms", "v_sh_coeffs", "v_raw_opacities")}
        only_colour = node.backward(v)["v_transforms"].cpu().numpy()
        assert np.abs(want["v_transforms"][:, :3] - only_colour[:, :3]).max() > 1e-3 * np.abs(only_colour[:, :3]).max()   # the term reaches the means
        # the step
        spl = _splats(ba, sc, dev)
        tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx)
        store = []
        _capture(tr, store)
        _, st = tr.step(ba.SceneBatch(gt, cam, view_id=2), spl)
        ctx.sync()
        assert np.float32(st.loss).tobytes() == want_loss.tobytes(), (st.loss, want_loss, xl)
        assert len(store) == 1
        _close(_blocks(store[0], n, c), want, GRAD_TOL, "step vs hand-composed (%s):" % kind)
    finally:
        ctx.close()


@pytest.mark.parametrize("others", ["alone", "depth", "depth-normal"])
@pytest.mark.parametrize("kind", ["z", "ndc"])
def test_row_marked_step_equals_the_zero_filled_step(dev, kind, others):
    """Without a hook the step zero-fills nothing and K18 marks the rows it writes; with one the whole span is cleared.  The term's v_z
    must land on marked, written rows — through the depth term's vector or its own: three steps either way leave the same bits."""
    one = _one_tile()
    n, c = one["transforms"].shape[0], one["sh"].shape[1]
    kw = dict(cfg_kw=NDC if kind == "ndc" else None, depth=others != "alone", normal=others == "depth-normal")
    with_term, without = [], []
    lm, a = _run(dev, one, 16, 16, 3, "distortion", **kw)
    lh, b = _run(dev, one, 16, 16, 3, "distortion", hook=True, store=with_term, **kw)
    _run(dev, one, 16, 16, 1, "plain", hook=True, store=without, depth=kw["depth"], normal=kw["normal"])
    gn, gp = _blocks(with_term[0], n, c)["v_transforms"], _blocks(without[0], n, c)["v_transforms"]
    moved = np.abs(gn[:, :3] - gp[:, :3]).max(axis=1) > 0
    print("splats whose mean gradient the distortion term changed: %d of %d" % (int(moved.sum()), n))
    assert moved.any()
    _assert_same_state(lm, a, lh, b)


def _assert_same_state(lm, a, lh, b):
    assert [v.tobytes() for v in lm] == [v.tobytes() for v in lh]
    for k in a:
        x, y = a[k], b[k]
        if k == "m2_sh":
            # the row-marked step's update keeps its "dormant" marks in the SIGN of a zero m2_sh (optim.hip; -0.0 where every moment
            # of the splat is zero), the zero-filled step keeps none: the sign of a zero is not part of the state
            assert bool((x[x == 0] == 0).all()) and bool((torch.signbit(y) == 0).all())
            x = torch.where(x == 0, torch.zeros_like(x), x)
        assert torch.equal(_bits(x), _bits(y)), k


def _black_scene_with_a_clamped_splat():
    """The one-tile scene painted black on a black background against a black target — the image term's cotangent is exactly zero, so
    K18 writes only the rows the distortion term reaches — plus one splat that covers the tile at alpha0 = 1 with sigma < 1e-3 at every
    pixel: each of its pairs sits at the 0.999 alpha clamp, its ten sums stay zero and it receives v_z alone."""
    sc = _one_tile()
    sc = {k: v.copy() for k, v in sc.items()}
    sc["sh"][:] = 0.0
    sc["sh"][:, 0, :] = -4.0
    z = np.sort(sc["transforms"][:, 2])
    giant = np.zeros((1, 10), np.float32)
    giant[0, :3] = (0.0, 0.0, float(z[8]) + 1e-3)   # behind the eight nearest splats: something contributes in front of it
    giant[0, 3] = 1.0
    giant[0, 7:10] = math.log(400.0)
    sc["transforms"] = np.concatenate([sc["transforms"], giant]).astype(np.float32)
    sc["sh"] = np.concatenate([sc["sh"], sc["sh"][:1]]).astype(np.float32)
    sc["raw_opac"] = np.concatenate([sc["raw_opac"], np.full((1,), 30.0, np.float32)]).astype(np.float32)
    return sc


def test_a_row_that_receives_only_v_z_is_written_whole_and_marked(dev):
    sc = _black_scene_with_a_clamped_splat()
    n, c = sc["transforms"].shape[0], sc["sh"].shape[1]
    gt = torch.zeros((16, 16), dtype=torch.int32, device=dev)
    kw = dict(gt=gt, bg=(0.0, 0.0, 0.0), weight=2.0)
    store = []
    lm, a = _run(dev, sc, 16, 16, 3, "distortion", **kw)
    lh, b = _run(dev, sc, 16, 16, 3, "distortion", hook=True, store=store, **kw)
    g = _blocks(store[0], n, c)
    vt = g["v_transforms"]
    rest = np.abs(vt[:, 3:]).max(axis=1) + np.abs(g["v_sh_coeffs"].reshape(n, -1)).max(axis=1) + np.abs(g["v_raw_opacities"])
    only_vz = (np.abs(vt[:, :3]).max(axis=1) > 0) & (rest == 0)
    print("rows that received v_z alone: %d (the clamped splat: %s); rows written at all: %d" % (int(only_vz.sum()), bool(only_vz[n - 1]),
                                                                                             int((np.abs(vt).max(axis=1) > 0).sum())))
    assert only_vz[n - 1], "the clamped splat did not receive v_z alone"
    _assert_same_state(lm, a, lh, b)


def test_cut_frame_agrees_with_the_exact_frame(dev):
    """The same view twice with per-tile cuts: the second step's loss and gradients agree with the complete-list step of the same
    state (nothing moves: lr 0)."""
    import brush_amd as ba
    w, h = 128, 96
    cp = synth.default_camera_params(w, h)
    sc = synth.make_scene(20000, 0x57, log_scale_range=(math.log(0.03), math.log(0.3)), tan_half_fov=(math.tan(cp["fov_x"] / 2.0), math.tan(cp["fov_y"] / 2.0)))
    n, c = sc["transforms"].shape[0], sc["sh"].shape[1]
    res = {}
    for exact in (True, False):
        ctx = ba.Context(dev)
        try:
            cam, gt = util.hip_camera(ba, cp), _gt(dev, w, h)
            spl = _splats(ba, sc, dev)
            tr = ba.SplatTrainer(ba.TrainConfig(exact_lists=exact, background_color=BG, distortion_loss_weight=0.5, **FROZEN), median_scene_scale=3.0, ctx=ctx)
            store = []
            _capture(tr, store)
            for _ in range(2):
                _, st = tr.step(ba.SceneBatch(gt, cam, view_id=3), spl)
                ctx.sync()
            near, far = ba.last_list_counts(ctx)
            res[exact] = (np.float32(st.loss), _blocks(store[1], n, c), near + far, st.num_intersections)
            assert np.array_equal(spl.transforms.cpu().numpy(), sc["transforms"])
        finally:
            ctx.close()
    print("pairs listed by the second frame: complete %d, cut %d of %d" % (res[True][2], res[False][2], res[False][3]))
    assert res[False][2] < res[False][3]   # the second frame did use cut lists
    assert abs(float(res[True][0]) - float(res[False][0])) <= 1e-6 * max(1.0, abs(float(res[True][0])))
    _close(res[False][1], res[True][1], CUT_TOL, "cut frame vs exact frame:")


def test_step_with_depth_normal_and_distortion_equals_the_hand_composed_path(dev):
    import brush_amd as ba
    sc = _scene()
    n, c = sc["transforms"].shape[0], sc["sh"].shape[1]
    cam, gt = util.hip_camera(ba, synth.default_camera_params(W, H)), _gt(dev)
    wn, wd, wx = 0.4, 0.6, 0.5
    cfg = ba.TrainConfig(exact_lists=True, background_color=BG, normal_loss_weight=wn, depth_loss_weight=wd, distortion_loss_weight=wx)
    ctx = ba.Context(dev)
    try:
        dgt = _depth_gt(ba, ctx, sc, cam, W, H, dev)
        spl0 = _splats(ba, sc, dev)
        node = ba.render_splats_diff(spl0, cam, (W, H), BG, ctx=ctx)
        e = node.depth("expected")
        nmap = node.normal("accumulated")
        mo = ba.render_distortion(node, "z", moments=True)
        x = node.img.clone()
        dl, v_depth = ba.depth_loss_value_and_grad(e, dgt, "l1", wd, ctx=ctx)
        nl, v_normal, v_depth = ba.normal_consistency_value_and_grad(nmap, e, x, cam, wn, v_depth=v_depth, ctx=ctx)
        xl = ba.distortion_loss(mo, wx, ctx=ctx)
        l_img, v = ba.image_loss_value_and_grad(x, gt, l1_weight=1.0 - cfg.ssim_weight, ssim_weight=-cfg.ssim_weight, ctx=ctx)
        gain = np.float32(np.float64(np.float32(wx)) / np.float64(W * H))
        v_dist = torch.full((H, W), float(gain), dtype=torch.float32, device=dev)
        want = node.backward(v, v_depth=v_depth, depth_mode="expected", v_normal=v_normal, normal_mode="accumulated", v_distortion=v_dist)
        ctx.sync()
        want_loss = np.float32(l_img.cpu().numpy()[0])
        for part in (dl, nl, xl):   # (image) + depth + normal + distortion, in f32, in this order
            want_loss = np.float32(want_loss + np.float32(part.cpu().numpy()[0]))
        want = {k: want[k].cpu().numpy() for k in ("v_transforms", "v_sh_coeffs", "v_raw_opacities")}
        spl = _splats(ba, sc, dev)
        tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx)
        store = []
        _capture(tr, store)
        _, st = tr.step(ba.SceneBatch(gt, cam, view_id=2, depth=dgt), spl)
        ctx.sync()
        assert np.float32(st.loss).tobytes() == want_loss.tobytes(), (st.loss, want_loss)
        _close(_blocks(store[0], n, c), want, GRAD_TOL, "step with three terms vs hand-composed:")
    finally:
        ctx.close()


def test_the_term_lowers_the_mean_distortion(dev):
    """30 steps with frozen colours on the scene's own image (the image term starts at its minimum): the mean distortion of the frame
    falls."""
    import brush_amd as ba
    cp = synth.default_camera_params(W, H)
    sc = synth.make_scene(1500, 0x7EA, sh_degree=0, log_scale_range=(math.log(0.05), math.log(0.3)),
                          tan_half_fov=(math.tan(math.radians(45)), math.tan(math.radians(45))))
    ctx = ba.Context(dev)
    try:
        cam = util.hip_camera(ba, cp)
        gt = ba.render_splats(_splats(ba, sc, dev), cam, (W, H), BG, ctx=ctx)[0].clone()
        ctx.sync()

        def value(spl):
            node = ba.render_splats_diff(spl, cam, (W, H), BG, ctx=ctx)
            loss = ba.distortion_loss(node.distortion("z"), 1.0, ctx=ctx)
            ctx.sync()
            return float(loss.cpu()[0])

        spl = _splats(ba, sc, dev)
        first = value(spl)
        cfg = ba.TrainConfig(background_color=BG, distortion_loss_weight=1.0, mean_noise_weight=0.0, lr_coeffs_dc=0.0)
        tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx)
        for s in range(30):
            tr.step(ba.SceneBatch(gt, cam, view_id=1), spl)
        last = value(spl)
    finally:
        ctx.close()
    print("mean distortion: initial %.5f, after 30 steps with the term %.5f" % (first, last))
    assert first > 0 and last < first


@pytest.mark.parametrize("case", ["window", "pose"])
def test_refusals_leave_the_step_unqueued(dev, case):
    import brush_amd as ba
    from brush_amd.host import _ptr
    sc = _scene()
    ctx = ba.Context(dev)
    try:
        cp = synth.default_camera_params(W, H)
        cam, gt = util.hip_camera(ba, cp), _gt(dev)
        spl = _splats(ba, sc, dev)
        tr = ba.SplatTrainer(ba.TrainConfig(background_color=BG, distortion_loss_weight=0.5), median_scene_scale=3.0, ctx=ctx)
        keep = []
        if case == "window":
            def window(b):
                b.camera.tile_row_begin, b.camera.tile_row_end = 0, 2   # two of the frame's three tile rows
            tr.batch_patch = window
        elif case == "pose":
            buf = torch.zeros((12,), dtype=torch.float32, device=dev)
            keep.append(buf)
            ctx.check(ctx.lib.bh_train_set_pose_grad(ctx._h, _ptr(buf)))
        torch.cuda.synchronize()
        with pytest.raises(ba.BrushHipError, match=r"brush_hip error -1: train_step: .*distortion term"):
            tr.step(ba.SceneBatch(gt, cam, view_id=2), spl)
        ctx.check(ctx.lib.bh_train_set_pose_grad(ctx._h, None))
        ctx.sync()
        assert tr.step_count == 0
        assert np.array_equal(spl.transforms.cpu().numpy(), sc["transforms"]) and np.array_equal(spl.sh_coeffs.cpu().numpy(), sc["sh"])
        assert np.array_equal(spl.raw_opacities.cpu().numpy(), sc["raw_opac"])
        # the same trainer steps once the obstacle is gone (the term was detached behind the refused step)
        tr.batch_patch = None
        tr.config.distortion_loss_weight = 0.0
        _, st = tr.step(ba.SceneBatch(gt, cam, view_id=2), spl)
        ctx.sync()
        assert tr.step_count == 1 and math.isfinite(st.loss)
        # a fisheye camera is no obstacle: the per-splat depth is z for every lens model
        kb4 = {k: v for k, v in cp.items() if k not in ("img_w", "img_h")}
        kb4["model"], kb4["dist"] = util.REF_LENSES["kb4"]
        tr.config.distortion_loss_weight = 0.5
        _, st = tr.step(ba.SceneBatch(gt, util.hip_camera(ba, kb4), view_id=3), spl)
        ctx.sync()
        assert tr.step_count == 2 and math.isfinite(st.loss)
    finally:
        ctx.close()


def test_distortion_loss_from_iter_starts_the_term_at_that_step(dev):
    one = _one_tile()
    plain, late = [], []
    lp, _ = _run(dev, one, 16, 16, 2, "plain", per_step=plain)
    ll, _ = _run(dev, one, 16, 16, 2, "distortion", cfg_kw=dict(distortion_loss_from_iter=2), per_step=late)
    assert lp[0].tobytes() == ll[0].tobytes()
    for k in plain[0]:
        assert torch.equal(_bits(plain[0][k]), _bits(late[0][k])), k   # step 1 is a plain step, bit for bit
    assert ll[1] > lp[1] and not torch.equal(_bits(plain[1]["transforms"]), _bits(late[1]["transforms"]))   # step 2 carries the term
