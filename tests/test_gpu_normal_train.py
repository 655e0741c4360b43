"""bh_train_set_normal / TrainConfig.normal_loss_weight (include/brush_hip_normal_loss.h), test for test after
tests/test_gpu_depth_train.py and on its scenes: nothing attached (or weight 0) changes nothing; a step with the term is the
hand-composed render -> expected depth -> accumulated normals [-> depth loss] -> fused normal consistency -> image loss -> ONE backward
with a depth and a normal term; the row-marked single-GPU step equals the zero-filled hook step bit for bit; a cut frame agrees with a
complete one; past growth_stop_iter the refine column is left alone; the term lowers the value it penalises; what cannot work is
refused before anything runs; normal_loss_from_iter starts the term at that step.  No seed: the noise terms are zero."""
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


def _run(dev, sc, w, h, steps, mode, hook=False, weight=0.5, cfg_kw=None, store=None, depth=False, per_step=None):
    """mode: "plain" (nothing attached), "zero" (the term attached at weight 0), "normal" (the term).  depth: an L1 depth target too."""
    import brush_amd as ba
    from brush_amd import _ffi
    ctx = ba.Context(dev)
    try:
        cam, gt = util.hip_camera(ba, synth.default_camera_params(w, h)), _gt(dev, w, h)
        dmap = _depth_gt(ba, ctx, sc, cam, w, h, dev) if depth else None
        spl = _splats(ba, sc, dev)
        kw = dict(cfg_kw or {})
        kw.setdefault("normal_loss_weight", weight if mode == "normal" else 0.0)
        cfg = ba.TrainConfig(background_color=BG, depth_loss_weight=0.5 if depth else 0.0, **kw)
        tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx)
        if mode == "zero":   # (the trainer detaches at weight 0: attach a zero-weight term behind it)
            zero = _ffi.BhNormalTermConfig(weight=0.0)
            tr.batch_patch = lambda b: ctx.check(ctx.lib.bh_train_set_normal(ctx._h, C.byref(zero)))
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
    assert math.isfinite(plain[0]) and plain[0].tobytes() == zero[0].tobytes(), (plain, zero)
    one = _one_tile()   # ONE 16x16 tile: whole steps repeat bit for bit, so the splats can be compared too
    lp, a = _run(dev, one, 16, 16, 3, "plain")
    lp2, a2 = _run(dev, one, 16, 16, 3, "plain")
    lz, b = _run(dev, one, 16, 16, 3, "zero")
    ln, d = _run(dev, one, 16, 16, 3, "normal")
    assert [v.tobytes() for v in lp] == [v.tobytes() for v in lp2] == [v.tobytes() for v in lz]
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(a2[k])) and torch.equal(_bits(a[k]), _bits(b[k])), k
    # ... and a weight > 0 does change something (the comparison above is not vacuous)
    assert ln[0] > lp[0] and not torch.equal(_bits(a["transforms"]), _bits(d["transforms"]))


@pytest.mark.parametrize("with_depth", [False, True], ids=["no-depth-target", "l1-depth-target"])
def test_step_equals_the_hand_composed_path(dev, with_depth):
    import brush_amd as ba
    sc = _scene()
    n, c = sc["transforms"].shape[0], sc["sh"].shape[1]
    cam, gt = util.hip_camera(ba, synth.default_camera_params(W, H)), _gt(dev)
    wn, wd = 0.4, 0.6
    cfg = ba.TrainConfig(exact_lists=True, background_color=BG, normal_loss_weight=wn, depth_loss_weight=wd if with_depth else 0.0)
    ctx = ba.Context(dev)
    try:
        dgt = _depth_gt(ba, ctx, sc, cam, W, H, dev) if with_depth else None
        # by hand on the untouched splats
        spl0 = _splats(ba, sc, dev)
        node = ba.render_splats_diff(spl0, cam, (W, H), BG, ctx=ctx)
        e = node.depth("expected")
        nmap = node.normal("accumulated")
        x = node.img.clone()
        dl, v_depth = (None, None)
        if with_depth:
            dl, v_depth = ba.depth_loss_value_and_grad(e, dgt, "l1", wd, ctx=ctx)   # the shared expected-depth map, then the accumulate
        nl, v_normal, v_depth = ba.normal_consistency_value_and_grad(nmap, e, x, cam, wn, v_depth=v_depth, ctx=ctx)
        l_img, v = ba.image_loss_value_and_grad(x, gt, l1_weight=1.0 - cfg.ssim_weight, ssim_weight=-cfg.ssim_weight, ctx=ctx)
        want = node.backward(v, v_depth=v_depth, depth_mode="expected", v_normal=v_normal, normal_mode="accumulated")
        ctx.sync()
        nl = nl.cpu().numpy()
        assert nl[0] > 0 and nl[1] > 0.2 * W * H and float(v_normal.abs().max()) > 0 and float(v_depth.abs().max()) > 0
        want_loss = np.float32(l_img.cpu().numpy()[0])
        if with_depth:
            want_loss = np.float32(want_loss + np.float32(dl.cpu().numpy()[0]))
        want_loss = np.float32(want_loss + np.float32(nl[0]))   # (image) + depth + normal, in f32, in this order
        want = {k: want[k].cpu().numpy() for k in ("v_transforms", "v_sh_coeffs", "v_raw_opacities")}
        only_colour = node.backward(v)["v_transforms"].cpu().numpy()
        assert np.abs(want["v_transforms"][:, 3:7] - only_colour[:, 3:7]).max() > 1e-3 * np.abs(only_colour[:, 3:7]).max()   # the term reaches the quaternions
        # the step
        spl = _splats(ba, sc, dev)
        tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx)
        store = []
        _capture(tr, store)
        _, st = tr.step(ba.SceneBatch(gt, cam, view_id=2, depth=dgt), spl)
        ctx.sync()
        assert np.float32(st.loss).tobytes() == want_loss.tobytes(), (st.loss, want_loss, nl)
        assert len(store) == 1
        _close(_blocks(store[0], n, c), want, GRAD_TOL, "step vs hand-composed (depth target %s):" % with_depth)
    finally:
        ctx.close()


@pytest.mark.parametrize("with_depth", [False, True], ids=["no-depth-target", "l1-depth-target"])
def test_row_marked_step_equals_the_zero_filled_step(dev, with_depth):
    """Without a hook the step zero-fills nothing and K18 marks the rows it writes; with one the whole span is cleared.  The normal
    term's Vn must land on marked, written rows, behind depth's v_z: three steps either way leave the same bits."""
    one = _one_tile()
    n, c = one["transforms"].shape[0], one["sh"].shape[1]
    with_term, without = [], []
    lm, a = _run(dev, one, 16, 16, 3, "normal", depth=with_depth)
    lh, b = _run(dev, one, 16, 16, 3, "normal", hook=True, store=with_term, depth=with_depth)
    _run(dev, one, 16, 16, 1, "plain", hook=True, store=without, depth=with_depth)
    gn, gp = _blocks(with_term[0], n, c)["v_transforms"], _blocks(without[0], n, c)["v_transforms"]
    turned = np.abs(gn[:, 3:7] - gp[:, 3:7]).max(axis=1) > 0
    print("splats whose quaternion gradient the normal term changed: %d of %d" % (int(turned.sum()), n))
    assert turned.any()
    assert [v.tobytes() for v in lm] == [v.tobytes() for v in lh]
    for k in a:
        x, y = a[k], b[k]
        if k == "m2_sh":
            # the row-marked step's update keeps its "dormant" marks in the SIGN of a zero m2_sh (optim.hip; -0.0 where every moment
            # of the splat is zero), the zero-filled step keeps none: the sign of a zero is not part of the state
            assert bool((x[x == 0] == 0).all()) and bool((torch.signbit(y) == 0).all())
            x = torch.where(x == 0, torch.zeros_like(x), x)
        assert torch.equal(_bits(x), _bits(y)), k


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
            tr = ba.SplatTrainer(ba.TrainConfig(exact_lists=exact, background_color=BG, normal_loss_weight=0.5, **FROZEN), median_scene_scale=3.0, ctx=ctx)
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


def test_past_growth_stop_iter_the_refine_column_is_left_alone(dev):
    sc = _scene()
    n, c = sc["transforms"].shape[0], sc["sh"].shape[1]
    kw = dict(growth_stop_iter=2, exact_lists=True, **FROZEN)   # step 1 computes the refine weight, step 2 is past the threshold
    store = []
    _run(dev, sc, W, H, 2, "normal", hook=True, cfg_kw=kw, store=store)
    _close(_blocks(store[1], n, c), _blocks(store[0], n, c), CUT_TOL, "past growth_stop_iter vs before:")
    # the row-marked path: the marks the normal term may set are signs of zeros, so the norm after step 2 is the norm after step 1 OF
    # THE SAME RUN, bit for bit (K17 sums the refine weight with float atomics across tiles: two runs agree only to their order)
    import brush_amd as ba
    norms = {}
    for mode in ("normal", "plain"):
        ctx = ba.Context(dev)
        try:
            cam, gt = util.hip_camera(ba, synth.default_camera_params(W, H)), _gt(dev)
            spl = _splats(ba, sc, dev)
            tr = ba.SplatTrainer(ba.TrainConfig(background_color=BG, normal_loss_weight=0.5 if mode == "normal" else 0.0, **kw), median_scene_scale=3.0, ctx=ctx)
            after = []
            for _ in range(2):
                tr.step(ba.SceneBatch(gt, cam, view_id=2), spl)
                ctx.sync()
                after.append(tr.state["refine_weight_norm"].clone())
            assert float(after[0].max()) > 0 and torch.equal(_bits(after[0]), _bits(after[1])), mode
            norms[mode] = after[1].cpu().numpy().astype(np.float64)
        finally:
            ctx.close()
    # ... and it is the colour term's alone: with and without the term it agrees to the atomics' order (tests/cpp/test_depth.cpp: 1e-6)
    assert np.abs(norms["normal"] - norms["plain"]).max() <= 1e-6 * norms["plain"].max()


def test_the_term_lowers_the_normal_consistency_value(dev):
    """A scene whose quaternions are perturbed, trained for 30 steps on the unperturbed scene's image: the value the term penalises
    (the operator at weight 1 on the final frame) ends lower with the term on than in the same run with weight 0."""
    import brush_amd as ba
    cp = synth.default_camera_params(W, H)
    teacher_sc = synth.make_scene(1500, 0x7EA, sh_degree=0, log_scale_range=(math.log(0.05), math.log(0.3)),
                                  tan_half_fov=(math.tan(math.radians(45)), math.tan(math.radians(45))))
    student_sc = dict(teacher_sc, transforms=teacher_sc["transforms"].copy())
    student_sc["transforms"][:, 3:7] += np.random.default_rng(11).uniform(-0.3, 0.3, (1500, 4)).astype(np.float32)
    ends = {}
    ctx = ba.Context(dev)
    try:
        cam = util.hip_camera(ba, cp)
        gt = ba.render_splats(_splats(ba, teacher_sc, dev), cam, (W, H), BG, ctx=ctx)[0].clone()
        ctx.sync()

        def value(spl):
            node = ba.render_splats_diff(spl, cam, (W, H), BG, ctx=ctx)
            loss, _, _ = ba.normal_consistency_value_and_grad(node.normal("accumulated"), node.depth("expected"), node.img, cam, 1.0, ctx=ctx)
            ctx.sync()
            return float(loss.cpu()[0])

        for weight in (1.0, 0.0):
            spl = _splats(ba, student_sc, dev)
            first = value(spl)
            cfg = ba.TrainConfig(background_color=BG, normal_loss_weight=weight, mean_noise_weight=0.0)
            tr = ba.SplatTrainer(cfg, median_scene_scale=3.0, ctx=ctx)
            for s in range(30):
                tr.step(ba.SceneBatch(gt, cam, view_id=1), spl)
            ends[weight] = value(spl)
    finally:
        ctx.close()
    print("normal-consistency value: initial %.5f, after 30 steps with the term %.5f, without %.5f" % (first, ends[1.0], ends[0.0]))
    assert ends[1.0] < first and ends[1.0] < ends[0.0]


@pytest.mark.parametrize("case", ["fisheye", "window", "pose"])
def test_refusals_leave_the_step_unqueued(dev, case):
    import brush_amd as ba
    from brush_amd.host import _ptr
    sc = _scene()
    ctx = ba.Context(dev)
    try:
        cp = synth.default_camera_params(W, H)
        cam, gt = util.hip_camera(ba, cp), _gt(dev)
        bad_cam = cam
        spl = _splats(ba, sc, dev)
        tr = ba.SplatTrainer(ba.TrainConfig(background_color=BG, normal_loss_weight=0.5), median_scene_scale=3.0, ctx=ctx)
        keep = []
        if case == "fisheye":
            kb4 = {k: v for k, v in cp.items() if k not in ("img_w", "img_h")}
            kb4["model"], kb4["dist"] = util.REF_LENSES["kb4"]
            bad_cam = util.hip_camera(ba, kb4)
        elif case == "window":
            def window(b):
                b.camera.tile_row_begin, b.camera.tile_row_end = 0, 2   # two of the frame's three tile rows
            tr.batch_patch = window
        elif case == "pose":
            buf = torch.zeros((12,), dtype=torch.float32, device=dev)
            keep.append(buf)
            ctx.check(ctx.lib.bh_train_set_pose_grad(ctx._h, _ptr(buf)))
        torch.cuda.synchronize()
        with pytest.raises(ba.BrushHipError, match=r"brush_hip error -1: train_step: .*normal term"):
            tr.step(ba.SceneBatch(gt, bad_cam, view_id=2), spl)
        ctx.check(ctx.lib.bh_train_set_pose_grad(ctx._h, None))
        ctx.sync()
        assert tr.step_count == 0
        assert np.array_equal(spl.transforms.cpu().numpy(), sc["transforms"]) and np.array_equal(spl.sh_coeffs.cpu().numpy(), sc["sh"])
        assert np.array_equal(spl.raw_opacities.cpu().numpy(), sc["raw_opac"])
        # the same trainer steps once the obstacle is gone (the term was detached behind the refused step)
        tr.batch_patch = None
        tr.config.normal_loss_weight = 0.0
        _, st = tr.step(ba.SceneBatch(gt, cam, view_id=2), spl)
        ctx.sync()
        assert tr.step_count == 1 and math.isfinite(st.loss)
    finally:
        ctx.close()


def test_normal_loss_from_iter_starts_the_term_at_that_step(dev):
    one = _one_tile()
    plain, late = [], []
    lp, _ = _run(dev, one, 16, 16, 2, "plain", per_step=plain)
    ll, _ = _run(dev, one, 16, 16, 2, "normal", cfg_kw=dict(normal_loss_from_iter=2), per_step=late)
    assert lp[0].tobytes() == ll[0].tobytes()
    for k in plain[0]:
        assert torch.equal(_bits(plain[0][k]), _bits(late[0][k])), k   # step 1 is a plain step, bit for bit
    assert ll[1] > lp[1] and not torch.equal(_bits(plain[1]["transforms"]), _bits(late[1]["transforms"]))   # step 2 carries the term
