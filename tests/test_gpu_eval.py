"""Held-out evaluation on the MI355X: bh_eval_metrics against the composed path (torch quantise + bh_image_loss_forward twice) and
the numpy restatement tests/eval_ref.py, its determinism and rgb8 copy, bh_eval_view against render + metrics, the oracle end to
end, and evals interleaved with training leaving the training untouched, bit for bit."""
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import eval_ref
import util

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (16, 16), (40, 52), (67, 131), (270, 480), (1080, 1920)]


def _random_case(h, w, seed):
    """[H,W,4] f32 in [-0.1, 1.2] with planted exact rounding ties, and a random packed GT."""
    rng = np.random.default_rng(seed)
    img = rng.uniform(-0.1, 1.2, size=(h, w, 4)).astype(np.float32)
    ties = eval_ref.tie_values(np.arange(255))
    m = rng.random((h, w, 3)) < 0.1
    img[..., :3][m] = ties[rng.integers(0, 255, size=int(m.sum()))]
    gt = rng.integers(0, 2 ** 32, size=(h, w), dtype=np.uint64).astype(np.uint32)
    return img, gt


def _gt_tensor(gt, dev):
    return torch.from_numpy(np.ascontiguousarray(gt).view(np.int32)).to(dev)


def _composed_terms(ba, img_t, gt_t):
    """The per-pixel terms as the reference composes them on the device: torch quantise, two image_loss_forward maps."""
    # (a tensor divisor: torch divides by a Python scalar as a multiply by its reciprocal, which is not the reference's divide)
    q = torch.round(img_t[..., :3] * 255.0) / torch.full_like(img_t[..., :3], 255.0)
    l1 = ba.image_loss(q, gt_t, l1_weight=1.0, ssim_weight=0.0)
    ss = ba.image_loss(q, gt_t, l1_weight=0.0, ssim_weight=1.0)
    return (l1 * l1).cpu().numpy(), ss.cpu().numpy()


def _within_ulp(got, want, ulps=1):
    got, want = np.float32(got), np.float32(want)
    return abs(float(got) - float(want)) <= ulps * float(np.spacing(np.abs(want)))


@pytest.mark.parametrize("h,w", SIZES)
def test_metrics_match_the_composed_path_and_the_reference(dev, h, w):
    import brush_amd as ba
    img, gt = _random_case(h, w, seed=h * 7919 + w)
    img_t, gt_t = torch.from_numpy(img).to(dev), _gt_tensor(gt, dev)
    m = ba.eval_metrics(img_t, gt_t).cpu().numpy()
    sq, ss = _composed_terms(ba, img_t, gt_t)
    mse, psnr, ssim = eval_ref.metrics_from_terms(sq, ss)
    assert _within_ulp(m[0], mse), (m[0], mse)
    assert _within_ulp(m[2], ssim), (m[2], ssim)
    p = eval_ref.psnr_f32(m[0])
    assert abs(float(m[1]) - float(p)) <= 1e-6 * abs(float(p)), (m[1], p)
    if h * w <= 270 * 480:   # the CPU oracle's maps (the 1080p case is covered by the device composition above)
        r = eval_ref.eval_metrics(img, gt)
        assert _within_ulp(m[0], r[0]) and _within_ulp(m[2], r[2]), (m, r)


def test_metrics_are_deterministic_and_rgb8_is_exact(dev):
    import brush_amd as ba
    for h, w in ((67, 131), (1080, 1920)):
        img, gt = _random_case(h, w, seed=5)
        img_t, gt_t = torch.from_numpy(img).to(dev), _gt_tensor(gt, dev)
        first, rgb8 = ba.eval_metrics(img_t, gt_t, keep_image=True)
        outs = [ba.eval_metrics(img_t, gt_t) for _ in range(4)]   # queued back to back, each into its own [3]
        for o in outs:
            assert torch.equal(o.view(torch.int32), first.view(torch.int32))
        assert np.array_equal(rgb8.cpu().numpy().view(np.uint32), eval_ref.rgb8(img))


def _scene_and_views(dev, n=3000, sh_degree=1, w=96, h=72, k=3, seed=0x3E):
    import brush_amd as ba
    sc = synth.make_scene(n, seed, sh_degree=sh_degree, log_scale_range=(math.log(0.02), math.log(0.2)))
    cams = []
    for i in range(k):
        cp = synth.default_camera_params(w, h)
        cp["rot_xyzw"] = util.quat_from_axis_angle((0, 1, 0), math.radians(-12 + 12 * i))
        cams.append(cp)
    return sc, cams


def _target_u8(w, h, seed):
    gt = synth.synthetic_gt_packed(w, h, seed=seed)
    return np.stack([(gt >> (8 * c)) & 0xFF for c in range(4)], axis=-1).astype(np.uint8)


@pytest.mark.parametrize("mip", [False, True])
@pytest.mark.parametrize("floor", [False, True])
def test_eval_view_equals_render_plus_metrics(dev, mip, floor):
    import brush_amd as ba
    sc, cams = _scene_and_views(dev)
    w, h = 96, 72
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], render_mip=mip, device=dev)
    if floor:
        spl.with_min_scale(np.full(spl.num_splats(), 0.03, np.float32))
    gt_t = _gt_tensor(synth.synthetic_gt_packed(w, h, seed=3), dev)
    ctx = ba.Context(dev)
    try:
        for cp in cams:
            cam = util.hip_camera(ba, cp)
            s = ba.eval_stats(spl, cam, gt_t, ctx=ctx, keep_image=True)
            img, _ = ba.render_splats(spl, cam, (w, h), (0.0, 0.0, 0.0), ba.RasterPass.Backward, ctx=ctx)
            m, rgb8 = ba.eval_metrics(img, gt_t, ctx=ctx, keep_image=True)
            assert torch.equal(s.metrics.view(torch.int32), m.view(torch.int32))
            assert torch.equal(s.image, rgb8)
            assert 5.0 < s.psnr < 60.0 and -1.0 <= s.ssim <= 1.0
        # n == 0 scores a black image
        empty = ba.Splats(np.zeros((0, 10), np.float32), np.zeros((0, 1, 3), np.float32), np.zeros((0,), np.float32), device=dev)
        s0 = ba.eval_stats(empty, util.hip_camera(ba, cams[0]), gt_t, ctx=ctx)
        black = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
        m0 = ba.eval_metrics(black, gt_t, ctx=ctx)
        assert torch.equal(s0.metrics.view(torch.int32), m0.view(torch.int32))
    finally:
        ctx.close()


def test_run_eval_matches_per_view_eval_stats(dev):
    import brush_amd as ba
    sc, cams = _scene_and_views(dev, k=4)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    views = [(_target_u8(96, 72, 10 + i), util.hip_camera(ba, cp)) for i, cp in enumerate(cams)]
    views.append((lambda: _target_u8(80, 64, 99)[..., :3], util.hip_camera(ba, cams[0])))   # a callable RGB view of another size
    ctx = ba.Context(dev)
    try:
        res = ba.run_eval(spl, views, ctx=ctx, keep_images=True)
        assert tuple(res.per_view.shape) == (len(views), 3) and len(res.images) == len(views)
        psnr, ssim = np.float32(0), np.float32(0)
        for i, (img, cam) in enumerate(views):
            img = img() if callable(img) else img
            up = ba.BatchUploader(img.shape[0] * img.shape[1], 2, ctx)
            gt, _ = up.acquire(up.submit(img, premultiply=True))
            s = ba.eval_stats(spl, cam, gt, ctx=ctx, keep_image=True)
            ctx.sync()
            up.close()
            assert torch.equal(res.per_view[i].view(torch.int32), s.metrics.cpu().view(torch.int32)), i
            assert torch.equal(res.images[i], s.image), i
            psnr, ssim = np.float32(psnr + np.float32(s.psnr)), np.float32(ssim + np.float32(s.ssim))
        assert res.avg_psnr == float(np.float32(psnr / np.float32(len(views))))
        assert res.avg_ssim == float(np.float32(ssim / np.float32(len(views))))
    finally:
        ctx.close()


def test_eval_against_the_oracle_render(dev, oracle_lib):
    import brush_amd as ba
    bo = oracle_lib
    sc, cams = _scene_and_views(dev, n=1500, sh_degree=2)
    w, h = 96, 72
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    gt = synth.synthetic_gt_packed(w, h, seed=4)
    gt_t = _gt_tensor(gt, dev)
    for cp in cams:
        s = ba.eval_stats(spl, util.hip_camera(ba, cp), gt_t)
        ref = bo.Render().forward(util.oracle_camera(bo, cp), sc["transforms"], sc["sh"], sc["raw_opac"], bg=(0.0, 0.0, 0.0), flags=bo.FLAG_BWD_INFO)
        mse, psnr, ssim = eval_ref.eval_metrics(ref.image(), gt)
        assert abs(s.psnr - float(psnr)) < 0.01, (s.psnr, psnr)
        assert abs(s.ssim - float(ssim)) < 1e-4, (s.ssim, ssim)


def test_a_render_scored_against_its_own_8bit_image(dev):
    import brush_amd as ba
    sc, cams = _scene_and_views(dev, sh_degree=0)   # SH 0 colours stay inside [0, 1]: the 8-bit copy loses nothing but rounding
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    w, h = 96, 72
    cam = util.hip_camera(ba, cams[1])
    first = ba.eval_stats(spl, cam, _gt_tensor(synth.synthetic_gt_packed(w, h), dev), keep_image=True)
    again = ba.eval_stats(spl, cam, first.image)
    assert again.psnr > 100.0 and again.ssim > 0.9999, (again.psnr, again.ssim)


@pytest.mark.parametrize("sh_degree", [0, 2])
def test_interleaved_evals_do_not_change_training(dev, sh_degree):
    """The one-tile deterministic set-up of test_gpu_masked_grads.py (16x16, 6000 splats, seed 77, 9 steps) with an eval at another
    camera and a larger size after every step (the arena's slots grow under the training): parameters, moments and refine statistics
    equal a run without evals, bit for bit."""
    import brush_amd as ba
    n, w, h = 6000, 16, 16
    sc = synth.make_scene(n, 0xD0A, sh_degree=sh_degree, log_scale_range=(math.log(0.05), math.log(0.4)),
                          tan_half_fov=(math.tan(math.radians(50)), math.tan(math.radians(50))))
    cams = []
    for i in range(3):
        c = dict(synth.default_camera_params(w, h))
        c["rot_xyzw"] = util.quat_from_axis_angle((0, 1, 0), math.radians(-35 + 35 * i))
        cams.append(c)
    gt = torch.from_numpy(synth.synthetic_gt_packed(w, h).view(np.int32)).to(dev)
    ew, eh = 200, 136
    eval_cam = synth.default_camera_params(ew, eh)
    eval_gt = _gt_tensor(synth.synthetic_gt_packed(ew, eh, seed=11), dev)
    runs = {}
    for key in ("plain", "with_evals"):
        ctx = ba.Context(dev)
        try:
            spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
            tr = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=3.0, ctx=ctx, seed=77)
            scores = []
            for s in range(9):
                tr.step(ba.SceneBatch(gt, util.hip_camera(ba, cams[s % len(cams)])), spl)
                if key == "with_evals":
                    scores.append(ba.eval_stats(spl, util.hip_camera(ba, eval_cam), eval_gt, ctx=ctx).psnr)
            ctx.sync()
            out = {"transforms": spl.transforms.clone(), "sh": spl.sh_coeffs.clone(), "opac": spl.raw_opacities.clone()}
            out.update({k: v.clone() for k, v in tr.state.items()})
            runs[key] = out
            if scores:
                assert all(math.isfinite(p) for p in scores)
        finally:
            ctx.close()
    a, b = runs["plain"], runs["with_evals"]
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_bad_arguments_are_refused(dev):
    import ctypes as C
    import brush_amd as ba
    from brush_amd import _ffi
    ctx = ba.Context(dev)
    try:
        w, h = 32, 32
        sc, cams = _scene_and_views(dev, n=200, w=w, h=h, k=1)
        spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
        gt = _gt_tensor(synth.synthetic_gt_packed(w, h), dev)
        metrics = torch.empty(3, dtype=torch.float32, device=dev)
        lib = ctx.lib

        def view(cam, flags, gt_ptr):
            return lib.bh_eval_view(ctx._h, C.byref(cam), spl.num_splats(), spl.sh_degree(), spl.transforms.data_ptr(), spl.sh_coeffs.data_ptr(),
                                    spl.raw_opacities.data_ptr(), None, flags, gt_ptr, metrics.data_ptr(), None)
        cam = util.hip_camera(ba, cams[0]).uniforms((w, h))
        assert view(cam, 0, gt.data_ptr()) == 0
        strip = util.hip_camera(ba, cams[0]).uniforms((w, h), tile_rows=(0, 1))
        assert view(strip, 0, gt.data_ptr()) == -1   # BH_ERR_INVALID_ARG: a view is scored whole
        for flags in (_ffi.FLAG_BWD_INFO, _ffi.FLAG_SLICED_LISTS, 64):
            assert view(cam, flags, gt.data_ptr()) == -1, flags
        assert view(cam, 0, None) == -1
        img = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
        assert lib.bh_eval_metrics(ctx._h, img.data_ptr(), None, h, w, metrics.data_ptr(), None) == -1
        assert lib.bh_eval_metrics(ctx._h, img.data_ptr(), gt.data_ptr(), 0, w, metrics.data_ptr(), None) == -1
        assert lib.bh_eval_metrics(ctx._h, img.data_ptr() + 4, gt.data_ptr(), h, w - 1, metrics.data_ptr(), None) == -1   # not 16-byte aligned
        assert lib.bh_eval_metrics(ctx._h, img.data_ptr(), gt.data_ptr(), h, w, None, None) == -1
        with pytest.raises(ba.BrushHipError):
            ba.eval_stats(spl, util.hip_camera(ba, cams[0]).uniforms((w, h), tile_rows=(0, 1)), gt, ctx=ctx)
        ctx.sync()
    finally:
        ctx.close()
