"""What the train step promises about its attached terms, whatever its code looks like ("The step's phases"): for every
term the FIRST refusal a step meets and its whole text, for a tile-row window and for a pose buffer, including the combinations whose
winner depends on the order of the checks; a refused step leaves the trainer, the splats and the ctx as they were; the terms are ctx
state that raw bh_train_step calls keep applying until they are detached, and that a SplatTrainer detaches behind its own step even
when the step raises.  At the smallest shape where a frame can be partial: 32 x 32 pixels (2 x 2 tiles), 64 splats, SH degree 0.
(The LPIPS term's refusal is tests/test_gpu_lpips.py's: a model costs seconds to build.)"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import util

pytestmark = pytest.mark.gpu
BG = (0.1, 0.2, 0.3)
W, H, N = 32, 32, 64
FROZEN = dict(lr_mean=1e-30, lr_mean_end=1e-30, lr_coeffs_dc=0.0, lr_opac=0.0, lr_scale=0.0, lr_rotation=0.0)   # steps that move nothing

PARTIAL = "train_step: the %s needs the whole frame on this rank (no tile-row partition)"
POSE = "train_step: %s and a pose-gradient buffer cannot be attached together (the pose pass does not carry the %s's gradient)"
# (id, term, obstacle, twist, the text bh_last_error holds): the texts as the step had them before it was cut into phases, letter for letter
CASES = [
    ("exposure-window", "exposure", "window", None, PARTIAL % "exposure term"),
    ("bilagrid-window", "bilagrid", "window", None, PARTIAL % "bilateral-grid term"),
    ("depth-window", "depth", "window", None, PARTIAL % "depth term"),
    ("depth-pose", "depth", "pose", None, POSE % ("a depth target", "depth term")),
    ("normal-window", "normal", "window", None, PARTIAL % "normal term"),
    ("normal-pose", "normal", "pose", None, POSE % ("a normal term", "normal term")),
    ("distortion-window", "distortion", "window", None, PARTIAL % "distortion term"),
    ("distortion-pose", "distortion", "pose", None, POSE % ("a distortion term", "distortion term")),
    ("feature-window", "feature", "window", None, PARTIAL % "feature term"),
    ("feature-pose", "feature", "pose", None, POSE % ("a feature term", "feature term")),
    # the winner depends on the order of the checks: size before frame, camera before frame, pose before rows
    ("depth-size-window", "depth", "window", "size", "train_step: the depth target's size differs from the camera's"),
    ("normal-fisheye-window", "normal", "window", "fisheye",
     "train_step: the normal term needs a pinhole camera (the normals of a depth map are defined for it alone)"),
    ("feature-rows-pose", "feature", "pose", "rows", POSE % ("a feature term", "feature term")),
]


def _scene():
    return synth.make_scene(N, 0x7E5, sh_degree=0, log_scale_range=(math.log(0.1), math.log(0.5)),
                            tan_half_fov=(math.tan(math.radians(50)), math.tan(math.radians(50))))


def _gt(dev):
    return torch.from_numpy(np.ascontiguousarray(synth.synthetic_gt_packed(W, H)).view(np.int32)).to(dev)


def _splats(ba, sc, dev):
    return ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)


def _bits(spl):
    return [t.contiguous().view(torch.int32).clone() for t in (spl.transforms, spl.sh_coeffs, spl.raw_opacities)]


class _Refused:
    """One ctx with a trainer whose next step is refused as `case` says; `clear()` removes the obstacle and the term."""

    def __init__(self, ba, dev, term, obstacle, twist):
        from brush_amd import _ffi
        from brush_amd.host import _ptr
        self.ba, self.ctx = ba, ba.Context(dev)
        ctx = self.ctx
        self.sc = _scene()
        cp = synth.default_camera_params(W, H)
        self.cam = self.bad_cam = util.hip_camera(ba, cp)
        self.gt, self.spl = _gt(dev), _splats(ba, self.sc, dev)
        self.keep = []
        cfg_kw, tr_kw, batch_kw = {}, {}, {}
        if term == "exposure":
            tr_kw["exposure"] = ba.ExposureTable(2, ctx=ctx)
        elif term == "bilagrid":
            tr_kw["bilagrid"] = ba.BilateralGridTable(2, grid=(4, 4, 2), ctx=ctx)
        elif term == "depth":
            cfg_kw["depth_loss_weight"] = 0.5
            if twist != "size":
                batch_kw["depth"] = torch.full((H, W), 3.0, dtype=torch.float32, device=dev)
        elif term == "normal":
            cfg_kw["normal_loss_weight"] = 0.5
            if twist == "fisheye":
                kb4 = {k: v for k, v in cp.items() if k not in ("img_w", "img_h")}
                kb4["model"], kb4["dist"] = util.REF_LENSES["kb4"]
                self.bad_cam = util.hip_camera(ba, kb4)
        elif term == "distortion":
            cfg_kw["distortion_loss_weight"] = 0.5
        elif term == "feature":
            cfg_kw["feature_loss_weight"] = 1.0
            tr_kw["feature_field"] = ba.FeatureField(N + 1 if twist == "rows" else N, 3, device=dev, ctx=ctx)
            batch_kw["features"] = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        self.tr = ba.SplatTrainer(ba.TrainConfig(background_color=BG, **cfg_kw), median_scene_scale=3.0, ctx=ctx, **tr_kw)
        self.batch = ba.SceneBatch(self.gt, self.bad_cam, view_id=2, **batch_kw)
        small = None
        if twist == "size":   # a target of half the camera's height, attached behind the trainer's own (it found no map in the batch)
            small = _ffi.BhDepthTarget()
            half = torch.full((H // 2, W), 3.0, dtype=torch.float32, device=dev)
            self.keep.append(half)
            small.gt, small.h, small.w, small.kind, small.weight, small.scale, small.offset = half.data_ptr(), H // 2, W, 0, 0.5, 1.0, 0.0

        def patch(b):
            if obstacle == "window":
                b.camera.tile_row_begin, b.camera.tile_row_end = 0, 1   # one of the frame's two tile rows
            if small is not None:
                ctx.check(ctx.lib.bh_train_set_depth(ctx._h, C.byref(small)))
        self.tr.batch_patch = patch
        if obstacle == "pose":
            buf = torch.zeros((12,), dtype=torch.float32, device=dev)
            self.keep.append(buf)
            ctx.check(ctx.lib.bh_train_set_pose_grad(ctx._h, _ptr(buf)))
        torch.cuda.synchronize()

    def refused_step(self):
        with pytest.raises(self.ba.BrushHipError) as e:
            self.tr.step(self.batch, self.spl)
        return str(e.value)

    def clear(self):
        tr, ctx = self.tr, self.ctx
        ctx.check(ctx.lib.bh_train_set_pose_grad(ctx._h, None))
        tr.batch_patch, tr.exposure, tr.bilagrid, tr.feature_field = None, None, None, None
        tr.config = self.ba.TrainConfig(background_color=BG)
        return self.ba.SceneBatch(self.gt, self.cam, view_id=2)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_first_refusal_text_per_term(dev, case):
    import brush_amd as ba
    _, term, obstacle, twist, text = case
    r = _Refused(ba, dev, term, obstacle, twist)
    try:
        assert r.refused_step() == "brush_hip error -1: " + text
    finally:
        r.ctx.close()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_refused_step_leaves_nothing_behind(dev, case):
    import brush_amd as ba
    _, term, obstacle, twist, _ = case
    r = _Refused(ba, dev, term, obstacle, twist)
    try:
        before = _bits(r.spl)
        r.refused_step()
        r.ctx.sync()
        assert r.tr.step_count == 0
        for a, b in zip(before, _bits(r.spl)):
            assert torch.equal(a, b)
        # the same trainer takes a plain step once the obstacle is gone: the refused step's terms were detached behind it
        _, st = r.tr.step(r.clear(), r.spl)
        r.ctx.sync()
        assert r.tr.step_count == 1 and math.isfinite(st.loss) and st.loss > 0
    finally:
        r.ctx.close()


def _raw_step(ba, ctx, spl, state, cam, gt, step_count):
    """One bh_train_step by hand (frozen learning rates, complete lists, no noise) -> (rc, the step's loss)."""
    from brush_amd import _ffi
    c = ba.TrainConfig(background_color=BG, exact_lists=True, **FROZEN)
    cfg = _ffi.BhTrainConfig()
    cfg.lr_mean, cfg.lr_mean_end, cfg.total_train_iters = c.lr_mean, c.lr_mean_end, c.total_train_iters
    cfg.lr_coeffs_dc, cfg.lr_coeffs_sh_scale, cfg.lr_opac = c.lr_coeffs_dc, c.lr_coeffs_sh_scale, c.lr_opac
    cfg.lr_scale, cfg.lr_rotation, cfg.ssim_weight = c.lr_scale, c.lr_rotation, c.ssim_weight
    cfg.match_alpha_weight, cfg.mean_noise_weight, cfg.median_scene_scale = c.match_alpha_weight, c.mean_noise_weight, 3.0
    cfg.exact_lists, cfg.growth_stop_iter = 1, c.growth_stop_iter
    st = _ffi.BhTrainState()
    st.n, st.sh_degree = spl.num_splats(), spl.sh_degree()
    st.transforms, st.sh_coeffs, st.raw_opacities = spl.transforms.data_ptr(), spl.sh_coeffs.data_ptr(), spl.raw_opacities.data_ptr()
    st.m1_transforms, st.m2_transforms = state["m1_t"].data_ptr(), state["m2_t"].data_ptr()
    st.m1_sh, st.m2_sh = state["m1_sh"].data_ptr(), state["m2_sh"].data_ptr()
    st.m1_opac, st.m2_opac = state["m1_o"].data_ptr(), state["m2_o"].data_ptr()
    st.refine_weight_norm, st.vis_weight, st.max_screen_size = (state[k].data_ptr() for k in ("refine_weight_norm", "vis_weight", "max_screen_size"))
    st.step_count = step_count
    b = _ffi.BhTrainBatch()
    b.camera = cam.uniforms((W, H))
    b.gt_packed, b.view_id = gt.data_ptr(), 2
    b.background[0], b.background[1], b.background[2] = BG
    stats = _ffi.BhTrainStats()
    rc = ctx.lib.bh_train_step(ctx._h, C.byref(cfg), C.byref(st), C.byref(b), None, None, 1.0, C.byref(stats))
    ctx.check(rc)
    ctx.sync()   # (delivers the loss into `stats`)
    assert st.step_count == step_count + 1
    return np.float32(stats.loss)


def test_terms_are_ctx_state(dev):
    import brush_amd as ba
    from brush_amd import _ffi
    sc = _scene()
    ctx = ba.Context(dev)
    try:
        cam, gt, spl = util.hip_camera(ba, synth.default_camera_params(W, H)), _gt(dev), _splats(ba, sc, dev)
        holder = ba.SplatTrainer(ba.TrainConfig(), ctx=ctx)
        holder._init_state(spl)   # (the moments and statistics of a state, zeroed)
        torch.cuda.synchronize()
        plain = _raw_step(ba, ctx, spl, holder.state, cam, gt, 0)
        assert math.isfinite(plain) and plain > 0
        # attached directly: every raw step carries the term until it is detached
        ctx.check(ctx.lib.bh_train_set_normal(ctx._h, C.byref(_ffi.BhNormalTermConfig(weight=0.5))))
        with_term = [_raw_step(ba, ctx, spl, holder.state, cam, gt, k) for k in (1, 2)]
        assert all(math.isfinite(v) and v > plain for v in with_term), (plain, with_term)
        assert with_term[0].tobytes() == with_term[1].tobytes()   # (nothing moved: the same frame, the same complete lists)
        ctx.check(ctx.lib.bh_train_set_normal(ctx._h, None))
        assert _raw_step(ba, ctx, spl, holder.state, cam, gt, 3).tobytes() == plain.tobytes()
        # a trainer's step attaches its own terms and detaches them behind it, also when the step raises
        tr = ba.SplatTrainer(ba.TrainConfig(background_color=BG, normal_loss_weight=0.5, distortion_loss_weight=0.5), median_scene_scale=3.0, ctx=ctx)

        def window(b):
            b.camera.tile_row_begin, b.camera.tile_row_end = 0, 1
        tr.batch_patch = window
        with pytest.raises(ba.BrushHipError, match="normal term"):
            tr.step(ba.SceneBatch(gt, cam, view_id=2), _splats(ba, sc, dev))
        assert _raw_step(ba, ctx, spl, holder.state, cam, gt, 4).tobytes() == plain.tobytes()
    finally:
        ctx.close()
