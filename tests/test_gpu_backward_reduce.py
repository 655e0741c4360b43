"""The per-splat wave reduction at the end of the blend backward (rasterize.hip K17, device_blend.h row_allreduce3_folded): the ten
sums of a (splat, tile) are folded into ONE register while they are reduced, and lanes 0 / 4 / 12 of the 16-lane rows send them.
A wrong fold puts a value into the wrong component, or drops it — which a frame with many contributing lanes can hide behind its
tolerance and a frame with ONE contributing lane cannot.

Reference and tolerance are those of test_gpu_backward.py: the oracle backward, per tensor 1e-4 * max|g| and that file's
per-element rule (assert_grads_match).  The variant without the refine weight only runs inside a train step (growth_stop_iter, as
in test_gpu_options.py): there the accumulator of a step without it is compared with the accumulator of the same step with it —
the nine other sums are the same instructions in the same order — whose kernel the other cases hold against the oracle."""
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import util
from test_gpu_backward import GRAD_TOL, assert_grads_match, mixed_violations, run_both

pytestmark = pytest.mark.gpu
TAN30 = math.tan(math.radians(30.0))


def _tile_scene(n, seed, w, h, log_scale, opacity=(0.05, 0.95), spread=0.9):
    """n seeded splats in front of a w x h frame of the default camera."""
    return synth.make_scene(n, seed, sh_degree=0, log_scale_range=(math.log(log_scale[0]), math.log(log_scale[1])), z_range=(3.0, 8.0),
                            tan_half_fov=(TAN30, TAN30 * h / w), spread=spread, opacity_range=opacity)


def _one_tile_eight():
    return _tile_scene(8, 0xA17, 16, 16, (0.4, 1.5))


def _ragged():
    return _tile_scene(200, 0xA18, 40, 24, (0.05, 0.5))


def _faint(n=320):
    return _tile_scene(n, 0xA19, 16, 16, (0.6, 2.0), opacity=(0.015, 0.025), spread=0.6)


def _clamping():
    sc = _tile_scene(40, 0xA1A, 16, 16, (0.3, 1.2))
    front = int(np.argmin(sc["transforms"][:, 2]))
    sc["raw_opac"][front] = 10.0                           # sigmoid = 0.99995: alpha0 above the 0.999 clamp
    sc["transforms"][front, 0:2] = (0.3, -0.2)             # near the middle of the tile, and small: the others still blend around it
    sc["transforms"][front, 7:10] = math.log(0.25)
    return sc


def _train_accumulators(ba, dev, sc, w, h, options=None):
    """The blend backward's accumulator [rows, 10] after ONE train step, with the refine weight and without it (growth_stop_iter = 1)."""
    from brush_amd import host
    cam = util.hip_camera(ba, synth.default_camera_params(w, h))
    gt = torch.from_numpy(synth.synthetic_gt_packed(w, h).view(np.int32)).to(dev)
    out = []
    for stop in (15000, 1):
        ctx = ba.Context(dev, options=dict(options or {}))
        spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
        trainer = ba.SplatTrainer(ba.TrainConfig(growth_stop_iter=stop), median_scene_scale=3.0, ctx=ctx)
        trainer.step(ba.SceneBatch(gt, cam), spl, background=(0.1, 0.2, 0.3))
        ctx.sync()
        rows = trainer.stats(ctx).num_visible
        assert rows > 0
        out.append(host._view(ctx.lib.bh_last_v_combined(ctx._h), (rows, 10), torch.float32, dev).clone().cpu().numpy())
        ctx.close()
    return out


def _assert_nine_sums_without_refine(with_rf, without_rf):
    assert with_rf.shape == without_rf.shape
    assert float(np.abs(with_rf[:, 9]).max()) > 0.0 and not without_rf[:, 9].any()   # the tenth sum: computed / left out (exact zeros)
    for c in range(9):
        assert float(np.abs(with_rf[:, c]).max()) > 0.0, c
        assert util.rel_linf(without_rf[:, c], with_rf[:, c]) <= GRAD_TOL, (c, util.rel_linf(without_rf[:, c], with_rf[:, c]))
        assert mixed_violations(without_rf[:, c], with_rf[:, c])[0] == 0, (c, mixed_violations(without_rf[:, c], with_rf[:, c]))


def test_every_lane_reaches_every_component(dev, oracle_lib):
    """One tile, eight splats, v_output one-hot at each of the 256 pixels in turn: a single lane of the wave contributes, and every
    one of the ten sums of every splat it touches has to come out in its own column."""
    import brush_amd as ba
    w = h = 16
    sc = _one_tile_eight()
    cp = synth.default_camera_params(w, h)
    touched = 0
    for pix in range(w * h):
        v_out = np.zeros((h, w, 4), np.float32)
        v_out[pix // w, pix % w] = (1.0, -0.6, 0.8, 0.5)
        res, ref = run_both(ba, oracle_lib, dev, sc, cp, w, h, v_out, bg=(0.2, 0.3, 0.1))
        assert_grads_match(res, ref)
        touched += int(np.abs(ref.get("v_combined")).max() > 0.0)
    assert touched >= 200, touched   # the splats cover the tile: nearly every pixel has a gradient to get wrong


@pytest.mark.parametrize("smooth", [False, True])
def test_ragged_frame_several_tiles(dev, oracle_lib, smooth):
    import brush_amd as ba
    w, h = 40, 24
    v_out = (np.random.default_rng(40 * 24).uniform(-1, 1, (h, w, 4)) / (h * w)).astype(np.float32)
    pass_ = ba.RasterPass.BackwardSmoothCutoff if smooth else ba.RasterPass.Backward
    res, ref = run_both(ba, oracle_lib, dev, _ragged(), synth.default_camera_params(w, h), w, h, v_out, bg=(0.7, 0.1, 0.4), pass_=pass_)
    assert float(np.abs(ref.get("v_combined")).max()) > 0.0
    assert_grads_match(res, ref)


def test_accumulator_addressed_in_64_bits(dev, oracle_lib):
    """From 2^32 bytes of accumulator on the kernel forms the row's address in 64 bits instead of adding a staged byte offset in 32;
    option bwd_wide_rows = 1 runs that variant at any size."""
    import brush_amd as ba
    w, h = 40, 24
    sc, cp = _ragged(), synth.default_camera_params(w, h)
    v_out = (np.random.default_rng(7).uniform(-1, 1, (h, w, 4)) / (h * w)).astype(np.float32)
    p = {k: v for k, v in cp.items() if k not in ("img_w", "img_h")}
    ref = oracle_lib.Render().forward(oracle_lib.camera(img_w=w, img_h=h, **p), sc["transforms"], sc["sh"], sc["raw_opac"], bg=(0.1, 0.2, 0.3),
                                      flags=oracle_lib.FLAG_BWD_INFO)
    ref.backward(v_out)
    for jobs in (1, 0):
        ctx = ba.Context(dev, options={"bwd_wide_rows": 1, "bwd_jobs": jobs})
        spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
        res = ba.render_splats_bwd(spl, util.hip_camera(ba, cp), (w, h), (0.1, 0.2, 0.3), torch.from_numpy(v_out).to(dev), ctx=ctx)
        assert_grads_match(res, ref)
        ctx.close()


def test_across_a_job_boundary(dev, oracle_lib):
    """One tile whose list of faint splats spans three 128-entry segments: the gradients through jobs equal those through whole tiles
    (option bwd_jobs = 0), and both equal the oracle's."""
    import brush_amd as ba
    w = h = 16
    sc = _faint()
    cp = synth.default_camera_params(w, h)
    v_out = (np.random.default_rng(5).uniform(-1, 1, (h, w, 4)) / (h * w)).astype(np.float32)
    p = {k: v for k, v in cp.items() if k not in ("img_w", "img_h")}
    ref = oracle_lib.Render().forward(oracle_lib.camera(img_w=w, img_h=h, **p), sc["transforms"], sc["sh"], sc["raw_opac"], bg=(0.1, 0.2, 0.3),
                                      flags=oracle_lib.FLAG_BWD_INFO)
    ref.backward(v_out)
    got = {}
    for jobs in (1, 0):
        ctx = ba.Context(dev, options={"bwd_jobs": jobs})
        spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
        res = ba.render_splats_bwd(spl, util.hip_camera(ba, cp), (w, h), (0.1, 0.2, 0.3), torch.from_numpy(v_out).to(dev), ctx=ctx)
        to = util.u32(res["aux"].tile_offsets).reshape(-1, 2).astype(np.int64)
        assert to.shape[0] == 1 and int(to[0, 1] - to[0, 0]) > 2 * 128, to   # one tile, three segments
        assert_grads_match(res, ref)
        got[jobs] = {k: res[k].cpu().numpy() for k in ("v_combined", "v_transforms", "v_sh_coeffs", "v_raw_opacities", "v_refine_weight")}
        ctx.close()
    for k in got[1]:
        cols = 10 if k in ("v_combined", "v_transforms") else 1
        a, b = got[1][k].reshape(-1, cols), got[0][k].reshape(-1, cols)
        for c in range(cols):
            assert util.rel_linf(a[:, c], b[:, c]) <= GRAD_TOL, (k, c, util.rel_linf(a[:, c], b[:, c]))


def test_a_batch_that_clamps(dev, oracle_lib):
    """A splat with alpha0 > 0.999 in front of an ordinary list: its batch runs the variant of the splat loop that carries the clamp,
    the other cases of this file the one without — both end in the same reduction."""
    import brush_amd as ba
    w = h = 16
    sc = _clamping()
    assert 1.0 / (1.0 + math.exp(-float(sc["raw_opac"].max()))) > 0.999
    v_out = (np.random.default_rng(6).uniform(-1, 1, (h, w, 4)) / (h * w)).astype(np.float32)
    res, ref = run_both(ba, oracle_lib, dev, sc, synth.default_camera_params(w, h), w, h, v_out, bg=(0.2, 0.3, 0.1))
    assert res["aux"].num_visible == 40
    assert_grads_match(res, ref)


@pytest.mark.parametrize("case,options", [("one_tile", None), ("ragged", None), ("faint_jobs", None), ("faint_tiles", {"bwd_jobs": 0}), ("clamping", None)])
def test_without_the_refine_weight_the_other_nine_sums_stay(dev, case, options):
    import brush_amd as ba
    sc, w, h = {"one_tile": (_one_tile_eight, 16, 16), "ragged": (_ragged, 40, 24), "faint_jobs": (_faint, 16, 16), "faint_tiles": (_faint, 16, 16),
                "clamping": (_clamping, 16, 16)}[case]
    with_rf, without_rf = _train_accumulators(ba, dev, sc(), w, h, options)
    _assert_nine_sums_without_refine(with_rf, without_rf)
