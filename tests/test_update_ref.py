"""tests/update_ref.py is wired to the oracle, not to the kernel it judges: fed the gradients one OracleTrainer.step returns, it
produces OracleTrainer's own next parameters, moments and statistics bit for bit — over consecutive steps, and for a two-view
sum with the 1/world gradient scale.  No GPU."""
import math
import types

import numpy as np
import pytest

from brush_amd import synth
import update_ref as ur

CFG = types.SimpleNamespace(total_train_iters=30000, lr_mean=2e-5, lr_mean_end=2e-7, lr_coeffs_dc=2e-3, lr_coeffs_sh_scale=10.0,
                            lr_opac=0.012, lr_scale=5e-3, lr_rotation=2e-3, ssim_weight=0.2, match_alpha_weight=0.1,
                            mean_noise_weight=0.0, render_mip=False)
W, H, MEDIAN = 48, 32, 3.0


def _problem(oracle_lib, sh_degree, n=150):
    sc = synth.make_scene(n, 0xA0 + sh_degree, sh_degree=sh_degree, log_scale_range=(math.log(0.05), math.log(0.3)),
                          tan_half_fov=(math.tan(math.radians(30)), math.tan(math.radians(30)) * H / W))
    return sc, synth.default_camera_params(W, H), synth.synthetic_gt_packed(W, H)


def _params(sc):
    return dict(transforms=sc["transforms"].copy(), sh=sc["sh"].copy(), opac=sc["raw_opac"].copy())


def _oracle_state(otr):
    s = otr.state
    return dict(m1_t=s["m1_t"], m2_t=s["m2_t"], m1_sh=s["m1_sh"], m2_sh=s["m2_sh"], m1_o=s["m1_o"].reshape(-1), m2_o=s["m2_o"].reshape(-1),
                refine_weight_norm=s["refine"], vis_weight=s["vis"], max_screen_size=s["screen"])


def _assert_same(params, state, sc, otr, what):
    want = dict(_oracle_state(otr), transforms=sc["transforms"], sh=sc["sh"], opac=sc["raw_opac"])
    got = dict(state, **params)
    for k in ur.KEYS:
        assert ur.first_difference(got[k], want[k]) is None, (what, k, ur.first_difference(got[k], want[k]))


@pytest.mark.parametrize("sh_degree", [0, 2])
def test_update_ref_is_the_oracle_trainers_tail(oracle_lib, sh_degree):
    from oracle.trainer import OracleTrainer
    sc, cp, gt = _problem(oracle_lib, sh_degree)
    n = sc["transforms"].shape[0]
    otr = OracleTrainer(oracle_lib, CFG, median_scene_scale=MEDIAN)
    cam = oracle_lib.camera(**cp)
    params, state = _params(sc), ur.zero_state(n, sc["sh"].shape[1] * 3)
    for t in range(1, 4):
        ref = otr.step(sc, cam, gt, (0.1, 0.2, 0.3))
        g = ref["grads"]
        assert np.abs(g["g_tr"]).max() > 0 and g["vis"].max() == 1.0   # a step that trains something
        params, state = ur.update_ref(oracle_lib, params, state, g["vis"], g["g_tr"], g["g_sh"], g["g_op"], g["refine"], g["radius"],
                                      CFG, t, 1.0, MEDIAN)
        assert math.isclose(ur.lr_mean_at(CFG, t, MEDIAN), ref["lr_mean"], rel_tol=0, abs_tol=0)
        _assert_same(params, state, sc, otr, "step %d" % t)


def test_update_ref_scales_a_sum_over_two_views(oracle_lib):
    """Data parallel over cameras: the ranks' gradients and visible flags summed, the maxima of refine weight and radius, and
    grad_scale = 1/2 — OracleTrainer.step(extra_grads=, world=2)."""
    from oracle.trainer import OracleTrainer
    sc, cp, gt = _problem(oracle_lib, 1)
    n = sc["transforms"].shape[0]
    cp2 = dict(cp, pos=(cp["pos"][0] + 0.4, cp["pos"][1], cp["pos"][2]))
    cams = [oracle_lib.camera(**cp), oracle_lib.camera(**cp2)]
    otr = OracleTrainer(oracle_lib, CFG, median_scene_scale=MEDIAN)
    params, state = _params(sc), ur.zero_state(n, sc["sh"].shape[1] * 3)
    for t in range(1, 3):
        a = otr.step(sc, cams[0], gt, (0.0, 0.0, 0.0), dry_run=True)
        b = otr.step(sc, cams[1], gt, (0.0, 0.0, 0.0), dry_run=True)
        assert b["vis"].max() == 1.0 and (a["vis"] + b["vis"]).max() == 2.0
        otr.step(sc, cams[0], gt, (0.0, 0.0, 0.0), extra_grads=[b], world=2)
        params, state = ur.update_ref(oracle_lib, params, state, a["vis"] + b["vis"], a["g_tr"] + b["g_tr"], a["g_sh"] + b["g_sh"],
                                      a["g_op"] + b["g_op"], np.maximum(a["refine"], b["refine"]), np.maximum(a["radius"], b["radius"]),
                                      CFG, t, 1.0 / 2, MEDIAN)
        _assert_same(params, state, sc, otr, "step %d" % t)
