"""Feature maps end to end (include/brush_hip_features.h): a zero-initialised FeatureField on a frozen 300-splat scene
learns the argmax labels of a 4-channel teacher from two views by cross-entropy, through render / loss / backward / step on the GPU.

The same loop runs first in float64 on the CPU: the map is linear in the features, F = sum of vis_i f_i with the per-splat weights
of tests/feature_ref.py rendered once per view, the loss is feature_ref.cross_entropy_loss, the optimiser a plain Adam.  STEPS is
chosen so that this reference alone brings the mean loss of the two views to <= 1/4 of its first value; the GPU run must reach
<= 1/2: a coarse cap that a wrong gradient does not meet, not a measurement."""
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import depth_ref
import feature_ref
import util

pytestmark = pytest.mark.gpu
C = 4
STEPS = 60   # (the float64 reference: 0.203 of the first loss at LR = 0.3; 0.324 at 0.1)
LR = 0.3
W, H = 64, 48


def _views():
    cp = synth.default_camera_params(W, H)
    tans = (math.tan(cp["fov_x"] / 2.0), math.tan(cp["fov_y"] / 2.0))
    sc = synth.make_scene(300, 0xE5, sh_degree=0, log_scale_range=(math.log(0.05), math.log(0.4)), z_range=(2.0, 9.0), tan_half_fov=tans)
    cp = {k: v for k, v in cp.items() if k not in ("img_w", "img_h")}
    views = []
    for pos, angle in (((0.15, -0.1, -0.4), 0.08), ((-0.3, 0.1, -0.2), -0.06)):
        v = dict(cp)
        v["pos"], v["rot_xyzw"] = pos, util.quat_from_axis_angle((0.3, 1.0, 0.1), angle)
        views.append(v)
    return sc, views


def _reference_run(sc, views, teacher):
    """-> (labels per view, loss ratio last / first, vis per view) of the float64 loop."""
    leaves = [torch.tensor(np.asarray(sc[k], np.float64)) for k in ("transforms", "sh", "raw_opac")]
    vis, labels = [], []
    for cp in views:
        with torch.no_grad():
            out = feature_ref.render(*leaves, torch.tensor(teacher.astype(np.float64)), cp, W, H, intrinsics=depth_ref.intrinsics(cp, W, H), map_grad=False)
        lab = out["feat"].numpy().argmax(-1).astype(np.uint8)
        lab[out["alpha"].numpy() == 0.0] = 255
        vis.append(out["vis"].numpy())
        labels.append(lab)
    f = np.zeros((teacher.shape[0], C))
    m1, m2 = np.zeros_like(f), np.zeros_like(f)
    losses = []
    for t in range(1, STEPS + 1):
        k = (t - 1) % len(views)
        fmap = np.einsum("nhw,nc->hwc", vis[k], f)
        loss, _, v = feature_ref.cross_entropy_loss(fmap.astype(np.float32), labels[k])
        g = np.einsum("nhw,hwc->nc", vis[k], v)
        m1 = 0.9 * m1 + 0.1 * g
        m2 = 0.999 * m2 + 0.001 * g * g
        f = f - LR * (m1 / (1 - 0.9 ** t)) / (np.sqrt(m2 / (1 - 0.999 ** t)) + 1e-15)
        losses.append(loss)
    return labels, (losses[-1] + losses[-2]) / (losses[0] + losses[1]), vis


def test_a_feature_field_learns_the_teachers_labels(dev):
    import brush_amd as ba
    sc, views = _views()
    n = sc["transforms"].shape[0]
    teacher = np.random.default_rng(0x7EAC).normal(0.0, 1.0, (n, C)).astype(np.float32)
    labels, ref_ratio, _ = _reference_run(sc, views, teacher)
    assert all(0.3 < float((lab < C).mean()) for lab in labels) and all((lab == 255).any() for lab in labels)
    assert ref_ratio <= 0.25, ref_ratio
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    ctx = ba.Context(dev)
    try:
        nodes = [ba.render_splats_diff(spl, util.hip_camera(ba, cp), (W, H), ctx=ctx, retain=True) for cp in views]
        lab_dev = [torch.from_numpy(lab).to(dev) for lab in labels]
        field = ba.FeatureField(n, C, lr=LR, device=dev, ctx=ctx)
        assert not bool(field.features.any())
        losses = []
        for t in range(STEPS):
            k = t % len(views)
            fmap = field.render(nodes[k])
            loss, v = ba.feature_loss_value_and_grad(fmap, lab_dev[k], "cross_entropy", ctx=ctx)
            field.step(field.backward(nodes[k], v)["v_features"])
            losses.append(loss)
        ctx.sync()
        losses = [float(x[0]) for x in losses]
        ratio = (losses[-1] + losses[-2]) / (losses[0] + losses[1])
        acc = []
        for k, node in enumerate(nodes):
            pred = field.render(node).argmax(-1).cpu().numpy()
            ok = labels[k] < C
            acc.append(float((pred[ok] == labels[k][ok]).mean()))
            node.release()
        print("loss ratio after %d steps: float64 reference %.4f, GPU %.4f; first loss %.4f; pixel accuracy %s" % (STEPS, ref_ratio, ratio, losses[0], acc))
        assert field.t == STEPS and abs(losses[0] - math.log(C) * float((labels[0] < C).mean())) <= 1e-5
        assert ratio <= 0.5, ratio
    finally:
        ctx.close()
