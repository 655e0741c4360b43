"""Numpy restatement of mask lifting (include/brush_hip_lift.h) — TEST INFRASTRUCTURE ONLY.

votes_from_weights(): the votes, the largest weight and the pixel count of every splat from its f32 blend weights at every pixel:
a vote is q = rint(w * 2^24) (the product is exact in f32, numpy's rint rounds half to even as v_rndne_f32 does), sums are int64.
assign() / select(): the two element-wise steps in integer and f64 arithmetic, as the header states them.

Also the scenes the lifting tests share: ref_case() (the 300-splat 64 x 48 case of tests/test_gpu_features.py::_ref_case), its
float64 render (reference(), rendered once per case and never written) and the two-object scene of the end-to-end tests.
"""
import functools
import math

import numpy as np

VOTE_ONE = 1 << 24
UNASSIGNED = 255


def quantise(w):
    """int64 votes of f32 weights: ONE rounding, half to even."""
    w = np.asarray(w)
    assert w.dtype == np.float32
    return np.rint(w * np.float32(VOTE_ONE)).astype(np.int64)


def votes_from_weights(w, labels, num_labels):
    """w [N,H,W] f32 (0 where the splat does not contribute), labels uint8 [H,W] or None (label 0 everywhere) ->
    (votes int64 [N,L], max_weight f32 [N], pixel_count int64 [N]).  A pixel whose label is >= num_labels votes nowhere; it still
    counts in the other two."""
    w = np.asarray(w)
    assert w.dtype == np.float32 and w.ndim == 3
    n = w.shape[0]
    lab = np.zeros(w.shape[1:], np.int64) if labels is None else np.asarray(labels).astype(np.int64)
    assert lab.shape == w.shape[1:]
    q = quantise(w).reshape(n, -1)
    column = np.minimum(lab.reshape(-1), num_labels)   # column L takes the pixels that vote nowhere, and is dropped
    votes = np.zeros((n, num_labels + 1), np.int64)
    np.add.at(votes, (np.arange(n)[:, None], column[None, :]), q)   # integer additions
    return votes[:, :num_labels].copy(), w.reshape(n, -1).max(axis=1), (w > 0).reshape(n, -1).sum(axis=1)


def min_total(min_weight):
    """(uint64_t)rint((double)min_weight * 2^24) of the f32 the C call receives; not > 0: 0."""
    mw = np.float32(min_weight)
    return int(np.rint(np.float64(mw) * float(VOTE_ONE))) if mw > 0 else 0


def assign(votes, min_weight=0.0):
    """-> (labels uint8 [N], share f32 [N]): the argmax of the row, ties to the lowest label; 255 and +0 where the row's total is 0 or
    below the threshold."""
    votes = np.asarray(votes, np.int64)
    total = votes.sum(axis=1)
    best = np.argmax(votes, axis=1)   # the first maximum
    ok = (total != 0) & (total >= min_total(min_weight))
    top = votes[np.arange(votes.shape[0]), best]
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(ok, top.astype(np.float64) / total.astype(np.float64), 0.0).astype(np.float32)
    return np.where(ok, best, UNASSIGNED).astype(np.uint8), share


def select(votes=None, max_weight=None, pixel_count=None, label=None, min_share=0.5, min_weight=0.0, min_max_weight=0.0, min_pixels=0, invert=False, n=None):
    """-> keep f32 [N] 1.0 / 0.0, every test asked for ANDed, then inverted.  A test whose table is None raises ValueError (the
    library refuses it)."""
    if votes is None and (label is not None or np.float32(min_weight) > 0):
        raise ValueError("a label or a min_weight needs the votes")
    if max_weight is None and np.float32(min_max_weight) > 0:
        raise ValueError("min_max_weight needs max_weight")
    if pixel_count is None and min_pixels > 0:
        raise ValueError("min_pixels needs pixel_count")
    n = n if votes is None else np.asarray(votes).shape[0]
    keep = np.ones(n, bool)
    if votes is not None:
        votes = np.asarray(votes, np.int64)
        total = votes.sum(axis=1)
        keep &= (total != 0) & (total >= min_total(min_weight))
        if label is not None:
            keep &= votes[:, label].astype(np.float64) >= np.float64(np.float32(min_share)) * total.astype(np.float64)
    if np.float32(min_max_weight) > 0:
        keep &= np.asarray(max_weight, np.float32) >= np.float32(min_max_weight)
    if min_pixels > 0:
        keep &= np.asarray(pixel_count).astype(np.int64) >= int(min_pixels)
    if invert:
        keep = ~keep
    return keep.astype(np.float32)


# ---- shared scenes ------------------------------------------------------------------------------------------------------------------
def _camera(w, h):
    from brush_amd import synth
    cp = synth.default_camera_params(w, h)
    return {k: v for k, v in cp.items() if k not in ("img_w", "img_h")}


def ref_case(model):
    """tests/test_gpu_features.py::_ref_case: 300 splats, 64 x 48, lists longer than one 64-entry batch."""
    from brush_amd import synth
    import util
    w, h = 64, 48
    cp = _camera(w, h)
    tans = (math.tan(cp["fov_x"] / 2.0), math.tan(cp["fov_y"] / 2.0))
    sc = synth.make_scene(300, 0xE5, sh_degree=0, log_scale_range=(math.log(0.05), math.log(0.4)), z_range=(2.0, 9.0), tan_half_fov=tans)
    cp["pos"] = (0.15, -0.1, -0.4)
    cp["rot_xyzw"] = util.quat_from_axis_angle((0.3, 1.0, 0.1), 0.08)
    if model != "pinhole":
        cp["model"], cp["dist"] = util.REF_LENSES[model]
    return sc, cp, w, h


def render_f64(sc, cp, w, h, mip=False, smooth=False):
    """tests/feature_ref.py::render of a scene without features: dict with vis [N,h,w], alpha [h,w], the tie margins (numpy)."""
    import torch
    import depth_ref
    import feature_ref
    # (leaves that require a gradient: the lens models take their Jacobian by autograd)
    leaves = [torch.tensor(np.asarray(sc[k], np.float64), requires_grad=True) for k in ("transforms", "sh", "raw_opac")]
    intr = depth_ref.intrinsics(cp, w, h) if cp.get("model", "pinhole") != "pinhole" else None
    n = leaves[0].shape[0]
    with torch.enable_grad():
        out = feature_ref.render(*leaves, torch.zeros((n, 1), dtype=torch.float64), cp, w, h, intrinsics=intr, mip=mip, smooth=smooth, map_grad=False)
    return {k: v.detach() if torch.is_tensor(v) else v for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def reference(model, mip, smooth):
    """(scene, camera, w, h, out) of ref_case(model): rendered once, shared, never written."""
    sc, cp, w, h = ref_case(model)
    return sc, cp, w, h, render_f64(sc, cp, w, h, mip, smooth)


def two_cluster_case():
    """Two separated objects in front of three cameras: (scene, cameras, w, h, member int [N] = the cluster of every splat)."""
    import util
    w, h, per = 64, 48, 40
    rng = np.random.default_rng(0x2C1)
    centres = np.array([[-1.3, 0.1, 5.0], [1.3, -0.1, 5.2]])
    means = np.concatenate([c + rng.uniform(-0.45, 0.45, (per, 3)) for c in centres]).astype(np.float32)
    member = np.repeat(np.arange(2), per)
    quats = rng.normal(size=(2 * per, 4)).astype(np.float32)
    ls = np.log(rng.uniform(0.08, 0.16, (2 * per, 3))).astype(np.float32)
    p = rng.uniform(0.6, 0.9, 2 * per)
    sc = dict(transforms=np.ascontiguousarray(np.concatenate([means, quats, ls], axis=1), np.float32),
              sh=np.ascontiguousarray(rng.uniform(0.2, 1.2, (2 * per, 1, 3)), np.float32), raw_opac=np.log(p / (1.0 - p)).astype(np.float32))
    cams = []
    for x, yaw in ((0.0, 0.0), (-0.8, 0.12), (0.8, -0.12)):
        cp = _camera(w, h)
        cp["pos"] = (x, 0.0, 0.0)
        cp["rot_xyzw"] = util.quat_from_axis_angle((0.0, 1.0, 0.0), yaw)
        cams.append(cp)
    return sc, cams, w, h, member


def subset(sc, rows):
    return {k: np.ascontiguousarray(v[rows]) for k, v in sc.items()}


def cluster_labels(alpha0, alpha1, threshold=0.3):
    """uint8 [H,W] from each cluster's own rendered alpha: 0 / 1 where that cluster's alpha exceeds the threshold (the larger one where
    both do), 255 elsewhere."""
    a0, a1 = np.asarray(alpha0, np.float64), np.asarray(alpha1, np.float64)
    lab = np.full(a0.shape, 255, np.uint8)
    lab[(a0 > threshold) & (a0 >= a1)] = 0
    lab[(a1 > threshold) & (a1 > a0)] = 1
    return lab
