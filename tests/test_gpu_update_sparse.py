"""The update kernel's second path (optim.hip, option `update_sparse`): a block with few non-dormant rows compacts them and fetches
everything it still needs in one round trip, element-wise over the listed rows.  It must leave every tensor — parameters, every
moment with its sign marks, the three statistics — bit for bit as the dense path leaves them.  As in
test_gpu_masked_grads.py::test_dormant_splats_are_skipped_without_changing_a_bit the image is ONE 16 x 16 tile: every splat has at
most one (splat, tile) pair, the backward's atomics add each gradient once into a zero, the step is deterministic.
update_sparse = 0: no block takes the path; 256: every block that may skip dormant rows does; unset: the library's default."""
import math

import numpy as np
import pytest
import torch

from brush_amd import synth
import util

pytestmark = pytest.mark.gpu

W = H = 16
MARK = -2147483648   # the bits of -0.0f: m2_sh of a dormant splat


def _views(w, h, k):
    cp = synth.default_camera_params(w, h)
    out = []
    for i in range(k):
        c = dict(cp)
        c["rot_xyzw"] = util.quat_from_axis_angle((0, 1, 0), math.radians(-35 + 70 * i / max(1, k - 1)))
        out.append(c)
    return out


def _scene(n, sh_degree):
    return synth.make_scene(n, 0xD0A + n, sh_degree=sh_degree, log_scale_range=(math.log(0.05), math.log(0.4)),
                            tan_half_fov=(math.tan(math.radians(50)), math.tan(math.radians(50))))


def _train(ba, dev, sc, cams, option, steps=9, after_first=None, options=None):
    """`steps` default stochastic steps over `cams`; option: None (default), a value of update_sparse, or a function step -> value;
    options: further option keys, set once."""
    ctx = ba.Context(dev)
    try:
        for k, v in (options or {}).items():
            ctx.set_option(k, v)
        gt = torch.from_numpy(synth.synthetic_gt_packed(W, H).view(np.int32)).to(dev)
        spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
        tr = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=3.0, ctx=ctx, seed=77)
        for s in range(steps):
            v = option(s) if callable(option) else option
            if v is not None:
                ctx.set_option("update_sparse", v)
            tr.step(ba.SceneBatch(gt, util.hip_camera(ba, cams[s % len(cams)])), spl)
            if s == 0 and after_first is not None:
                ctx.sync()
                after_first(tr.state)
        ctx.sync()
        out = {"transforms": spl.transforms.clone(), "sh": spl.sh_coeffs.clone(), "opac": spl.raw_opacities.clone()}
        out.update({k: v.clone() for k, v in tr.state.items()})
        return out
    finally:
        ctx.close()


_DENSE = {}


def _dense(ba, dev, n, sh_degree):
    """The reference of a size: update_sparse = 0, computed once."""
    if (n, sh_degree) not in _DENSE:
        _DENSE[(n, sh_degree)] = _train(ba, dev, _scene(n, sh_degree), _views(W, H, 3), 0)
    return _DENSE[(n, sh_degree)]


def _assert_same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (what, k)


@pytest.mark.parametrize("n,sh_degree", [
    (6000, 0),   # 256 rows per block
    (6000, 2),   # 128
    (1500, 3),   # 64
    (300, 0), (300, 1),   # fewer splats than one block
    (257, 0), (257, 1),   # one full block + one row
])
def test_sparse_path_leaves_the_dense_paths_bits(dev, n, sh_degree):
    import brush_amd as ba
    sc, cams = _scene(n, sh_degree), _views(W, H, 3)
    ref = _dense(ba, dev, n, sh_degree)
    _assert_same_bits(_train(ba, dev, sc, cams, 256), ref, "update_sparse=256")
    _assert_same_bits(_train(ba, dev, sc, cams, None), ref, "default")
    if n >= 1500:   # the runs skip dormant splats (all three: the marks agree too) and train others
        marks = ref["m2_sh"].view(torch.int32) == MARK
        assert 0.25 < float(marks.float().mean()) < 1.0, float(marks.float().mean())
        assert float((ref["m2_t"].abs().sum(1) > 0).float().mean()) > 0.02


@pytest.mark.parametrize("sh_degree", [0, 3])
def test_every_row_active(dev, sh_degree):
    """300 faint, large splats in front of one camera: the tile never saturates (0.98^300 > the blend's cut-off), every splat
    receives a gradient at the first step and none is dormant afterwards — the sparse path, forced, walks its chunk loop over all
    256 (64) rows of a block, and its row sums and element updates are still the dense path's."""
    import brush_amd as ba
    n = 300
    sc = synth.make_scene(n, 0xAC7, sh_degree=sh_degree, log_scale_range=(math.log(0.3), math.log(0.6)), z_range=(2.0, 5.0),
                          tan_half_fov=(math.tan(math.radians(30)),) * 2, spread=0.6, opacity_range=(0.012, 0.02))
    cams = [synth.default_camera_params(W, H)]

    def none_dormant(state):
        assert not bool((state["m2_sh"].view(torch.int32) == MARK).any())
        assert bool((state["m2_t"].abs().sum(1) > 0).all())
    a = _train(ba, dev, sc, cams, 256, steps=6, after_first=none_dormant)
    b = _train(ba, dev, sc, cams, 0, steps=6, after_first=none_dormant)
    none_dormant(a)
    _assert_same_bits(a, b, "update_sparse=256 against 0")


@pytest.mark.parametrize("n,sh_degree", [(6000, 0), (6000, 2)])
def test_paths_alternate(dev, n, sh_degree):
    """One context, the option flipped in front of every step: the marks one path leaves are the marks the other reads."""
    import brush_amd as ba
    a = _train(ba, dev, _scene(n, sh_degree), _views(W, H, 3), lambda s: 256 if s % 2 else 0)
    _assert_same_bits(a, _dense(ba, dev, n, sh_degree), "alternating")
    b = _train(ba, dev, _scene(n, sh_degree), _views(W, H, 3), lambda s: 0 if s % 2 else 256)
    _assert_same_bits(b, _dense(ba, dev, n, sh_degree), "alternating, sparse first")


@pytest.mark.parametrize("n", [65, 129, 300])   # one full block of 64 / of 128 rows plus one row; a ragged tail behind several blocks
@pytest.mark.parametrize("sh_degree", [0, 1])
@pytest.mark.parametrize("rows", [64, 128])
def test_block_sizes_off_their_default(dev, rows, sh_degree, n):
    """Option update_rows: the 64- and 128-row instantiations, which by default run only at SH degree >= 2, on short SH rows.  Under
    the same block size the sparse path, forced and at its default, leaves the bits of the dense path."""
    import brush_amd as ba
    sc, cams = _scene(n, sh_degree), _views(W, H, 3)
    ref = _train(ba, dev, sc, cams, 0, options={"update_rows": rows})
    _assert_same_bits(_train(ba, dev, sc, cams, 256, options={"update_rows": rows}), ref, "update_sparse=256")
    _assert_same_bits(_train(ba, dev, sc, cams, None, options={"update_rows": rows}), ref, "default")
    if n == 300:   # some splats were found dormant (the runs skipped them: all three carry the same marks), others trained
        marks = ref["m2_sh"].view(torch.int32) == MARK
        assert 0 < int(marks.sum()) < n, int(marks.sum())
        assert bool((ref["m2_t"].abs().sum(1) > 0).any())


def _misalign_m1_t(state):
    """Rebinds the transforms' first moment to a copy whose data pointer is 4 mod 16: the launcher then takes the scalar
    (VEC = false) instantiations for every tensor.  (The step after this one finds a state it has not seen and processes every
    splat; the marks count again from the step behind it.)"""
    old = state["m1_t"]
    buf = torch.empty(old.numel() + 1, dtype=old.dtype, device=old.device)
    new = buf[1:].view(old.shape)
    new.copy_(old)
    assert new.data_ptr() % 16 == 4
    state["m1_t"] = new


_SCALAR_CASES = (("update_sparse=256", 256, None), ("update_sparse=0", 0, None), ("no_dormant=1", None, {"no_dormant": 1}))
_LAYOUTS = {}


def _layout_runs(ba, dev, sh_degree, misaligned):
    """The three runs of _SCALAR_CASES on one layout of the state, computed once."""
    key = (sh_degree, misaligned)
    if key not in _LAYOUTS:
        sc, cams = _scene(300, sh_degree), _views(W, H, 3)
        _LAYOUTS[key] = {what: _train(ba, dev, sc, cams, sparse, after_first=_misalign_m1_t if misaligned else None, options=opts)
                         for what, sparse, opts in _SCALAR_CASES}
    return _LAYOUTS[key]


@pytest.mark.parametrize("sh_degree", [0, 2])
@pytest.mark.parametrize("misaligned", [True, False])
def test_scalar_instantiations(dev, misaligned, sh_degree):
    """A state tensor off a 16-byte boundary selects the kernel's scalar instantiations (no other test reaches them): there, as on
    the aligned layout, the sparse path, the dense path and the run that skips no dormant splat leave the same bits."""
    import brush_amd as ba
    runs = _layout_runs(ba, dev, sh_degree, misaligned)
    for what, _, _ in _SCALAR_CASES[1:]:
        _assert_same_bits(runs[what], runs[_SCALAR_CASES[0][0]], what + " against " + _SCALAR_CASES[0][0])


@pytest.mark.parametrize("sh_degree", [0, 2])
def test_scalar_layout_leaves_the_aligned_layouts_bits(dev, sh_degree):
    """The scalar instantiations against the vector ones, run for run (the element arithmetic is the same; what differs is which
    stores are left out)."""
    import brush_amd as ba
    a, b = _layout_runs(ba, dev, sh_degree, True), _layout_runs(ba, dev, sh_degree, False)
    for what, _, _ in _SCALAR_CASES:
        _assert_same_bits(a[what], b[what], what + ": misaligned against aligned")


def _run_masked(ba, dev, zero_fill, sc, cams, gt, steps, poison, sparse):
    """tests/test_gpu_masked_grads.py::_run with the option: the single-GPU step over a gradient scratch full of quiet NaNs."""
    from brush_amd import _ffi
    options = {"zero_grads": 1} if zero_fill else {}
    if sparse is not None:
        options["update_sparse"] = sparse
    ctx = ba.Context(dev, lib=_ffi.load_test_hooks() if poison else None, options=options)
    try:
        trainer = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=3.0, ctx=ctx, seed=1234)
        spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
        gt_t = torch.from_numpy(gt.view(np.int32)).to(dev)
        for s in range(steps):
            if poison and s > 0:
                ctx.check(ctx.lib.bh_debug_fill_train_scratch(ctx._h, 0x7FC00000))
            trainer.step(ba.SceneBatch(gt_t, util.hip_camera(ba, cams[s % len(cams)])), spl)
        ctx.sync()
        out = {"transforms": spl.transforms.clone(), "sh": spl.sh_coeffs.clone(), "opac": spl.raw_opacities.clone()}
        out.update({k: v.clone() for k, v in trainer.state.items()})
        return out, trainer.stats()
    finally:
        ctx.close()


def test_unwritten_rows_are_never_read(dev):
    """Every block on the sparse path, the gradient scratch NaN-filled in front of every step after the first: a listed row that
    K18 did not mark takes 0 without touching the gradient tensors.  Compared with the zero-filling step by the protocol and the
    factors of test_gpu_masked_grads.py::test_masked_rows_equal_zero_filled (yardstick: the zero-filling path run twice)."""
    import brush_amd as ba
    n, w, h, steps = 20000, 320, 192, 7
    sc = synth.make_scene(n, 0x51, sh_degree=0, log_scale_range=(math.log(0.02), math.log(0.2)),
                          tan_half_fov=(math.tan(math.radians(50)), math.tan(math.radians(50)) * h / w))
    gt = synth.synthetic_gt_packed(w, h)
    cams = _views(w, h, 4)
    a, sa = _run_masked(ba, dev, False, sc, cams, gt, steps, True, 256)
    b, sb = _run_masked(ba, dev, True, sc, cams, gt, steps, False, None)
    c, _ = _run_masked(ba, dev, True, sc, cams, gt, steps, False, None)
    assert 0 < sa.num_visible < n
    for k in a:
        assert bool(torch.isfinite(a[k]).all()), k
    assert abs(sa.num_visible - sb.num_visible) <= max(2, n // 2000)
    assert abs(sa.loss - sb.loss) <= 1e-5 * max(1.0, abs(sb.loss))
    cfg = ba.TrainConfig()
    lr = {"transforms": max(cfg.lr_rotation, cfg.lr_scale), "sh": cfg.lr_coeffs_dc, "opac": cfg.lr_opac}
    for k in ("transforms", "sh", "opac"):
        d_ab = (a[k] - b[k]).abs()
        d_bc = (b[k] - c[k]).abs()
        assert float(d_ab.mean()) <= 2.0 * float(d_bc.mean()) + 1e-3 * lr[k], (k, float(d_ab.mean()), float(d_bc.mean()))
        assert float((d_ab > 0.5 * lr[k]).float().mean()) <= 2.0 * float((d_bc > 0.5 * lr[k]).float().mean()) + 1e-3, k
    for k in ("m1_t", "m2_t", "m1_sh", "m2_sh", "m1_o", "m2_o", "refine_weight_norm"):
        ref = float(b[k].abs().max())
        assert float((a[k] - b[k]).abs().max()) <= 4.0 * float((b[k] - c[k]).abs().max()) + 1e-3 * ref, k
    assert float((a["vis_weight"] != b["vis_weight"]).float().mean()) <= 2e-3
    assert (a["m2_sh"].view(torch.int32) == MARK).any()   # dormant splats were skipped: the sparse path ran
