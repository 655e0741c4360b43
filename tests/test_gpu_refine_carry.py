"""bh_refine_carry_rows (include/brush_hip_feature_train.h): any per-splat table through a pending refine plan.

1. Pinned to what refine already does, with no oracle: the splats' own SH rows through BH_CARRY_COPY and their first moments through
   BH_CARRY_ZERO_SPLIT, between plan and apply, are the new sh_coeffs and the new m1_sh bit for bit (non-finite rows included: the
   carry moves bits).
2. Random tables of 1, 19 and 256 channels against the array numpy builds from SplatTrainer.last_refine_plan by the header's rule;
   in zero-split mode both halves of a split are +0 with a clear sign bit; no row of the output is left unwritten.
3. Errors: BH_ERR_STATE before any plan and after the apply, BH_ERR_INVALID_ARG for a null pointer, 0 channels and an unknown mode.

The state is tests/test_gpu_refine.py::_setup's (restated): 20000 splats in which every prune reason and every split reason occurs."""
import math

import numpy as np
import pytest
import torch

from brush_amd import synth

pytestmark = pytest.mark.gpu
NAN_PATTERN = 0x7FC0BEEF   # a quiet NaN no carried row can hold


def _setup(dev, n=20000, deg=1, seed=0xF1):
    import brush_amd as ba
    sc = synth.make_scene(n, seed, sh_degree=deg, log_scale_range=(math.log(0.02), math.log(0.3)))
    rng = np.random.default_rng(seed)
    # make every prune reason and every split reason occur
    sc["raw_opac"][rng.choice(n, 900, replace=False)] = -7.0
    sc["transforms"][rng.choice(n, 40, replace=False), 8] = 12.0
    sc["transforms"][rng.choice(n, 30, replace=False), 1] = 5e4
    sc["sh"][rng.choice(n, 25, replace=False), 0, 2] = np.inf
    sc["transforms"][rng.choice(n, 10, replace=False), 4] = np.nan
    ctx = ba.Context(dev)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    tr = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=3.0, ctx=ctx)
    tr._init_state(spl)
    st = tr.state
    for k, lo, hi in (("m1_t", -1, 1), ("m2_t", 0, 1), ("m1_sh", -1, 1), ("m2_sh", 0, 1), ("m1_o", -1, 1), ("m2_o", 0, 1)):
        st[k].copy_(torch.from_numpy(rng.uniform(lo, hi, tuple(st[k].shape)).astype(np.float32)))
    st["refine_weight_norm"].copy_(torch.from_numpy((rng.uniform(0, 0.01, n) * (rng.uniform(size=n) < 0.5)).astype(np.float32)))
    st["vis_weight"].copy_(torch.from_numpy(np.floor(rng.uniform(0, 3, n)).astype(np.float32)))
    st["max_screen_size"].copy_(torch.from_numpy((rng.uniform(0, 0.3, n) + 0.6 * (rng.uniform(size=n) < 0.01)).astype(np.float32)))
    tr.set_bounds((0.0, 0.0, 6.0), (4.0, 2.5, 5.0))
    tr.step_count = 400
    return ba, ctx, spl, tr


class _Between:
    """Stands where SplatTrainer.refine expects its feature field: `carry` runs between bh_refine_plan and bh_refine_apply and sends
    the given tables through bh_refine_carry_rows."""

    def __init__(self, n, tables):
        self.features = torch.empty((n, 1))   # (refine checks the row count)
        self.tables, self.out = tables, {}

    def carry(self, ctx, total_splats):
        from brush_amd.host import _ptr
        self.total = int(total_splats)
        for name, (t, mode) in self.tables.items():
            rows = t.contiguous().view(t.shape[0], -1)
            out = torch.full((self.total, rows.shape[1]), float("nan"), dtype=torch.float32, device=rows.device)
            out.view(torch.int32).fill_(NAN_PATTERN)
            torch.cuda.synchronize()
            ctx.check(ctx.lib.bh_refine_carry_rows(ctx._h, _ptr(rows), _ptr(out), int(rows.shape[1]), mode))
            self.out[name] = (rows, out)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("deg", [0, 2])
def test_carry_is_what_refine_does_to_the_sh_rows_and_their_moments(dev, deg):
    from brush_amd import _ffi
    ba, ctx, spl, tr = _setup(dev, deg=deg)
    try:
        n = spl.num_splats()
        probe = _Between(n, {"sh": (spl.sh_coeffs, _ffi.CARRY_COPY), "m1_sh": (tr.state["m1_sh"], _ffi.CARRY_ZERO_SPLIT)})
        tr.feature_field = probe
        new, rs = tr.refine(400, spl, seed=1234)
        ctx.sync()
        assert rs.num_pruned > 0 and rs.num_added > 0 and probe.total == rs.total_splats == new.num_splats()
        assert torch.equal(_bits(probe.out["sh"][1]), _bits(new.sh_coeffs.view(rs.total_splats, -1)))
        assert torch.equal(_bits(probe.out["m1_sh"][1]), _bits(tr.state["m1_sh"].view(rs.total_splats, -1)))
    finally:
        ctx.close()


@pytest.mark.parametrize("ch", [1, 19, 256])
def test_carry_follows_the_plan(dev, ch):
    from brush_amd import _ffi
    ba, ctx, spl, tr = _setup(dev)
    try:
        n = spl.num_splats()
        table = np.random.default_rng(0xCA + ch).normal(0.0, 1.0, (n, ch)).astype(np.float32)
        t = torch.from_numpy(table).to(dev)
        probe = _Between(n, {"copy": (t, _ffi.CARRY_COPY), "zero": (t, _ffi.CARRY_ZERO_SPLIT)})
        tr.feature_field = probe
        new, rs = tr.refine(400, spl, seed=1234)
        ctx.sync()
        plan = {k: v.cpu().numpy().astype(np.int64) for k, v in tr.last_refine_plan.items()}
        keep, split = plan["keep"].astype(bool), plan["split"].astype(bool) & plan["keep"].astype(bool)
        n_keep, total = int(keep.sum()), rs.total_splats
        assert total == n_keep + int(split.sum()) and split.any() and not keep.all()
        for name, zero in (("copy", False), ("zero", True)):
            want = np.full((total, ch), np.nan, np.float32)
            want.view(np.uint32)[:] = NAN_PATTERN
            want[plan["new_row"][keep]] = table[keep]
            want[n_keep + plan["child_slot"][split]] = table[split]
            if zero:
                want[plan["new_row"][split]] = 0.0
                want[n_keep + plan["child_slot"][split]] = 0.0
            got = probe.out[name][1].cpu().numpy()
            assert not (got.view(np.uint32) == NAN_PATTERN).any(), "%s: rows were left unwritten" % name
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
        halves = np.concatenate([plan["new_row"][split], n_keep + plan["child_slot"][split]])
        assert not probe.out["zero"][1].cpu().numpy().view(np.uint32)[halves].any()   # +0: every bit clear, the sign too
    finally:
        ctx.close()


def test_carry_errors(dev):
    from brush_amd import _ffi
    from brush_amd.host import _ptr
    ba, ctx, spl, tr = _setup(dev, n=2000)
    try:
        n = spl.num_splats()
        t = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        out = torch.zeros((2 * n, 3), dtype=torch.float32, device=dev)
        carry = lambda *a: ctx.lib.bh_refine_carry_rows(ctx._h, *a)   # noqa: E731
        assert carry(_ptr(t), _ptr(out), 3, _ffi.CARRY_COPY) == -4 and b"bh_refine_plan" in ctx.lib.bh_last_error(ctx._h)   # BH_ERR_STATE: no plan yet
        seen = {}

        class Probe:
            features = t

            def carry(self, ctx_, total_splats):
                seen["null_in"] = carry(None, _ptr(out), 3, 0)
                seen["null_out"] = carry(_ptr(t), None, 3, 0)
                seen["zero_channels"] = carry(_ptr(t), _ptr(out), 0, 0)
                seen["too_many"] = carry(_ptr(t), _ptr(out), 4097, 0)
                seen["mode"] = carry(_ptr(t), _ptr(out), 3, 2)
                seen["ok"] = carry(_ptr(t), _ptr(out), 3, 1)
        tr.feature_field = Probe()
        tr.refine(400, spl, seed=5)
        ctx.sync()
        assert seen == dict(null_in=-1, null_out=-1, zero_channels=-1, too_many=-1, mode=-1, ok=0), seen
        assert carry(_ptr(t), _ptr(out), 3, _ffi.CARRY_COPY) == -4   # the apply consumed the plan
    finally:
        ctx.close()
