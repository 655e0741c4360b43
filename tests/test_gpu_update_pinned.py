"""train_update_kernel (optim.hip) — the one launch that applies every parameter change of every training step — against
tests/update_ref.py, the oracle's own composition of the step's tail (tests/test_update_ref.py ties it to OracleTrainer).

The lever is bh_grad_hook: with a hook set, bh_train_step hands over the step's exchange buffer
    visible[N] | v_transforms[10N] | v_sh[3CN] | v_raw_opac[N] | refine_weight[N]      (each section padded to 4 floats)
behind the backward and in front of the update launch.  brush_amd.host._view of that buffer is writable, so a hook can REPLACE
what the scene rendered — flags, all three gradients, and the refine weight that lies behind `sum_count` — with values of the
test's choosing: the step becomes a deterministic function of them.  screen_radius is not in the buffer; it comes from a
stand-alone forward of the same parameters and camera (bit exact against the oracle, tests/test_gpu_render.py), on a context of
its own so that the trainer's context sees nothing but its steps.

Ordering: every Context here is the default one (ctx.uses_torch_stream): the library's kernels and torch's copies run on the SAME
stream, so the copy a hook queues lies between the backward and the update.  The tests rely on that and assert it; nothing
synchronises inside a hook.

Part A — injected inputs, bit for bit against update_ref after each of 5 steps (parameters, six moments, three statistics).
  rows, interleaved with period 6 so that the float4s of the transforms (10 floats a row) and of the SH rows straddle classes:
    0 a gradient at every step, visible 1        3 every gradient word -0.0, visible 1
    1 never a gradient, visible 0                4 a gradient at every step, visible 2.0 (a sum over ranks)
    2 a gradient at steps 1 and 4 only           5 a gradient at every step, visible 3.0
  elements of a gradient row, by the row's mix: normal * 10^[-6..0]; tiny, 1e-24 .. 1e-20 (the square is subnormal or 0); large,
    1e15 .. 1e18 (squares up to 1e36, a 75-word row's sum below FLT_MAX); exact +0.0 and -0.0
  refine_weight: 0, tiny (1e-30 .. 1e-20), and uniform(0, 2) * 10^[-3..0] — above and below the running maximum as it grows
  cases (n, SH degree, option update_rows, _world, m1_t rebound to a pointer 4 mod 16 after step 1) -> the (ROWS, VEC) they run:
    (257, 0, unset, 1, no)  (256, vec)  short      (1025, 3, unset, 1, no)  (64, vec)   long
    (300, 1, unset, 2, yes) (256, scalar) short    (300, 4, unset, 3, yes)  (64, scalar) long
    (63, 0, 64, 3, no)      (64, vec)   short      (257, 4, 128, 1, no)     (128, vec)  long
    (1025, 1, 64, 1, yes)   (64, scalar) short     (300, 3, 128, 2, yes)    (128, scalar) long
    (300, 0, 128, 2, no)    (128, vec)  short      (300, 4, 256, 1, no)     (256, vec)  long: 85 KB of LDS, opted in by the launcher
    (257, 1, 128, 1, yes)   (128, scalar) short    (257, 3, 256, 1, yes)    (256, scalar) long
    (1, 2, unset, 1, no)    (128, vec)             (1025, 4, 256, 2, yes)   (256, scalar) long, several blocks
    (63, 2, unset, 3, yes)  (128, scalar)          (1, 0, unset, 1, yes)    (256, scalar)
Part B — the masked, dormant and sparse paths, which a hook cannot reach (a hook means zero-filled gradients), tied to the same
  reference on the deterministic one-tile problem of test_gpu_update_sparse.py: a run with a capturing identity hook equals the
  replay of what it captured through update_ref at every step, and the default run, update_sparse = 256 and zero_grads = 1 equal it.
Part C — the noise drawn inside the update launch equals the stand-alone noise kernel on injected samples bit for bit, and both
  the float64 gate of oracle/trainer.py within the float32 formula's own error."""
import numpy as np
import pytest
import torch

from brush_amd import synth
import update_ref as ur
import util
from test_gpu_update_sparse import MARK, _misalign_m1_t, _scene, _views

gpu = pytest.mark.gpu   # (per test: the table check of part A needs no GPU)

W = H = 16
MEDIAN = 3.0
STATE_KEYS = ur.MOMENTS + ur.STATS


def _pad4(x):
    return (x + 3) & ~3


def _offsets(n, words):
    """Section starts of the exchange buffer (include/brush_hip.h, bh_grad_hook) and its length."""
    o_tr = _pad4(n)
    o_sh = o_tr + _pad4(n * 10)
    o_op = o_sh + _pad4(n * words)
    o_ref = o_op + _pad4(n)
    return o_tr, o_sh, o_op, o_ref, o_ref + _pad4(n)


def _pack(n, words, vis, g_tr, g_sh, g_op, refine):
    o_tr, o_sh, o_op, o_ref, total = _offsets(n, words)
    buf = np.zeros(total, np.float32)
    buf[:n] = vis
    buf[o_tr:o_tr + n * 10] = g_tr.reshape(-1)
    buf[o_sh:o_sh + n * words] = g_sh.reshape(-1)
    buf[o_op:o_op + n] = g_op.reshape(-1)
    buf[o_ref:o_ref + n] = refine
    return buf


def _unpack(buf, n, words):
    o_tr, o_sh, o_op, o_ref, _ = _offsets(n, words)
    return dict(vis=buf[:n], g_tr=buf[o_tr:o_tr + n * 10].reshape(n, 10), g_sh=buf[o_sh:o_sh + n * words].reshape(n, words),
                g_op=buf[o_op:o_op + n], refine=buf[o_ref:o_ref + n])


def _hook_into(tr, fn, world=1):
    """Routes tr's steps through bh_grad_hook: fn(the whole buffer as a writable device tensor) runs between backward and update."""
    from brush_amd import _ffi
    from brush_amd.host import _view
    errors = []

    def hook(_user, ptr, count):
        try:
            n, words = tr._pin_n, tr._pin_words
            total = _offsets(n, words)[4]
            assert int(count) == _offsets(n, words)[3], (int(count), n, words)   # data parallel over cameras: everything before refine_weight
            fn(_view(ptr, (total,), torch.float32, torch.device("cuda", torch.cuda.current_device())))
            return 0
        except Exception as e:  # never unwind across the C boundary
            errors.append(e)
            return 1
    tr._hook = _ffi.GRAD_HOOK(hook)
    tr._world = world
    tr.pg = object()   # (only its presence matters: the step takes the hook above, partition "cameras")
    tr.sparse_exchange = False
    tr._pin_errors = errors


def _download(spl, tr):
    out = {k: v.detach().cpu().numpy().copy() for k, v in (("transforms", spl.transforms), ("sh", spl.sh_coeffs), ("opac", spl.raw_opacities))}
    if tr.state is None:   # a trainer that has not stepped
        out.update(ur.zero_state(out["opac"].shape[0], out["sh"][0].size))
    else:
        out.update({k: tr.state[k].detach().cpu().numpy().copy() for k in STATE_KEYS})
    return out


def _split(full):
    return {k: full[k] for k in ur.PARAMS}, {k: full[k] for k in STATE_KEYS}


def _assert_bits(got, want, what, keys=ur.KEYS):
    for k in keys:
        d = ur.first_difference(got[k], want[k])
        assert d is None, (what, k, d)


def _screen_radius(ba, fctx, spl, cam):
    """max_radius of a stand-alone forward of the splats as they are now."""
    _, aux = ba.render_splats(spl, cam, (W, H), (0.0, 0.0, 0.0), ctx=fctx)
    return aux.max_radius.cpu().numpy().copy()


# ---------------------------------------------------------------------------------------------------------------------------
# Part A
# ---------------------------------------------------------------------------------------------------------------------------
STEPS_A = 5


def _inputs_a(n, words, step, seed):
    """The buffer's content of step `step` (from 1): a function of (seed, step, row, element)."""
    rng = np.random.default_rng([seed, step])
    cls = (np.arange(n) % 6)
    mix = (np.arange(n) + seed) % len(ur.MIXES)   # a row keeps its mix over the steps; period 5 against the classes' 6: every pair occurs
    g_tr, g_sh, g_op = ur.elements(rng, mix, 10), ur.elements(rng, mix, words), ur.elements(rng, mix, 1)
    has = np.isin(cls, (0, 4, 5)) | ((cls == 2) & (step in (1, 4)))
    neg0 = cls == 3
    for g in (g_tr, g_sh, g_op):
        g[~has & ~neg0] = 0.0
        g[neg0] = -0.0
    vis = np.select([cls == 4, cls == 5, has | neg0], [2.0, 3.0, 1.0], 0.0).astype(np.float32)
    kind = rng.integers(0, 4, n)
    refine = np.select([kind == 0, kind == 1], [0.0, 10.0 ** rng.uniform(-30.0, -20.0, n)],
                       rng.uniform(0.0, 2.0, n) * 10.0 ** rng.integers(-3, 1, n)).astype(np.float32)
    return dict(vis=vis, g_tr=g_tr, g_sh=g_sh, g_op=g_op.reshape(n), refine=refine)


CASES_A = [
    (257, 0, None, 1, False), (300, 1, None, 2, True), (63, 0, 64, 3, False), (1025, 1, 64, 1, True), (300, 0, 128, 2, False),
    (257, 1, 128, 1, True), (1025, 3, None, 1, False), (300, 4, None, 3, True), (257, 4, 128, 1, False), (300, 3, 128, 2, True),
    (300, 4, 256, 1, False), (257, 3, 256, 1, True), (1, 2, None, 1, False), (1025, 4, 256, 2, True), (63, 2, None, 3, True),
    (1, 0, None, 1, True),
]


def test_the_cases_cover_every_value_and_instantiation():
    """The module docstring's promise, checked: every value of every parameter occurs, every (ROWS, VEC) pair runs at a short SH row
    (degree 0 or 1) and at a long one (degree 3 or 4)."""
    assert {c[0] for c in CASES_A} == {1, 63, 257, 300, 1025} and {c[1] for c in CASES_A} == {0, 1, 2, 3, 4}
    assert {c[2] for c in CASES_A} == {None, 64, 128, 256} and {c[3] for c in CASES_A} == {1, 2, 3}
    default_rows = {0: 256, 1: 256, 2: 128, 3: 64, 4: 64}   # launch_train_update
    reached = {(c[2] or default_rows[c[1]], not c[4], "short" if c[1] <= 1 else "long") for c in CASES_A if c[1] != 2}
    assert reached == {(r, v, s) for r in (64, 128, 256) for v in (True, False) for s in ("short", "long")}


@gpu
@pytest.mark.parametrize("n,sh_degree,rows,world,misalign", CASES_A)
def test_injected_step_equals_the_reference_bit_for_bit(dev, oracle_lib, n, sh_degree, rows, world, misalign):
    import brush_amd as ba
    words = 3 * (sh_degree + 1) ** 2
    sc = _scene(n, sh_degree)
    cfg = ba.TrainConfig(mean_noise_weight=0.0)
    ctx, fctx = ba.Context(dev), ba.Context(dev)
    try:
        assert ctx.uses_torch_stream and fctx.uses_torch_stream   # the hook's copy is ordered by the stream (module docstring)
        if rows is not None:
            ctx.set_option("update_rows", rows)
        gt = torch.from_numpy(synth.synthetic_gt_packed(W, H).view(np.int32)).to(dev)
        cam = util.hip_camera(ba, synth.default_camera_params(W, H))
        spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
        tr = ba.SplatTrainer(cfg, median_scene_scale=MEDIAN, ctx=ctx)
        tr._pin_n, tr._pin_words = n, words
        payload = {}
        _hook_into(tr, lambda buf: buf.copy_(payload["now"]), world)
        params = dict(transforms=sc["transforms"].copy(), sh=sc["sh"].copy(), opac=sc["raw_opac"].copy())
        state = ur.zero_state(n, words)
        state["m1_sh"] = state["m1_sh"].reshape(sc["sh"].shape)
        for t in range(1, STEPS_A + 1):
            x = _inputs_a(n, words, t, 0xA11 + n * 7 + sh_degree)
            radius = _screen_radius(ba, fctx, spl, cam)
            payload["now"] = torch.from_numpy(_pack(n, words, x["vis"], x["g_tr"], x["g_sh"], x["g_op"], x["refine"])).to(dev)
            tr.step(ba.SceneBatch(gt, cam), spl)
            ctx.sync()
            assert not tr._pin_errors, tr._pin_errors
            params, state = ur.update_ref(oracle_lib, params, state, x["vis"], x["g_tr"], x["g_sh"], x["g_op"], x["refine"], radius,
                                          cfg, t, 1.0 / world, MEDIAN)
            got = _download(spl, tr)
            _assert_bits(got, dict(params, **state), "step %d" % t)
            if misalign and t == 1:
                _misalign_m1_t(tr.state)
        # the run was not trivially zero: parameters moved, moments grew, the -0.0 rows left no mark on the values
        assert all(np.isfinite(got[k]).all() for k in ur.KEYS)
        assert n == 1 or (float(np.abs(got["transforms"] - sc["transforms"]).max()) > 0 and float(got["m2_t"].max()) > 0)
    finally:
        ctx.close()
        fctx.close()


@gpu
def test_update_rows_256_at_sh_degree_4_opts_in_to_its_lds(dev):
    """launch_train_update asks for (256 * 76 + 4 * 256 + 4 + 768) * 4 bytes there, above the 64 KB a kernel gets without asking:
    the launcher raises the instantiation's limit once per context — with the fused noise too (the 768 words), which part A's
    cases (mean_noise_weight 0) do not stage.  The step must run and move the means of visible, faint splats."""
    import brush_amd as ba
    n, sh_degree = 300, 4
    sc = _scene(n, sh_degree)
    sc["raw_opac"][:] = np.float32(-4.0)
    ctx = ba.Context(dev, options={"update_rows": 256})
    try:
        gt = torch.from_numpy(synth.synthetic_gt_packed(W, H).view(np.int32)).to(dev)
        spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
        tr = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=MEDIAN, ctx=ctx, seed=5)
        for _ in range(2):
            tr.step(ba.SceneBatch(gt, util.hip_camera(ba, synth.default_camera_params(W, H))), spl)
        ctx.sync()
        vis = tr.state["vis_weight"].cpu().numpy() > 0
        moved = np.abs(spl.transforms.cpu().numpy()[:, :3] - sc["transforms"][:, :3]).max(1) > 0
        assert vis.any() and moved[vis].all() and not moved[~vis].any()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------
# Part B
# ---------------------------------------------------------------------------------------------------------------------------
STEPS_B = 9
_RUN_H = {}


def _train_b(ba, dev, n, sh_degree, options, capture=None, fctx=None, per_step=None):
    """STEPS_B steps of the one-tile problem (seeded trainer: jittered background; no mean noise), as
    test_gpu_update_sparse.py::_train.  capture: a list that receives each step's exchange buffer (the run then goes through an
    identity hook); per_step(t, camera, splats, trainer) runs in front of / behind each step (see the caller)."""
    sc, cams = _scene(n, sh_degree), _views(W, H, 3)
    ctx = ba.Context(dev, options=options)
    try:
        assert ctx.uses_torch_stream
        gt = torch.from_numpy(synth.synthetic_gt_packed(W, H).view(np.int32)).to(dev)
        spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
        tr = ba.SplatTrainer(ba.TrainConfig(mean_noise_weight=0.0), median_scene_scale=MEDIAN, ctx=ctx, seed=77)
        if capture is not None:
            tr._pin_n, tr._pin_words = n, 3 * (sh_degree + 1) ** 2
            _hook_into(tr, lambda buf: capture.append(buf.clone()), 1)
        for s in range(STEPS_B):
            cam = util.hip_camera(ba, cams[s % len(cams)])
            if per_step is not None:
                per_step("before", s + 1, cam, spl, tr)
            tr.step(ba.SceneBatch(gt, cam), spl)
            if per_step is not None:
                ctx.sync()
                per_step("after", s + 1, cam, spl, tr)
        ctx.sync()
        assert capture is None or not tr._pin_errors, tr._pin_errors
        return _download(spl, tr)
    finally:
        ctx.close()


def _run_h(ba, dev, oracle_lib, n, sh_degree):
    """Run H of a size, once: the capturing identity hook (zero-filled gradients, no marks, no skip), every step replayed through
    update_ref and compared with it bit for bit.  Returns H's final tensors."""
    key = (n, sh_degree)
    if key in _RUN_H:
        return _RUN_H[key]
    words = 3 * (sh_degree + 1) ** 2
    sc = _scene(n, sh_degree)
    cfg = ba.TrainConfig(mean_noise_weight=0.0)
    captured, radius = [], {}
    ref = {"params": dict(transforms=sc["transforms"].copy(), sh=sc["sh"].copy(), opac=sc["raw_opac"].copy()), "state": ur.zero_state(n, words)}
    ref["state"]["m1_sh"] = ref["state"]["m1_sh"].reshape(sc["sh"].shape)
    fctx = ba.Context(dev)
    trained = []

    def per_step(when, t, cam, spl, tr):
        if when == "before":
            radius["now"] = _screen_radius(ba, fctx, spl, cam)
            return
        x = _unpack(captured[t - 1].cpu().numpy(), n, words)
        trained.append(int((np.abs(x["g_tr"]).max(1) > 0).sum()))
        ref["params"], ref["state"] = ur.update_ref(oracle_lib, ref["params"], ref["state"], x["vis"], x["g_tr"], x["g_sh"], x["g_op"],
                                                    x["refine"], radius["now"], cfg, t, 1.0, MEDIAN)
        _assert_bits(_download(spl, tr), dict(ref["params"], **ref["state"]), "run H against its replay, step %d" % t)
    try:
        out = _train_b(ba, dev, n, sh_degree, None, capture=captured, per_step=per_step)
    finally:
        fctx.close()
    assert len(captured) == STEPS_B and min(trained) > 0, trained   # every step's backward reached some splat
    assert not (out["m2_sh"].view(np.int32) == MARK).any()          # no marks where nothing is masked
    _RUN_H[key] = out
    return out


@gpu
@pytest.mark.parametrize("n,sh_degree", [(6000, 0), (6000, 2), (1500, 3), (300, 1)])
def test_masked_dormant_and_sparse_paths_equal_the_replayed_reference(dev, oracle_lib, n, sh_degree):
    """Run H equals update_ref's replay of its own captured buffers at every step (_run_h); the library's default run D (row-marked
    gradients, dormant skip, default update_sparse), run S (update_sparse = 256) and run Z (zero_grads = 1) equal H: parameters,
    five moment tensors and the statistics bit for bit, m2_sh by value, and in D and S the -0.0 marks of m2_sh say exactly "every
    moment of this splat is zero".  Many splats are dormant, some are trained — else the paths were not exercised (measured:
    47 % of the 6000 splats dormant, 34 % of the 1500, 35 % of the 300)."""
    import brush_amd as ba
    h = _run_h(ba, dev, oracle_lib, n, sh_degree)
    runs = {"D": _train_b(ba, dev, n, sh_degree, None), "S": _train_b(ba, dev, n, sh_degree, {"update_sparse": 256}),
            "Z": _train_b(ba, dev, n, sh_degree, {"zero_grads": 1})}
    exact = tuple(k for k in ur.KEYS if k != "m2_sh")
    for name, r in runs.items():
        _assert_bits(r, h, "run %s against run H" % name, exact)
        assert np.array_equal(r["m2_sh"], h["m2_sh"]), (name, "m2_sh by value")
    zero = (np.abs(h["m1_t"]).sum(1) == 0) & (np.abs(h["m2_t"]).sum(1) == 0) & (np.abs(h["m1_sh"].reshape(n, -1)).sum(1) == 0) & \
        (h["m1_o"] == 0) & (h["m2_o"] == 0) & (h["m2_sh"] == 0)
    for name in ("D", "S"):
        marks = runs[name]["m2_sh"].view(np.int32) == MARK
        assert np.array_equal(marks, zero), (name, "the mark must say exactly: every moment of this splat is zero")
    assert not (runs["Z"]["m2_sh"].view(np.int32) == MARK).any()
    share = float(zero.mean())
    print("dormant share %.3f, trained rows %d of %d" % (share, int((np.abs(h["m2_t"]).sum(1) > 0).sum()), n))
    assert 0.25 < share < 1.0, share
    assert float((np.abs(h["m2_t"]).sum(1) > 0).mean()) > 0.02


# ---------------------------------------------------------------------------------------------------------------------------
# Part C
# ---------------------------------------------------------------------------------------------------------------------------
STEPS_C = 3
N_C = 300
SEED_C = 0xC0FFEE


def _gate32(raw_opac):
    """mean_noise_gate's formula (device_rng.h) in numpy float32, without the visibility factor."""
    x = (np.float32(1.0) - np.float32(1.0) / (np.float32(1.0) + np.exp(-raw_opac.astype(np.float32)))).astype(np.float32)
    x2 = x * x; x4 = x2 * x2; x8 = x4 * x4; x16 = x8 * x8; x32 = x16 * x16; x64 = x32 * x32; x128 = x64 * x64
    return np.clip(x128 * x16 * x4 * x2, np.float32(0.0), np.float32(1.0))


def _gate64(raw_opac):
    """oracle/trainer.py:85-86 in float64, without the visibility factor."""
    sig = 1.0 / (1.0 + np.exp(-raw_opac.astype(np.float64)))
    return np.clip((1.0 - sig) ** 150, 0, 1)


GATE_FLOOR = 1e-30   # below it the noise (gate * lr_mean * 50 * N(0,1), lr_mean 6e-5) is far under half an ulp of any mean of the scene


def _gate_rel_error(raw_opac):
    """The largest relative error of the float32 formula against the float64 gate over these opacities (gate64 >= GATE_FLOOR)."""
    g64 = _gate64(raw_opac)
    ok = g64 >= GATE_FLOOR
    assert ok.any()
    return float((np.abs(_gate32(raw_opac)[ok].astype(np.float64) - g64[ok]) / g64[ok]).max())


def _inputs_c(n, words, step):
    rng = np.random.default_rng([0xC, step])
    mix = np.zeros(n, np.int64)   # normal * 10^[-6..0] everywhere
    vis = rng.integers(0, 3, n).astype(np.float32)
    return dict(vis=vis, g_tr=ur.elements(rng, mix, 10), g_sh=ur.elements(rng, mix, words), g_op=ur.elements(rng, mix, 1).reshape(n),
                refine=rng.uniform(0.0, 1.0, n).astype(np.float32))


def _run_c(ba, dev, sh_degree, injected, check=None):
    n, words = N_C, 3 * (sh_degree + 1) ** 2
    sc = _scene(n, sh_degree)
    sc["raw_opac"] = np.linspace(-6.0, 6.0, n).astype(np.float32)[np.random.default_rng(3).permutation(n)]
    ctx, fctx = ba.Context(dev), ba.Context(dev)
    try:
        assert ctx.uses_torch_stream
        gt = torch.from_numpy(synth.synthetic_gt_packed(W, H).view(np.int32)).to(dev)
        cam = util.hip_camera(ba, synth.default_camera_params(W, H))
        spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
        tr = ba.SplatTrainer(ba.TrainConfig(), median_scene_scale=MEDIAN, ctx=ctx, seed=SEED_C)
        tr._pin_n, tr._pin_words = n, words
        payload = {}
        _hook_into(tr, lambda buf: buf.copy_(payload["now"]), 1)
        outs = []
        for t in range(1, STEPS_C + 1):
            x = _inputs_c(n, words, t)
            before = _download(spl, tr)
            radius = _screen_radius(ba, fctx, spl, cam) if check is not None else None
            payload["now"] = torch.from_numpy(_pack(n, words, x["vis"], x["g_tr"], x["g_sh"], x["g_op"], x["refine"])).to(dev)
            samples = tr.normal_samples(n, t, dev)
            if injected:   # the stand-alone mean_noise_kernel behind the update, on the samples the seeded step draws
                tr.step(ba.SceneBatch(gt, cam), spl, background=tr.sample_background(), noise_samples=samples)
            else:          # noise_fused: drawn inside the update launch
                tr.step(ba.SceneBatch(gt, cam), spl)
            ctx.sync()
            assert not tr._pin_errors, tr._pin_errors
            outs.append(_download(spl, tr))
            if check is not None:
                check(t, x, before, outs[-1], radius, samples.cpu().numpy())
        return outs
    finally:
        ctx.close()
        fctx.close()


@gpu
@pytest.mark.parametrize("sh_degree", [0, 2])
def test_fused_noise_equals_injected_samples_and_the_float64_gate(dev, oracle_lib, sh_degree):
    """With injected gradients a seeded step is deterministic: the noise drawn inside the update launch must equal, bit for bit and
    in every tensor, the same step with bh_normal_samples' tensor injected (the stand-alone noise kernel on the updated opacity).
    Against the reference, per step from the kernel's own previous state: everything but the means equals update_ref bit for bit;
    rows with visible == 0 carry exactly update_ref's means; for the others, means - update_ref's means is compared with
    clip(samples * gate64 * min(visible, 1) * float32(lr_mean * weight), +-median), gate64 = (1 - sigmoid(opacity))^150 in float64
    of the UPDATED opacity.  Bound per element: 4 x E x |expected| + one float32 ulp of the mean (the final add), E = the largest
    relative error of the device formula evaluated in numpy float32 against gate64 over the step's own opacities (where gate64 >=
    1e-30; below it the noise is under 1e-32).  Measured over the initial opacities (linspace(-6, 6, 300), 137 of them above the floor):
    E = 8.7e-6, at opacity -1.5, so the bound is 3.5e-5 of the expected noise — x^150 multiplies a relative error of x by 150, and
    the device's exp is another polynomial than numpy's, hence the factor 4.  A wrong sample, gate, scale or visibility clamp moves
    a row by the whole noise."""
    import brush_amd as ba
    n, words = N_C, 3 * (sh_degree + 1) ** 2
    cfg = ba.TrainConfig()
    worst = {"E": 0.0, "ratio": 0.0, "noised": 0}

    def check(t, x, before, after, radius, samples):
        bp, bs = _split(before)
        rp, rs = ur.update_ref(oracle_lib, bp, bs, x["vis"], x["g_tr"], x["g_sh"], x["g_op"], x["refine"], radius, cfg, t, 1.0, MEDIAN)
        want = dict(rp, **rs)
        _assert_bits(after, want, "step %d" % t, tuple(k for k in ur.KEYS if k != "transforms"))
        assert ur.first_difference(after["transforms"][:, 3:], want["transforms"][:, 3:]) is None
        unseen = x["vis"] == 0
        assert unseen.any() and (~unseen).any()
        assert ur.first_difference(after["transforms"][unseen, :3], want["transforms"][unseen, :3]) is None
        E = _gate_rel_error(want["opac"])
        scale = np.float32(ur.lr_mean_at(cfg, t, MEDIAN) * cfg.mean_noise_weight)
        w64 = _gate64(want["opac"]) * np.minimum(x["vis"], 1.0)
        expected = np.clip(samples.astype(np.float64) * w64[:, None] * np.float64(scale), -MEDIAN, MEDIAN)
        got = after["transforms"][:, :3].astype(np.float64) - want["transforms"][:, :3].astype(np.float64)
        bound = 4.0 * E * np.abs(expected) + np.spacing(np.abs(after["transforms"][:, :3])).astype(np.float64)
        err = np.abs(got - expected)
        worst["E"], worst["ratio"] = max(worst["E"], E), max(worst["ratio"], float((err / bound).max()))
        worst["noised"] += int((np.abs(got).max(1) > 0.1 * float(scale)).sum())
        print("step %d: E %.3g, worst error / bound %.3g" % (t, E, float((err / bound).max())))
        assert (err <= bound).all(), (t, int((err > bound).sum()), float((err / bound).max()))

    fused = _run_c(ba, dev, sh_degree, False, check)
    inj = _run_c(ba, dev, sh_degree, True)
    for t in range(STEPS_C):
        _assert_bits(fused[t], inj[t], "fused noise against injected samples, step %d" % (t + 1))
    assert worst["noised"] > 20, worst   # the gate let noise through for the faint, visible rows
