"""A float32 reference of the train step's tail — what SplatTrainer::step does behind its backward (brush-train/src/train.rs:280-381)
— composed of the C oracle's pieces exactly as oracle/trainer.py composes them: the gradients times float32(grad_scale), then
RefineRecord::gather_stats, then three AdamScaled steps (the transforms with the per-column learning-rate table at lr 1, the SH
rows with one second moment per row and the (1, 1/lr_coeffs_sh_scale) table at lr_coeffs_dc, the opacity at lr_opac).  No noise.
tests/test_update_ref.py ties it to OracleTrainer bit for bit; the GPU tests compare the fused update kernel with it.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

PARAMS = ("transforms", "sh", "opac")
MOMENTS = ("m1_t", "m2_t", "m1_sh", "m2_sh", "m1_o", "m2_o")
STATS = ("refine_weight_norm", "vis_weight", "max_screen_size")
KEYS = PARAMS + MOMENTS + STATS


def zero_state(n, sh_words):
    """The state of a trainer that has not stepped: `sh_words` = 3 * (degree + 1)^2 floats per SH row."""
    z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
    return dict(m1_t=z(n, 10), m2_t=z(n, 10), m1_sh=z(n, sh_words), m2_sh=z(n), m1_o=z(n), m2_o=z(n),
                refine_weight_norm=z(n), vis_weight=z(n), max_screen_size=z(n))


def lr_mean_at(cfg, t, median_scene_scale):
    """The means' learning rate of step t (from 1), a Python float (train.rs:328-334; oracle/trainer.py:72-73)."""
    decay = (cfg.lr_mean_end / cfg.lr_mean) ** (1.0 / cfg.total_train_iters)
    return cfg.lr_mean * decay ** (t - 1) * float(median_scene_scale)


def update_ref(bo, params, state, visible, g_transforms, g_sh, g_opac, refine_weight, screen_radius, cfg, t, grad_scale=1.0,
               median_scene_scale=1.0):
    """One step's tail.  params: dict transforms [n,10], sh [n,C,3] (or [n,3C]), opac [n]; state: the six moments and the three
    statistics (zero_state's keys); the gradients in the parameters' shapes; t: the step's number, from 1.  Nothing is modified:
    returns (new params, new state), float32 arrays of the shapes that came in."""
    f32 = lambda a: np.array(a, dtype=np.float32, order="C", copy=True)  # noqa: E731
    tr, sh, op = f32(params["transforms"]), f32(params["sh"]), f32(params["opac"])
    n = tr.shape[0]
    sh_shape = sh.shape
    sh2 = sh.reshape(n, -1)
    words = sh2.shape[1]
    st = {k: f32(state[k]) for k in MOMENTS + STATS}
    g_tr, g_s, g_o = f32(g_transforms).reshape(n, 10), f32(g_sh).reshape(n, words), f32(g_opac).reshape(n, 1)
    # data parallel over cameras: the summed gradients times 1/world first (oracle/trainer.py:67-69; a scale of 1 changes no bit)
    s = np.float32(grad_scale)
    g_tr *= s; g_s *= s; g_o *= s
    bo.lib().bo_gather_stats(bo._fp(st["refine_weight_norm"]), bo._fp(st["vis_weight"]), bo._fp(st["max_screen_size"]),
                             bo._fp(f32(refine_weight)), bo._fp(f32(visible)), bo._fp(f32(screen_radius)), n)
    lr_mean = lr_mean_at(cfg, t, median_scene_scale)
    lrs = np.array([lr_mean] * 3 + [cfg.lr_rotation] * 4 + [cfg.lr_scale] * 3, np.float32)
    bo.adam_step(tr, g_tr, st["m1_t"], st["m2_t"], 1.0, t, col_scale=lrs)
    rest = np.float32(1.0) / np.float32(cfg.lr_coeffs_sh_scale)
    sh_scale = np.array([1.0 if k // 3 == 0 else rest for k in range(words)], np.float32)
    m1_sh = st["m1_sh"].reshape(n, words)
    bo.adam_step(sh2, g_s, m1_sh, st["m2_sh"], np.float32(cfg.lr_coeffs_dc), t, col_scale=sh_scale, reduce_m2=True)
    st["m1_sh"] = m1_sh.reshape(np.shape(state["m1_sh"]))
    op2, m1_o, m2_o = op.reshape(n, 1), st["m1_o"].reshape(n, 1), st["m2_o"].reshape(n, 1)
    bo.adam_step(op2, g_o, m1_o, m2_o, np.float32(cfg.lr_opac), t)
    st["m1_o"], st["m2_o"] = m1_o.reshape(np.shape(state["m1_o"])), m2_o.reshape(np.shape(state["m2_o"]))
    return dict(transforms=tr, sh=sh2.reshape(sh_shape), opac=op2.reshape(np.shape(params["opac"]))), st


# ---- inputs at which an update kernel can go wrong (the GPU tests' generators)
# a gradient row's element mix: probabilities of (normal, tiny, large, +0.0, -0.0)
MIXES = np.array([[1.0, 0.0, 0.0, 0.0, 0.0], [0.5, 0.2, 0.0, 0.15, 0.15], [0.0, 1.0, 0.0, 0.0, 0.0], [0.4, 0.15, 0.25, 0.1, 0.1],
                   [0.0, 0.5, 0.5, 0.0, 0.0]])


def elements(rng, mix_of_row, width):
    """[rows, width] float32 gradients: row r draws each element's class from MIXES[mix_of_row[r]]."""
    n = mix_of_row.shape[0]
    u = rng.random((n, width))
    kind = (u[..., None] >= np.cumsum(MIXES[mix_of_row], axis=1)[:, None, :]).sum(-1).clip(0, 4)
    sign = np.where(rng.random((n, width)) < 0.5, -1.0, 1.0)
    normal = rng.normal(size=(n, width)) * 10.0 ** rng.integers(-6, 1, (n, width))
    tiny = sign * 10.0 ** rng.uniform(-24.0, -20.0, (n, width))
    large = sign * 10.0 ** rng.uniform(15.0, 18.0, (n, width))
    return np.select([kind == 0, kind == 1, kind == 2, kind == 3], [normal, tiny, large, 0.0], -0.0).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def first_difference(got, want):
    """None when the two float32 arrays agree bit for bit, else a line about the first word that does not."""
    g, w = bits(got).reshape(-1), bits(np.asarray(want).reshape(np.shape(got))).reshape(-1)
    bad = np.flatnonzero(g != w)
    if bad.size == 0:
        return None
    i = int(bad[0])
    return "%d of %d words differ, first at flat index %d: got %r (0x%08x), want %r (0x%08x)" % (
        bad.size, g.size, i, float(g.view(np.float32)[i]), int(g[i]) & 0xFFFFFFFF, float(w.view(np.float32)[i]), int(w[i]) & 0xFFFFFFFF)
