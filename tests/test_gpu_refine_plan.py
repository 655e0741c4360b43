"""bh_refine_plan / bh_refine_apply / bh_splat_bounds against tests/refine_ref.py, bit for bit: which splats each stage samples
(hash_unit, sample_key, the two argsorts of float bit patterns, the mark kernels), the scans and control scalars behind the plan, the
split arithmetic and the opacity decay of the apply kernel, the zeroed RefineRecord and the percentile bounds.  Floats are compared
through their uint32 views, so the sign of zero and NaN payloads count.  Nothing of the expected side is taken from the library.

The sizes sit at the seams of the plan's building blocks (64-lane ballots, 256-thread blocks, 4096-element scan tiles and sort
blocks, sort groups of 32 blocks, the scan spine beyond 1024 tiles) and run in descending order on one context, so every plan finds
the scratch slot, the sort tables and the control block as a longer plan left them.  The scenes and the premises they carry are in
tests/refine_scenes.py (asserted there on the restatement, and again here for the case at hand)."""
import numpy as np
import pytest
import torch

import refine_ref as rr
import refine_scenes as rs

pytestmark = pytest.mark.gpu

F = np.float32
OUT = (("transforms", "transforms"), ("sh", "sh"), ("raw_opac", "raw_opac")) + tuple((k, k) for k in rr.MOMENTS) + \
    tuple((k, k) for k in ("refine_weight_norm", "vis_weight", "max_screen_size"))


@pytest.fixture(scope="module")
def ctx(dev):
    import brush_amd as ba
    c = ba.Context(dev)
    yield c
    c.close()


def _refine(dev, ctx, st, seed, iter_=400, **cfg_kw):
    """one SplatTrainer.refine of the state st on ctx -> what the library produced, as host arrays"""
    import brush_amd as ba
    own = lambda a: a if a.flags.writeable else a.copy()   # noqa: E731  (torch wants writable arrays; a shared scene is read-only)
    spl = ba.Splats(own(st["transforms"]), own(st["sh"]), own(st["raw_opac"]), device=dev)
    tr = ba.SplatTrainer(ba.TrainConfig(**cfg_kw), median_scene_scale=3.0, ctx=ctx)
    tr._init_state(spl)
    for k in rr.MOMENTS + ("refine_weight_norm", "vis_weight", "max_screen_size"):
        tr.state[k].copy_(torch.from_numpy(own(st[k])))
    tr.set_bounds(*rs.BOUNDS)
    tr.step_count = 400
    new, stats = tr.refine(iter_, spl, seed=seed)
    got = dict(transforms=new.transforms, sh=new.sh_coeffs, raw_opac=new.raw_opacities, **tr.state)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    plan = {k: v.cpu().numpy() for k, v in tr.last_refine_plan.items()}
    c = tr.config
    cfg = rs.ref_cfg(max_splats=c.max_splats, growth_grad_threshold=c.growth_grad_threshold, growth_select_fraction=c.growth_select_fraction,
                     split_at_screen_size=c.split_at_screen_size, iter=iter_, growth_stop_iter=min(c.growth_stop_iter, c.total_train_iters),
                     total_train_iters=c.total_train_iters, opac_decay=c.opac_decay)
    return got, plan, stats, tr.bounds, cfg


def _check(label, st, seed, cfg, got, plan, stats, bounds, p=None):
    """every integer and every float of one refine against the restatement; -> (its plan, its output)"""
    p = p if p is not None else rr.plan(st, cfg, seed)
    keep, split = p["keep"], p["split"]
    assert plan["keep"].dtype == np.int32 and np.array_equal(plan["keep"], keep.astype(np.int32)), label
    assert np.array_equal(plan["split"], split.astype(np.int32)), label
    assert np.array_equal(plan["new_row"][keep], p["new_row"][keep].astype(np.int32)), label
    assert np.array_equal(plan["child_slot"][split], p["child_slot"][split].astype(np.int32)), label
    assert {k: getattr(stats, k) for k in rr.STATS} == p["stats"], label
    out = rr.apply(st, p, cfg)
    for gk, rk in OUT:
        g, r = got[gk], out[rk]
        assert g.shape == r.shape and g.dtype == F, (label, gk)
        same = rr.bits(g) == rr.bits(r)
        assert same.all(), (label, gk, int((~same).sum()), np.argwhere(~same)[:4].tolist(), g[~same][:4], r[~same][:4])
    c, e = rr.bounds(0.8, out["transforms"][:, 0:3])
    assert np.array_equal(rr.bits(np.array(bounds[0], F)), rr.bits(c)) and np.array_equal(rr.bits(np.array(bounds[1], F)), rr.bits(e)), label
    print("%s: n %d -> %d, plan flags, 7 stats, %d tensors and the bounds bit-equal  %s" % (label, keep.size, p["stats"]["total_splats"], len(OUT), p["stats"]))
    return p, out


SIZES = [(1025 * 4096 + 3, "pruned"), (1025 * 4096 + 3, "split")] + \
    [(n, last) for n in (32 * 4096 + 1, 20000, 2 * 4096 + 1, 4097, 4096, 4095, 257, 256, 255) for last in ("kept", "pruned", "split")] + \
    [(65, "kept"), (64, "split"), (63, "pruned"), (1, "kept"), (257, "split")]


@pytest.mark.parametrize("n,last", SIZES, ids=["%d-%s-%d" % (n, last, i) for i, (n, last) in enumerate(SIZES)])
def test_sizes_in_descending_order_on_one_context(dev, ctx, n, last):
    st, rows = rs.make_state(n, last=last)
    got, plan, stats, bounds, cfg = _refine(dev, ctx, st, 1234)
    p = rr.plan(st, cfg, 1234)
    rs.check_premises(st, rows, p, "mixed", last)
    _check("n=%d last=%s" % (n, last), st, 1234, cfg, got, plan, stats, bounds, p)


@pytest.fixture(scope="module")
def base():
    """the mixed scene the plans below vary, with its default plan"""
    st, rows = rs.make_state(4097, seed=2, last="split")
    for v in st.values():
        v.setflags(write=False)
    p = rr.plan(st, rs.ref_cfg(), 1234)
    rs.check_premises(st, rows, p, "mixed", "split")
    return st, rows, p


@pytest.mark.parametrize("which", ["zero", "n_keep", "n_keep+k1", "n_keep+k1+3", "n_keep+k1+n_over+2", "below_kept"])
def test_max_splats_at_every_budget_boundary(dev, ctx, base, which):
    st, rows, b = base
    assert b["total_over"] > 3
    max_splats = {"zero": 0, "n_keep": b["n_keep"], "n_keep+k1": b["n_keep"] + b["k1"], "n_keep+k1+3": b["n_keep"] + b["k1"] + 3,
                  "n_keep+k1+n_over+2": b["n_keep"] + b["k1"] + b["total_over"] + 2, "below_kept": b["n_keep"] // 2}[which]
    got, plan, stats, bounds, cfg = _refine(dev, ctx, st, 1234, max_splats=max_splats)
    p, _ = _check("max_splats=%s" % which, st, 1234, cfg, got, plan, stats, bounds)
    want = {"zero": (0, 0), "n_keep": (0, 0), "n_keep+k1": (0, 0), "n_keep+k1+3": (3, 0), "n_keep+k1+n_over+2": (b["total_over"], 2), "below_kept": (0, 0)}[which]
    assert (p["n_over"], p["k3"]) == want and p["k1"] == b["k1"] > 0     # stage 1 always refills the pruned budget
    if which == "n_keep+k1+3":      # the budget cuts stage 2 after its third candidate in index order
        cand = np.nonzero(b["over"] & ~b["stage1"])[0]
        assert np.array_equal(np.nonzero(p["stage2"])[0], cand[:3]) and cand.size > 3


@pytest.mark.parametrize("seed", [0, 1234, 2 ** 64 - 1])
def test_seeds(dev, ctx, base, seed):
    st, rows, b = base
    got, plan, stats, bounds, cfg = _refine(dev, ctx, st, seed)
    p, _ = _check("seed=%d" % seed, st, seed, cfg, got, plan, stats, bounds)
    if seed != 1234:
        assert not np.array_equal(p["stage1"], b["stage1"]) and not np.array_equal(p["stage3"], b["stage3"])


def test_growth_stopped(dev, ctx, base):
    st, rows, b = base
    got, plan, stats, bounds, cfg = _refine(dev, ctx, st, 1234, iter_=15000)
    p, _ = _check("iter>=growth_stop_iter", st, 1234, cfg, got, plan, stats, bounds)
    assert p["k3"] == 0 and p["stats"]["num_split_high_grad"] == 0 and p["n_over"] > 0 and b["k3"] > 0
    assert not p["split"][rows["screen_zero"]].any()


def test_no_screen_size_splits(dev, ctx, base):
    st, rows, b = base
    got, plan, stats, bounds, cfg = _refine(dev, ctx, st, 1234, split_at_screen_size=0.0)
    p, _ = _check("split_at_screen_size=0", st, 1234, cfg, got, plan, stats, bounds)
    assert p["n_over"] == 0 and not p["over"].any() and p["k3"] > 0 and p["split"][rows["screen_zero"]].all()   # k_max = 1/sqrt(2) for every split


def test_want_ending_in_one_half(dev, ctx, base):
    st, rows, b = base
    frac, want = rs.half_fraction(b["thr"], b["pruned"])
    got, plan, stats, bounds, cfg = _refine(dev, ctx, st, 1234, growth_select_fraction=frac)
    p, _ = _check("want=%d-0.5 rounds up" % want, st, 1234, cfg, got, plan, stats, bounds)
    prod = F(b["thr"]) * F(frac)
    assert float(prod) == want - 0.5 and p["want"] == want and p["k3"] == want - b["pruned"]


def test_upper_clamp_of_the_decay(dev, ctx, base):
    """opac_decay = 0 at iter >= total_train_iters: nothing is subtracted, so only the clamp to [1e-12, 1 - 1e-12] acts, and
    1 - 1e-12 is 1.0f.  The restatement says: raw = 20 has sigmoid 1.0f, 1 / (1 - 1) = +inf and logf(+inf) = +inf, as in the reference
    (train.rs:812-816); the kept, unsplit row `saturated` comes out as +inf."""
    st, rows, b = base
    got, plan, stats, bounds, cfg = _refine(dev, ctx, st, 1234, iter_=30000, opac_decay=0.0)
    assert rr.minus_opac(cfg) == 0.0
    p, out = _check("opac_decay=0", st, 1234, cfg, got, plan, stats, bounds)
    assert out["raw_opac"][p["new_row"][rows["saturated"][0]]] == np.inf
    assert np.isfinite(out["raw_opac"]).sum() == out["raw_opac"].size - 1


def test_fewer_positive_weights_than_pruned(dev, ctx):
    st, rows = rs.make_state(4097, seed=3, kind="few_visible")
    got, plan, stats, bounds, cfg = _refine(dev, ctx, st, 1234)
    p = rr.plan(st, cfg, 1234)
    rs.check_premises(st, rows, p, "few_visible", "kept")
    _check("k1 == #positive < pruned", st, 1234, cfg, got, plan, stats, bounds, p)


def test_nothing_pruned_and_nothing_split(dev, ctx):
    st, rows = rs.make_state(4097, seed=4, kind="clean")
    got, plan, stats, bounds, cfg = _refine(dev, ctx, st, 1234, iter_=15000, split_at_screen_size=0.0)
    p, out = _check("nothing to do", st, 1234, cfg, got, plan, stats, bounds)
    assert p["keep"].all() and not p["split"].any() and p["stats"]["total_splats"] == 4097
    for k in ("transforms", "sh") + rr.MOMENTS:        # plain copies; raw_opac alone goes through the decay
        assert np.array_equal(rr.bits(got[k]), rr.bits(st[k])), k


def test_every_visible_splat_oversized(dev, ctx):
    st, rows = rs.make_state(4097, seed=5, kind="all_over", last="split")
    got, plan, stats, bounds, cfg = _refine(dev, ctx, st, 1234)
    p, _ = _check("all oversized", st, 1234, cfg, got, plan, stats, bounds)
    assert p["split"].all() and p["stats"]["total_splats"] == 2 * p["n_keep"] == 2 * 4097 and p["stats"]["num_split_high_grad"] == 0 < p["k3"]


def test_every_splat_prunable_then_a_plain_refine(dev, ctx, base):
    """All opacities at -9: the plan would keep nothing, so it runs again without pruning (train.rs:866-869).  num_pruned is 0, the
    rows poisoned with NaN / inf still count as non-finite, and sampling runs on the unpruned set.  The plain refine that follows
    finds the context as the re-plan left it."""
    st, rows = rs.make_state(4097, seed=6, kind="all_prunable")
    got, plan, stats, bounds, cfg = _refine(dev, ctx, st, 1234)
    p = rr.plan(st, cfg, 1234)
    rs.check_premises(st, rows, p, "all_prunable", "kept")
    assert p["stats"]["num_pruned"] == 0 and p["stats"]["num_pruned_non_finite"] == 5 and p["stats"]["num_added"] > 0 and p["k1"] == 0
    _check("every splat prunable", st, 1234, cfg, got, plan, stats, bounds, p)
    st2, _, _ = base
    got, plan, stats, bounds, cfg = _refine(dev, ctx, st2, 1234)
    _check("plain refine after the re-plan", st2, 1234, cfg, got, plan, stats, bounds)


@pytest.mark.parametrize("deg", [3, 4])
def test_wide_sh_rows(dev, ctx, deg):
    st, rows = rs.make_state(4097, deg=deg, seed=7, last="split")
    assert st["sh"].shape[1] * 3 == (48, 75)[deg - 3]
    got, plan, stats, bounds, cfg = _refine(dev, ctx, st, 1234)
    _check("sh degree %d" % deg, st, 1234, cfg, got, plan, stats, bounds)


# ---- bh_splat_bounds ----------------------------------------------------------------------------------------------------------
def _bounds_cases():
    rng = np.random.default_rng(11)
    cases = {}
    for n in (1, 2, 4096, 4097):
        m = rng.uniform(-5, 5, (n, 3)).astype(F)
        cases["plain-%d" % n] = m
        cases["negative-%d" % n] = (-np.abs(m) - F(1)).astype(F)
        mix = m.copy()
        pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-45, -1e-45], F)
        sel = rng.uniform(size=(n, 3)) < 0.6
        mix[sel] = pool[rng.integers(0, pool.size, int(sel.sum()))]
        mix[0, 0] = -0.0 if n > 1 else 0.0
        cases["mixed-%d" % n] = mix
        zeros = np.where(rng.uniform(size=(n, 3)) < 0.5, F(0.0), F(-0.0)).astype(F)
        cases["signed-zeros-%d" % n] = zeros
        dead = m.copy()
        dead[:, 1] = np.array([np.nan, np.inf, -np.inf], F)[rng.integers(0, 3, n)]
        cases["dead-axis-%d" % n] = dead
    return cases


@pytest.mark.parametrize("percentile", [0.0, 0.8, 1.0])
def test_splat_bounds_exactly(dev, ctx, percentile):
    import brush_amd as ba
    for name, m in _bounds_cases().items():
        n = m.shape[0]
        t = np.zeros((n, 10), F)
        t[:, 0:3] = m
        t[:, 3] = 1.0
        c, e = ba.splat_bounds(ba.Splats(t, np.zeros((n, 1, 3), F), np.zeros(n, F), device=dev), percentile, ctx=ctx)
        rc, re = rr.bounds(percentile, m)
        assert np.array_equal(rr.bits(np.array(c, F)), rr.bits(rc)) and np.array_equal(rr.bits(np.array(e, F)), rr.bits(re)), (name, percentile, c, e, rc, re)
        if name.startswith("dead-axis"):
            assert list(rc) == [0, 0, 0] and list(re) == [1, 1, 1]
        if name.startswith("negative"):
            assert (rc < 0).all()
    print("bounds at percentile %s: %d cases bit-equal" % (percentile, len(_bounds_cases())))
