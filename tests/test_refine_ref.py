"""tests/refine_ref.py, the restatement tests/test_gpu_refine_plan.py judges the refine kernels by, pinned on the CPU: against the
distribution its sampler claims (exact inclusion probabilities by enumeration), against oracle/refine.py on the counting rules and the
split arithmetic, and against small plans whose answers are written out by hand.  Nothing here touches the kernels."""
import itertools
import math

import numpy as np
import pytest

from brush_amd import synth
from oracle import refine as orf

import refine_ref as rr
import refine_scenes as rs

F = np.float32


# ---- the sampler -------------------------------------------------------------------------------------------------------------
def _inclusion_exact(w, k):
    """P(i is among k successive draws without replacement, each proportional to the remaining weights), by enumeration"""
    w = [float(x) for x in w]
    p = np.zeros(len(w))
    for tup in itertools.permutations([i for i in range(len(w)) if w[i] > 0], k):
        rest, pr = sum(w), 1.0
        for i in tup:
            pr *= w[i] / rest
            rest -= w[i]
        for i in tup:
            p[i] += pr
    return p


def _inclusion_measured(w, k, stream, seeds):
    w = np.asarray(w, F)
    u = rr.hash_unit(seeds[:, None], stream, np.arange(len(w))[None, :])
    keys = rr.sample_key(np.broadcast_to(w, u.shape), u)
    order = np.argsort(keys.view(np.uint32), axis=1, kind="stable")[:, :k]
    hit = np.zeros(u.shape, bool)
    np.put_along_axis(hit, order, True, axis=1)
    return hit.mean(axis=0)


@pytest.mark.parametrize("w,k", [((1, 2, 3, 4, 0, 6), 2), ((1, 2, 3, 4, 0, 6), 1), ((5, 0, 1, 1, 0.5, 2.5, 8), 3)])
def test_sampler_has_the_distribution_of_successive_weighted_sampling(w, k):
    S = 20000
    exact = _inclusion_exact(w, k)
    assert abs(exact.sum() - k) < 1e-12
    worst = 0.0
    for stream in (1, 3):
        for name, seeds in (("consecutive", np.arange(S, dtype=np.uint64)),
                            ("strided", np.arange(S, dtype=np.uint64) * np.uint64(0x1000193) + np.uint64(12345))):
            got = _inclusion_measured(w, k, stream, seeds)
            for i, wi in enumerate(w):
                if wi == 0:
                    assert got[i] == 0.0, "a zero weight is never picked"
                    continue
                sigma = math.sqrt(exact[i] * (1.0 - exact[i]) / S)   # binomial: S independent seeds
                dev = abs(got[i] - exact[i]) / sigma
                worst = max(worst, dev)
                assert dev <= 5.0, (stream, name, i, got[i], exact[i], dev)
    print("worst sampler deviation for w=%s k=%d: %.2f sigma" % (w, k, worst))


def test_hash_unit_lies_on_its_grid_and_streams_are_uncorrelated():
    near = np.array([0, 1, 2, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 3, 2 ** 32 - 2, 2 ** 32 - 1], np.uint64)
    for seed in (0, 1, 1234, 2 ** 63, 2 ** 64 - 1):
        for stream in (1, 3):
            for i in (near, np.arange(100000, dtype=np.uint64)):
                u = rr.hash_unit(seed, stream, i)
                assert u.dtype == F and (u > 0).all() and (u < 1).all()
                k = u.astype(np.float64) * 8388608.0 - 0.5
                assert np.array_equal(k, np.floor(k)) and k.min() >= 0 and k.max() <= 8388607
    # the literal value of one draw, worked through in Python integers
    z = (7 + (5 + 1) * 0x9E3779B97F4A7C15 + 3 * 0xD1B54A32D192ED03) & (2 ** 64 - 1)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    z ^= z >> 31
    assert float(rr.hash_unit(7, 3, 5)[0]) == ((z >> 41) + 0.5) / 8388608.0
    n = 100000
    for seed in (0, 1234, 2 ** 64 - 1):
        a = rr.hash_unit(seed, 1, np.arange(n)).astype(np.float64)
        b = rr.hash_unit(seed, 3, np.arange(n)).astype(np.float64)
        r = np.corrcoef(a, b)[0, 1]
        assert abs(r) <= 5.0 / math.sqrt(n), (seed, r)
        assert abs(a.mean() - 0.5) <= 5.0 / math.sqrt(12 * n) and abs(b.mean() - 0.5) <= 5.0 / math.sqrt(12 * n)


def test_sample_key_edges():
    u = np.full(7, 0.5, F)
    w = np.array([1.0, 0.0, -0.0, -1.0, np.inf, np.nan, 2.0], F)
    k = rr.sample_key(w, u)
    assert np.isinf(k[1:6]).all() and (k[1:6] > 0).all()
    l = rr.logf(np.array([0.5], F))[0]
    assert k[0] == -l and k[6] == F(-l) / F(2.0)
    assert abs(float(l) + math.log(2.0)) < 1e-7
    assert list(rr.smallest(np.array([3, 1, np.inf, 1, 0.5], F), 3)) == [4, 1, 3]      # ties by index
    assert [rr.round_half_away(x) for x in (0.0, 0.49, 0.5, 1.5, 2.5, 2.4999, 3.5)] == [0, 0, 1, 2, 3, 2, 4]


# ---- against oracle/refine.py on the scene of tests/test_gpu_refine.py ----------------------------------------------------
def gpu_refine_scene(n=20000, deg=1, seed=0xF1):
    """The host side of test_gpu_refine._setup, draw for draw."""
    sc = synth.make_scene(n, seed, sh_degree=deg, log_scale_range=(math.log(0.02), math.log(0.3)))
    rng = np.random.default_rng(seed)
    sc["raw_opac"][rng.choice(n, 900, replace=False)] = -7.0
    sc["transforms"][rng.choice(n, 40, replace=False), 8] = 12.0
    sc["transforms"][rng.choice(n, 30, replace=False), 1] = 5e4
    sc["sh"][rng.choice(n, 25, replace=False), 0, 2] = np.inf
    sc["transforms"][rng.choice(n, 10, replace=False), 4] = np.nan
    c = (deg + 1) ** 2
    state = dict(transforms=sc["transforms"], sh=sc["sh"], raw_opac=sc["raw_opac"])
    for k, lo, hi, shape in (("m1_t", -1, 1, (n, 10)), ("m2_t", 0, 1, (n, 10)), ("m1_sh", -1, 1, (n, c, 3)), ("m2_sh", 0, 1, (n,)),
                             ("m1_o", -1, 1, (n,)), ("m2_o", 0, 1, (n,))):
        state[k] = rng.uniform(lo, hi, shape).astype(F)
    state["refine_weight_norm"] = (rng.uniform(0, 0.01, n) * (rng.uniform(size=n) < 0.5)).astype(F)
    state["vis_weight"] = np.floor(rng.uniform(0, 3, n)).astype(F)
    state["max_screen_size"] = (rng.uniform(0, 0.3, n) + 0.6 * (rng.uniform(size=n) < 0.01)).astype(F)
    return state


def default_cfg(**kw):
    cfg = dict(bounds_center=(0.0, 0.0, 6.0), bounds_extent=(4.0, 2.5, 5.0), max_splats=10_000_000, growth_grad_threshold=0.0025,
               growth_select_fraction=0.25, split_at_screen_size=0.5, iter=400, growth_stop_iter=15000, total_train_iters=30000,
               opac_decay=0.004)
    cfg.update(kw)
    return cfg


@pytest.fixture(scope="module")
def scene():
    st = gpu_refine_scene()
    for v in st.values():
        v.setflags(write=False)
    return st


@pytest.mark.parametrize("iter_,max_splats", [(400, 10_000_000), (400, 20_150), (20000, 10_000_000)])
def test_plan_counts_agree_with_the_oracle(scene, iter_, max_splats):
    cfg = default_cfg(iter=iter_, max_splats=max_splats)
    t, ro = scene["transforms"], scene["raw_opac"]
    # premise: no input within a few ulp of a prune threshold, so numpy's exp and bo_expf decide alike
    mab = rr.max_allowed_bounds(cfg)
    fin = np.isfinite(t).all(axis=1) & np.isfinite(ro)
    with np.errstate(all="ignore"):
        op = rr.sigmoid(ro[fin])
        assert (np.abs(op - rr.MIN_OPACITY) > 8 * np.spacing(rr.MIN_OPACITY)).all()
        assert (np.abs(rr.expf(t[fin, 7:10]) - mab) > 8 * np.spacing(mab)).all()
        assert (np.abs(np.abs(t[fin, 0:3] - np.array(cfg["bounds_center"], F)) - mab) > 8 * np.spacing(mab)).all()
    p = rr.plan(scene, cfg, 1234)
    mask, bad = orf.prune_mask(t, scene["sh"], ro, cfg["bounds_center"], cfg["bounds_extent"])
    assert np.array_equal(p["keep"], ~mask) and np.array_equal(p["bad"], bad)
    assert mask.sum() > 0 and bad.sum() > 0
    bc = orf.budget_counts(t.shape[0], p["keep"], scene["vis_weight"], scene["refine_weight_norm"], scene["max_screen_size"], cfg)
    s = p["stats"]
    assert s["num_pruned"] == bc["pruned"] == int(mask.sum()) and s["num_pruned_non_finite"] == int(bad.sum())
    assert np.array_equal(p["over"], bc["oversized"]) and np.array_equal(p["above"], bc["above"])
    assert p["thr"] == bc["threshold_count"]
    k1 = min(bc["pruned"], int((p["keep"] & (scene["vis_weight"] > 0)).sum()))
    assert s["num_resampled"] == k1 == int(p["stage1"].sum())
    budget = max(0, max_splats - (bc["n_keep"] + k1))
    assert s["num_split_oversized"] == min(budget, int((bc["oversized"] & ~p["stage1"]).sum())) == int(p["stage2"].sum())
    if iter_ < cfg["growth_stop_iter"]:
        assert p["want"] == bc["grow_count"]
        headroom = max(0, max_splats - (bc["n_keep"] + k1 + s["num_split_oversized"]))
        assert p["k3"] == min(max(0, bc["grow_count"] - bc["pruned"]), headroom, int(bc["above"].sum())) == int(p["stage3"].sum())
    else:
        assert p["k3"] == 0 and s["num_split_high_grad"] == 0
    assert s["num_split_high_grad"] == int((p["stage3"] & ~p["stage1"] & ~p["stage2"]).sum())
    assert s["num_added"] == int(p["split"].sum()) and s["total_splats"] == bc["n_keep"] + s["num_added"]
    assert not (p["split"] & ~p["keep"]).any()
    assert not (p["stage1"] & ~(p["keep"] & (scene["vis_weight"] > 0))).any() and not (p["stage3"] & ~bc["above"]).any()
    assert np.array_equal(p["new_row"][p["keep"]], np.arange(bc["n_keep"]))
    assert np.array_equal(p["child_slot"][p["split"]], np.arange(s["num_added"]))


@pytest.mark.parametrize("iter_,sass", [(400, 0.5), (30000, 0.5), (400, 0.0)])
def test_apply_agrees_with_the_oracle(scene, iter_, sass):
    cfg = default_cfg(iter=iter_, split_at_screen_size=sass)
    p = rr.plan(scene, cfg, 1234)
    assert p["split"].sum() > 100
    got = rr.apply(scene, p, cfg)
    ref = orf.apply({k: scene[k] for k in ("transforms", "sh", "raw_opac") + rr.MOMENTS}, p["keep"], p["split"], cfg, scene["max_screen_size"])
    n_keep = p["n_keep"]
    plain = np.ones(ref["raw_opac"].shape[0], bool)
    plain[p["new_row"][p["split"]]] = False
    plain[n_keep:] = False
    for k, r in ref.items():
        g = got[k]
        assert g.shape == r.shape and g.dtype == F, k
        assert np.allclose(g, r, rtol=2e-5, atol=2e-5), (k, float(np.abs(g - r).max()))
        if k != "raw_opac":
            assert np.array_equal(rr.bits(g[plain]), rr.bits(r[plain])), k
    for k in rr.MOMENTS:        # +0.0, not -0.0
        assert not rr.bits(got[k][~plain]).any(), k
    for k in ("refine_weight_norm", "vis_weight", "max_screen_size"):
        assert got[k].shape == (n_keep + int(p["split"].sum()),) and not rr.bits(got[k]).any()


def test_bounds_agree_with_the_oracle_and_order_signed_zeros(scene):
    for pc in (0.0, 0.8, 1.0):
        c, e = rr.bounds(pc, scene["transforms"][:, :3])
        rc, re = orf.bounds_from_pos(pc, scene["transforms"][:, :3])
        assert np.array_equal(rr.bits(c), rr.bits(np.array(rc, F))) and np.array_equal(rr.bits(e), rr.bits(np.array(re, F)))
    m = np.zeros((4, 3), F)
    m[:, 0] = (0.0, -0.0, 0.0, -0.0)            # sorted: -0 -0 +0 +0; percentile 1 -> lo = row 0, hi = row 3
    c, e = rr.bounds(1.0, m)
    assert rr.bits(c)[0] == 0 and rr.bits(e)[0] == 0       # (+0 + -0) / 2 = +0, (+0 - -0) / 2 = +0
    m[:, 0] = (-0.0, -0.0, -0.0, -0.0)
    c, e = rr.bounds(1.0, m)
    assert rr.bits(c)[0] == 0x80000000 and rr.bits(e)[0] == 0
    m[:, 1] = np.nan
    c, e = rr.bounds(0.8, m)
    assert list(c) == [0, 0, 0] and list(e) == [1, 1, 1]
    m[:, 1] = (np.inf, 3.0, -np.inf, np.nan)    # one finite value on the axis
    m[:, 2] = (-5.0, -1.0, -3.0, -2.0)
    c, e = rr.bounds(0.5, m)                    # axis 2, n = 4: lo = int(0.25 * 4) = 1, hi = int(0.75 * 4) = 3 -> -3, -1
    assert (c[1], e[1], c[2], e[2]) == (3.0, 0.0, -2.0, 1.0)
    k = rr.total_order_key(np.array([-np.inf, -1.0, -0.0, 0.0, 1e-45, 2.0, np.nan], F))
    assert list(np.argsort(k, kind="stable")) == [1, 2, 3, 4, 5, 0, 6] and k[0] == k[6] == 0xFFFFFFFF
    assert np.array_equal(rr.bits(rr.from_total_order_key(k[1:6])), rr.bits(np.array([-1.0, -0.0, 0.0, 1e-45, 2.0], F)))


# ---- small plans, answers by hand ------------------------------------------------------------------------------------------
def _tiny(n, raw_opac, vis, rn, ms):
    t = np.zeros((n, 10), F)
    t[:, 0:3] = np.arange(n * 3, dtype=F).reshape(n, 3) * F(0.01)
    t[:, 2] += F(6.0)
    t[:, 3] = 1.0
    t[:, 7:10] = -3.0
    return dict(transforms=t, sh=np.zeros((n, 1, 3), F), raw_opac=np.asarray(raw_opac, F), vis_weight=np.asarray(vis, F),
                refine_weight_norm=np.asarray(rn, F), max_screen_size=np.asarray(ms, F))


def _flags(n, rows):
    f = np.zeros(n, bool)
    f[list(rows)] = True
    return f


def test_hand_plan_rounding_and_headroom():
    """10 kept, visible splats, every one above the gradient threshold, weights a decade apart: thr * fraction = 10 * 0.25 = 2.5,
    which rounds half away from zero to 3; nothing pruned, so k3 = 3 and the three largest weights (rows 9, 8, 7) are drawn."""
    n = 10
    rn = [0.01 * 10.0 ** i for i in range(n)]
    st = _tiny(n, [0.0] * n, [1.0] * n, rn, [0.0] * n)
    cfg = default_cfg()
    p = rr.plan(st, cfg, 5)
    assert list(rr.smallest(p["key3"], 4)) == [9, 8, 7, 6], "premise: a decade between weights outweighs -log u at this seed"
    assert p["thr"] == 10 and p["want"] == 3 and p["k1"] == 0 and p["k3"] == 3
    assert np.array_equal(p["keep"], np.ones(n, bool)) and np.array_equal(p["split"], _flags(n, (7, 8, 9)))
    assert list(p["new_row"]) == list(range(10)) and list(p["child_slot"]) == [0, 0, 0, 0, 0, 0, 0, 0, 1, 2]
    assert p["stats"] == dict(num_added=3, num_split_oversized=0, num_split_high_grad=3, num_pruned=0, num_pruned_non_finite=0,
                              total_splats=13, num_resampled=0)
    # headroom: max_splats = 12 leaves room for two
    p = rr.plan(st, default_cfg(max_splats=12), 5)
    assert p["want"] == 3 and p["headroom"] == 2 and p["k3"] == 2
    assert np.array_equal(p["split"], _flags(n, (8, 9)))
    assert p["stats"] == dict(num_added=2, num_split_oversized=0, num_split_high_grad=2, num_pruned=0, num_pruned_non_finite=0,
                              total_splats=12, num_resampled=0)
    # max_splats below what is kept: nothing grows, nothing is dropped
    p = rr.plan(st, default_cfg(max_splats=4), 5)
    assert p["k3"] == 0 and not p["split"].any() and p["stats"]["total_splats"] == 10
    # growth stopped
    p = rr.plan(st, default_cfg(iter=15000), 5)
    assert p["k3"] == 0 and not p["split"].any()
    # 2.4999 rounds down
    p = rr.plan(st, default_cfg(growth_select_fraction=0.24999), 5)
    assert p["want"] == 2 and np.array_equal(p["split"], _flags(n, (8, 9)))


def _hand_scene_12():
    """Row 11 is pruned (opacity), row 10 is invisible.  Row 0 has opacity 1, the other visible rows 0.0041: stage 1 (k1 = 1 pruned)
    takes row 0.  Oversized: rows 0 2 3 5 6 8; row 0 is already split, so the candidates are 2 3 5 6 8 in index order.  Above the
    gradient threshold: rows 1 2 3 4 5 7 8 9 (thr = 8), weights 1e6 (row 3), 1e3 (row 4), 1 (row 5), 0.01 (the rest)."""
    n = 12
    raw = [20.0] + [-5.5] * 10 + [-9.0]
    vis = [1.0] * 10 + [0.0, 1.0]
    rn = [0.0, 0.01, 0.01, 1e6, 1e3, 1.0, 0.0, 0.01, 0.01, 0.01, 5.0, 5.0]
    ms = [0.9, 0.1, 0.9, 0.9, 0.1, 0.9, 0.9, 0.5, 0.9, 0.1, 0.9, 0.9]      # 0.5 is not > 0.5
    return n, _tiny(n, raw, vis, rn, ms)


def test_hand_plan_budget_cuts_stage_two():
    n, st = _hand_scene_12()
    p = rr.plan(st, default_cfg(max_splats=15, growth_select_fraction=0.5), 9)
    assert int(rr.smallest(p["key1"], 1)[0]) == 0, "premise: opacity 1 against 0.0041 outweighs -log u at this seed"
    assert p["n_keep"] == 11 and p["k1"] == 1 and p["budget_over"] == 3 and p["total_over"] == 5 and p["n_over"] == 3
    assert p["want"] == 4 and p["headroom"] == 0 and p["k3"] == 0
    assert np.array_equal(p["keep"], ~_flags(n, (11,))) and np.array_equal(p["split"], _flags(n, (0, 2, 3, 5)))
    assert list(p["new_row"]) == list(range(12)) and list(p["child_slot"]) == [0, 1, 1, 2, 3, 3, 4, 4, 4, 4, 4, 4]
    assert p["stats"] == dict(num_added=4, num_split_oversized=3, num_split_high_grad=0, num_pruned=1, num_pruned_non_finite=0,
                              total_splats=15, num_resampled=1)


def test_hand_plan_stage_three_picks_what_stage_two_split():
    n, st = _hand_scene_12()
    p = rr.plan(st, default_cfg(max_splats=100, growth_select_fraction=0.5), 9)
    assert int(rr.smallest(p["key1"], 1)[0]) == 0
    assert list(rr.smallest(p["key3"], 4))[:3] == [3, 4, 5], "premise: three decades between weights outweigh -log u at this seed"
    assert p["thr"] == 8 and p["want"] == 4 and p["pruned"] == 1 and p["k3"] == 3 and p["n_over"] == 5
    assert np.array_equal(p["stage2"], _flags(n, (2, 3, 5, 6, 8))) and np.array_equal(p["stage3"], _flags(n, (3, 4, 5)))
    assert np.array_equal(p["split"], _flags(n, (0, 2, 3, 4, 5, 6, 8)))
    assert list(p["child_slot"]) == [0, 1, 1, 2, 3, 4, 5, 6, 6, 7, 7, 7]
    assert p["stats"] == dict(num_added=7, num_split_oversized=5, num_split_high_grad=1, num_pruned=1, num_pruned_non_finite=0,
                              total_splats=18, num_resampled=1)
    # the children follow in ascending parent order; both halves of a split carry +0 moments
    full = dict(st)
    rng = np.random.default_rng(3)
    for k, shape in (("m1_t", (n, 10)), ("m2_t", (n, 10)), ("m1_sh", (n, 1, 3)), ("m2_sh", (n,)), ("m1_o", (n,)), ("m2_o", (n,))):
        full[k] = rng.uniform(0.5, 1, shape).astype(F)
    out = rr.apply(full, p, default_cfg(max_splats=100, growth_select_fraction=0.5))
    assert out["transforms"].shape == (18, 10)
    parents = [0, 2, 3, 4, 5, 6, 8]
    for slot, i in enumerate(parents):
        mid = (out["transforms"][i, 0:3].astype(np.float64) + out["transforms"][11 + slot, 0:3]) / 2
        assert np.allclose(mid, st["transforms"][i, 0:3], atol=1e-6)      # the two halves straddle the old mean
        assert not out["m1_t"][i].any() and not out["m2_o"][11 + slot].any()
    assert out["m1_o"][1] == full["m1_o"][1] and out["m2_sh"][10] == full["m2_sh"][10]


def test_hand_plan_replans_when_nothing_would_be_kept():
    """Every opacity at -9: prune_points refuses to create an empty splat (train.rs:866-869), so nothing is pruned; the poisoned row
    is still counted as non-finite (train.rs:524-535) and sampling runs on the unpruned set with k1 = 0."""
    n = 8
    st = _tiny(n, [-9.0] * n, [1.0] * n, [0.01 * 10.0 ** i for i in range(n)], [0.0] * n)
    st["transforms"][2, 4] = np.nan
    p = rr.plan(st, default_cfg(), 1)
    assert p["replanned"] and p["keep"].all() and p["k1"] == 0 and p["thr"] == 8 and p["want"] == 2 and p["k3"] == 2
    assert list(rr.smallest(p["key3"], 2)) == [7, 6]
    assert p["stats"] == dict(num_added=2, num_split_oversized=0, num_split_high_grad=2, num_pruned=0, num_pruned_non_finite=1,
                              total_splats=10, num_resampled=0)
    q = rr.plan(st, default_cfg(), 1, skip_replan=True)
    assert not q["keep"].any() and q["stats"]["total_splats"] == 0


# ---- the scenes of tests/test_gpu_refine_plan.py carry what they are meant to carry -------------------------------------------
@pytest.mark.parametrize("n,kind,last", [(255, "mixed", "kept"), (256, "mixed", "pruned"), (257, "mixed", "split"), (4097, "mixed", "split"),
                                         (20000, "mixed", "kept"), (4097, "few_visible", "kept"), (4097, "all_prunable", "kept")])
def test_gpu_scene_premises(n, kind, last):
    st, rows = rs.make_state(n, kind=kind, last=last)
    p = rr.plan(st, rs.ref_cfg(), 1234)
    rs.check_premises(st, rows, p, kind, last)
    assert rows
    oa, ob = rs.opacity_edge()
    assert rr.sigmoid(np.array([oa, ob], F))[0] < rr.MIN_OPACITY <= rr.sigmoid(np.array([oa, ob], F))[1] and np.nextafter(oa, F(np.inf)) == ob
    sa, sb = rs.scale_edge()
    assert rr.expf(np.array([sa, sb], F))[0] <= rs.MAB < rr.expf(np.array([sa, sb], F))[1] and np.nextafter(sa, F(np.inf)) == sb
    if kind == "all_prunable":
        return
    # the split parents the apply kernel's clamps and boundary paths need
    t = st["transforms"]
    assert not t[rows["zero_quat"][0], 3:7].any() and st["raw_opac"][rows["opaque"][0]] == 20.0
    assert st["max_screen_size"][rows["screen_zero"][0]] == 0.0
    assert np.unique(t[rows["isotropic"][0], 7:10]).size == 1 and t[rows["needle"][0], 8] - t[rows["needle"][0], 7] == 8.0
    out = rr.apply(st, p, rs.ref_cfg())
    assert np.isfinite(out["raw_opac"]).all() and np.isfinite(out["transforms"]).all()
