"""Seeded refine states for tests/test_gpu_refine_plan.py, built on the host only, with the premises each scene is meant to carry
asserted on the restatement (tests/refine_ref.py) by check_premises(); tests/test_refine_ref.py runs those assertions without a GPU.

Log-scales and raw opacities are drawn from palettes of a few hundred values and at most ~30000 splats are visible, so the
restatement's one-call-per-distinct-value exp / log stay cheap at every size."""
import math

import numpy as np

import refine_ref as rr

F = np.float32
BOUNDS = ((0.0, 0.0, 6.0), (4.0, 2.5, 5.0))
MAB = F(500.0)      # 100 x the largest extent
SPECIAL_MIN_N = 255


def ref_cfg(**kw):
    """TrainConfig's refine defaults, as SplatTrainer.refine hands them to the library"""
    cfg = dict(bounds_center=BOUNDS[0], bounds_extent=BOUNDS[1], max_splats=10_000_000, growth_grad_threshold=0.0025,
               growth_select_fraction=0.25, split_at_screen_size=0.5, iter=400, growth_stop_iter=15000, total_train_iters=30000,
               opac_decay=0.004)
    cfg.update(kw)
    return cfg


def _crossing(x0, value, threshold):
    """adjacent f32 (a, b = the next float above a) near x0 with value(a) <= threshold < value(b)"""
    x = np.empty(129, F)
    x[64] = F(x0)
    for k in range(64):
        x[65 + k] = np.nextafter(x[64 + k], F(np.inf))
        x[63 - k] = np.nextafter(x[64 - k], F(-np.inf))
    v = value(x)
    j = np.nonzero((v[:-1] <= threshold) & (v[1:] > threshold))[0]
    assert j.size == 1, "one crossing among the neighbours of %r" % x0
    return x[j[0]], x[j[0] + 1]


def opacity_edge():
    """(a, b): sigmoid(a) < 1/255 <= sigmoid(b), one ulp apart: a is pruned, b is kept"""
    below = np.nextafter(rr.MIN_OPACITY, F(0))
    return _crossing(-math.log(254.0), rr.sigmoid, below)


def scale_edge():
    """(a, b): expf(a) <= 500 < expf(b), one ulp apart: a is kept, b is pruned"""
    return _crossing(math.log(500.0), rr.expf, MAB)


def make_state(n, deg=0, seed=1, last="kept", kind="mixed"):
    """-> (state dict of numpy arrays, dict of the special rows).  kind: "mixed" every prune and split reason; "few_visible" fewer
    positive stage-1 weights than pruned splats; "clean" nothing prunable; "all_over" every splat visible and oversized;
    "all_prunable" every opacity at -9 and five non-finite, invisible rows.  last: the last splat is "kept", "pruned" or "split"."""
    rng = np.random.default_rng(seed * 1000003 + n)
    c = (deg + 1) ** 2
    t = np.empty((n, 10), F)
    t[:, 0:3] = rng.uniform(-3, 3, (n, 3)) + np.array(BOUNDS[0])
    t[:, 3:7] = rng.normal(size=(n, 4))
    t[:, 7:10] = rng.uniform(math.log(0.02), math.log(0.3), 257).astype(F)[rng.integers(0, 257, (n, 3))]
    ro = rng.uniform(-4, 4, 509).astype(F)[rng.integers(0, 509, n)]
    st = dict(transforms=t, sh=rng.uniform(-1, 1, (n, c, 3)).astype(F), raw_opac=ro)
    for k, lo, hi, shape in (("m1_t", -1, 1, (n, 10)), ("m2_t", 0, 1, (n, 10)), ("m1_sh", -1, 1, (n, c, 3)), ("m2_sh", 0, 1, (n,)),
                             ("m1_o", -1, 1, (n,)), ("m2_o", 0, 1, (n,))):
        st[k] = rng.uniform(lo, hi, shape).astype(F)
    p_vis = min(2.0 / 3.0, 30000.0 / n) if kind != "few_visible" else min(0.02, 30000.0 / n)
    vis = np.where(rng.uniform(size=n) < p_vis, np.floor(rng.uniform(1, 3, n)), 0.0).astype(F)
    # stage-3 weights: half of the splats above the threshold (nearly all in a small scene, where the special rows alone prune two
    # dozen: stage 3 needs want > pruned), over six decades; the rest below it; ~5 % exact duplicates
    rn = np.where(rng.uniform(size=n) < (0.5 if n >= 1000 else 0.95), 0.0025 * 10.0 ** rng.uniform(0.001, 6.2, n), 10.0 ** rng.uniform(-7, -3, n)).astype(F)
    dup = np.nonzero(rng.uniform(size=n) < 0.05)[0]
    if n > 1:
        rn[dup] = rn[rng.integers(0, n, dup.size)]
        ro[dup] = ro[rng.integers(0, n, dup.size)]
    ms = (rng.uniform(0, 0.3, n) + 0.6 * (rng.uniform(size=n) < 0.02)).astype(F)
    rows = {}
    if kind in ("mixed", "few_visible"):
        ro[rng.uniform(size=n) < min(0.03, 1000.0 / n)] = F(-7.0)
    if kind == "all_over":
        vis[:] = 1.0
        ms[:] = 0.9
    if kind == "all_prunable":
        ro[:] = F(-9.0)
    if n >= SPECIAL_MIN_N and kind in ("mixed", "few_visible", "all_prunable"):
        it = iter(rng.permutation(n - 1)[:64])      # never the last row
        take = lambda k: [int(next(it)) for _ in range(k)]   # noqa: E731
        rows["prune_scale"], rows["prune_pos"], rows["prune_sh"], rows["prune_quat"], rows["prune_opac"] = take(2), take(2), take(2), take(2), take(1)
        t[rows["prune_scale"], 8] = 12.0
        t[rows["prune_pos"], 1] = 5e4
        st["sh"][rows["prune_sh"], 0, 2] = np.inf
        t[rows["prune_quat"], 4] = np.nan
        ro[rows["prune_opac"]] = np.nan
        vis[rows["prune_sh"] + rows["prune_quat"] + rows["prune_opac"]] = 0.0     # never split, even when nothing is pruned: NaN arithmetic is not specified
    if n >= SPECIAL_MIN_N and kind in ("mixed", "few_visible"):
        oa, ob = opacity_edge()
        sa, sb = scale_edge()
        rows["opac_below"], rows["opac_at"] = take(1), take(1)
        ro[rows["opac_below"]], ro[rows["opac_at"]] = oa, ob
        vis[rows["opac_at"]] = 1.0
        rows["scale_at"], rows["scale_above"] = take(3), take(3)
        for a in range(3):
            t[rows["scale_at"][a], 7 + a], t[rows["scale_above"][a], 7 + a] = sa, sb
        rows["pos_at"], rows["pos_above"] = take(6), take(6)
        for a in range(3):
            cen = F(BOUNDS[0][a])
            for j, sign in enumerate((1.0, -1.0)):
                edge = F(cen + F(sign) * MAB)
                t[rows["pos_at"][2 * a + j], a] = edge
                t[rows["pos_above"][2 * a + j], a] = np.nextafter(edge, F(sign * np.inf))
        vis[rows["scale_at"] + rows["pos_at"]] = 0.0
        ro[rows["scale_at"] + rows["pos_at"]] = F(0.5)
        # split parents: oversized and visible, so an unconstrained plan splits each of them
        for name in ("zero_quat", "opaque", "isotropic", "needle", "over_and_high"):
            rows[name] = take(1)
        rows["over_bright"] = take(8)
        par = sum((rows[k] for k in ("zero_quat", "opaque", "isotropic", "needle", "over_and_high", "over_bright")), [])
        vis[par], ms[par] = 2.0, 0.9
        ro[par] = F(0.5)
        t[rows["zero_quat"], 3:7] = 0.0
        ro[rows["opaque"]] = 20.0                    # 1 - sigmoid = 0
        t[rows["isotropic"], 7:10] = -3.0
        t[rows["needle"], 7:10] = (-6.0, 2.0, -6.0)  # one log-scale 8 above the others
        rn[rows["over_and_high"]] = 1e20             # first in stage 3's order
        ro[rows["over_bright"]] = 8.0                # likely stage-1 picks that are oversized as well
        rows["screen_zero"] = take(1)                # max_screen_size = 0 with a positive split_at_screen_size: split by stage 3 only
        vis[rows["screen_zero"]], ms[rows["screen_zero"]], rn[rows["screen_zero"]], ro[rows["screen_zero"]] = 1.0, 0.0, 1e19, 0.5
        rows["saturated"] = take(1)                  # kept, never split: sigmoid rounds to one
        ro[rows["saturated"]], vis[rows["saturated"]] = 20.0, 0.0
    if last == "kept":
        vis[n - 1] = 0.0
        if kind != "all_prunable":
            ro[n - 1] = F(0.25)
    elif last == "pruned":
        ro[n - 1] = F(-7.0)
    elif last == "split":
        ro[n - 1], vis[n - 1], ms[n - 1] = F(0.25), 1.0, 0.9
    if kind == "all_over":
        vis[:] = 1.0
    st["refine_weight_norm"], st["vis_weight"], st["max_screen_size"] = rn, vis, ms
    return st, rows


def half_fraction(thr, pruned):
    """a growth_select_fraction whose f32 product with thr ends in .5 and exceeds pruned"""
    for m in range(pruned + 3, thr):
        f = F((m + 0.5) / thr)
        prod = F(thr) * f
        if float(prod) - math.floor(float(prod)) == 0.5:
            return float(f), int(math.floor(float(prod))) + 1
    raise AssertionError("no fraction gives a product ending in .5")


def check_premises(st, rows, p, kind="mixed", last=None):
    """what the scene is meant to contain, asserted on the default plan p = rr.plan(st, ref_cfg(), seed)"""
    n = st["raw_opac"].shape[0]
    keep, split = p["keep"], p["split"]
    if last is not None:
        assert (keep[n - 1], split[n - 1]) == {"kept": (True, False), "pruned": (False, False), "split": (True, True)}[last]
    if not rows:
        return
    if kind == "all_prunable":
        assert p["replanned"] and keep.all() and p["stats"]["num_pruned"] == 0 and p["stats"]["num_pruned_non_finite"] == 5
        return
    t, ro = st["transforms"], st["raw_opac"]
    for k in ("prune_scale", "prune_pos", "prune_sh", "prune_quat", "prune_opac", "opac_below", "scale_above", "pos_above"):
        assert not keep[rows[k]].any(), k
    for k in ("opac_at", "scale_at", "pos_at", "saturated"):
        assert keep[rows[k]].all(), k
    assert p["stats"]["num_pruned_non_finite"] == 5
    # the edges are one ulp apart
    assert np.nextafter(ro[rows["opac_below"][0]], F(np.inf)) == ro[rows["opac_at"][0]]
    for a in range(3):
        assert np.nextafter(t[rows["scale_at"][a], 7 + a], F(np.inf)) == t[rows["scale_above"][a], 7 + a]
        for j in range(2):
            at, ab = t[rows["pos_at"][2 * a + j], a], t[rows["pos_above"][2 * a + j], a]
            assert abs(F(at - F(BOUNDS[0][a]))) == MAB and abs(F(ab - F(BOUNDS[0][a]))) == np.nextafter(MAB, F(np.inf))
    for k in ("zero_quat", "opaque", "isotropic", "needle", "over_and_high", "screen_zero"):
        assert split[rows[k]].all(), k
    assert p["over"][rows["over_and_high"]].all() and not p["over"][rows["screen_zero"]].any()
    assert rr.sigmoid(ro[rows["saturated"]])[0] == F(1.0) and not split[rows["saturated"]].any()
    if kind == "mixed":
        assert 0 < p["k1"] == p["pruned"] < p["npos1"]
        assert p["stage3"][rows["screen_zero"]].all() and p["stage3"][rows["over_and_high"]].all()
        assert (p["stage1"] & p["over"]).any(), "a stage-1 pick that is oversized as well"
        assert p["stats"]["num_split_high_grad"] < p["k3"]
        w3 = p["key3"] < rr.INF
        rn = st["refine_weight_norm"][w3]
        assert rn.max() / rn.min() >= 1e6
        assert np.unique(rn).size < rn.size, "exact duplicates among the positive weights"
    else:
        assert 0 < p["k1"] == p["npos1"] < p["pruned"]
