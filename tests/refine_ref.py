"""numpy restatement of the whole of refine (brush_amd/csrc/refine.hip, DESIGN.md refine section) that tests/test_refine_ref.py
pins on the CPU and tests/test_gpu_refine_plan.py holds bh_refine_plan / bh_refine_apply / bh_splat_bounds to, bit for bit.

Every operation is an f32 operation in the order the kernels write it (numpy rounds each one; no contraction).  exp / log are taken
only through bo_expf / bo_logf of the oracle library, the restatements of the device's bh_expf / bh_logf.  Nothing here is taken
from the code under test: the sampling keys, the two stable sorts, the scans and the control scalars are all computed from the
inputs.  Reference lines: brush-train/src/train.rs:431-663 (refine), :665-822 (refine_splats), :848-893 (prune_points),
multinomial.rs, splat_init.rs:130-160 (bounds_from_pos)."""
import numpy as np

F = np.float32
U32 = np.uint32
U64 = np.uint64
INF = F(np.inf)
MIN_OPACITY = F(1.0) / F(255.0)                 # train.rs:32
FRAC_1_SQRT_2 = F(0.70710678118654752440)
STATS = ("num_added", "num_split_oversized", "num_split_high_grad", "num_pruned", "num_pruned_non_finite", "total_splats", "num_resampled")
MOMENTS = ("m1_t", "m2_t", "m1_sh", "m2_sh", "m1_o", "m2_o")


def _per_distinct(name, x):
    """bo_<name> (oracle/brush_oracle.cpp, = the device's bh_<name>) of every element, one call per distinct bit pattern."""
    from oracle import bo
    x = np.ascontiguousarray(x, F)
    u, inv = np.unique(x.view(U32), return_inverse=True)
    f = getattr(bo.lib(), name)
    vals = np.array([f(float(v)) for v in u.view(F)], F)
    return vals[inv.reshape(-1)].reshape(x.shape)


def expf(x):
    return _per_distinct("bo_expf", x)


def logf(x):
    return _per_distinct("bo_logf", x)


def is_finite(x):
    return ((np.ascontiguousarray(x, F).view(U32) >> U32(23)) & U32(0xFF)) != U32(0xFF)


def sigmoid(x):
    with np.errstate(all="ignore"):
        return (F(1) / (F(1) + expf(-np.asarray(x, F))).astype(F)).astype(F)


def inv_sigmoid(x):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        return logf((x / (F(1) - x).astype(F)).astype(F))


def clampf(x, lo, hi):
    """fminf(fmaxf(x, lo), hi): a NaN comes out as lo"""
    return np.fmin(np.fmax(np.asarray(x, F), F(lo)), F(hi)).astype(F)


def hash_unit(seed, stream, i):
    """u of (seed, stream, i): SplitMix-style mixing in wrapping uint64; the top 23 bits k give (k + 0.5) * 2^-23, exact in f32."""
    i = np.atleast_1d(np.asarray(i)).astype(U64)
    s = seed.astype(U64) if isinstance(seed, np.ndarray) else np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], U64)   # arrays broadcast against i
    st = np.array([int(stream)], U64)
    with np.errstate(over="ignore"):
        z = s + (i + U64(1)) * U64(0x9E3779B97F4A7C15) + st * U64(0xD1B54A32D192ED03)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        z = z ^ (z >> U64(31))
    k = (z >> U64(41)).astype(U32)
    return ((k.astype(F) + F(0.5)).astype(F) * F(1.0 / 8388608.0)).astype(F)


def sample_key(w, u):
    """the exponential clock -logf(u) / w (one f32 division); +inf unless w is positive and finite (multinomial.rs:8-14)"""
    w, u = np.asarray(w, F), np.asarray(u, F)
    with np.errstate(all="ignore"):
        ok = (w > F(0)) & is_finite(w)
    key = np.full(w.shape, INF, F)
    if ok.any():
        with np.errstate(all="ignore"):
            key[ok] = ((-logf(u[ok])).astype(F) / w[ok]).astype(F)
    return key


def smallest(keys, k):
    """the indices of the k smallest keys: order by unsigned bit pattern, ties by index (a stable sort)"""
    order = np.argsort(np.ascontiguousarray(keys, F).view(U32), kind="stable")
    return order[:k]


def round_half_away(x):
    """f32::round of a non-negative f32 -> int"""
    x = F(x)
    fl = np.floor(x)
    return int(fl) + (1 if F(x - fl) >= F(0.5) else 0)


def _excl(flags):
    c = np.cumsum(flags.astype(np.int64))
    return (c - flags).astype(np.int64)


def max_allowed_bounds(cfg):
    e = [F(x) for x in cfg["bounds_extent"]]
    return F(max(max(e[0], e[1]), e[2]) * F(100.0))   # train.rs:485


def classify(state, cfg, seed, no_prune=False):
    """refine_classify_kernel: per-splat keep flag, the two sampling keys, the flags the stages read"""
    t = np.asarray(state["transforms"], F).reshape(-1, 10)
    n = t.shape[0]
    sh = np.asarray(state["sh"], F).reshape(n, -1)
    ro = np.asarray(state["raw_opac"], F).reshape(n)
    mab = max_allowed_bounds(cfg)
    c = [F(x) for x in cfg["bounds_center"]]
    with np.errstate(all="ignore"):
        bad = (~is_finite(t)).any(axis=1) | (~is_finite(sh)).any(axis=1) | ~is_finite(ro)
        opac = sigmoid(ro)
        alpha_low = opac < MIN_OPACITY                                              # train.rs:493
        scale_big = (expf(t[:, 7:10]) > mab).any(axis=1)
        oob = np.zeros(n, bool)
        for a in range(3):
            oob |= np.abs((t[:, a] - c[a]).astype(F)) > mab
        prune = (alpha_low | scale_big | oob | bad) & (not no_prune)
        keep = ~prune
        vis = np.asarray(state["vis_weight"], F) > F(0)                              # stats.rs:52-54
        rn = np.asarray(state["refine_weight_norm"], F)
        above = (rn > F(cfg["growth_grad_threshold"])) & vis                         # stats.rs:23-28
        w1 = np.where(keep & vis, opac, F(0)).astype(F)                              # train.rs:530-533
        w3 = np.where(keep & above, rn, F(0)).astype(F)                              # train.rs:613
        idx = np.arange(n, dtype=np.uint64)
        key1 = sample_key(w1, hash_unit(seed, 1, idx))
        key3 = sample_key(w3, hash_unit(seed, 3, idx))
        sass = F(cfg["split_at_screen_size"])
        over = keep & vis & (np.asarray(state["max_screen_size"], F) > sass) & bool(sass > F(0))   # stats.rs:32-37
    return dict(keep=keep, bad=bad, key1=key1, key3=key3, over=over, thr=keep & above, opac=opac, w1=w1, w3=w3)


def plan(state, cfg, seed, skip_replan=False):
    """bh_refine_plan -> dict: keep / split (bool [n]), new_row / child_slot (int64 [n], the exclusive scans), stats (dict of the
    seven RefineStats fields) and the intermediate scalars and stage sets (k1, k3, want, stage1, stage2, stage3, ...).
    cfg["growth_stop_iter"] is already the host's min(growth_stop_iter, total_train_iters)."""
    n = np.asarray(state["transforms"]).reshape(-1, 10).shape[0]
    c = classify(state, cfg, seed)
    replanned = False
    if int(c["keep"].sum()) == 0 and not skip_replan:   # prune_points: "Trying to create empty splat!" (train.rs:866-869)
        c = classify(state, cfg, seed, no_prune=True)
        replanned = True
    keep = c["keep"]
    max_splats = int(cfg["max_splats"])
    n_keep = int(keep.sum())
    pruned = n - n_keep
    npos1 = int((c["key1"] < INF).sum())
    npos3 = int((c["key3"] < INF).sum())
    thr = int(c["thr"].sum())
    k1 = min(pruned, npos1)                              # always refill the pruned budget (train.rs:527-540)
    budget_over = max(0, max_splats - (n_keep + k1))     # train.rs:572-576 (saturating)
    split = np.zeros(n, bool)
    stage1 = np.zeros(n, bool)
    stage1[smallest(c["key1"], k1)] = True
    split |= stage1
    cand = c["over"] & ~split                            # train.rs:577-585: index order until the budget runs out
    stage2 = cand & (_excl(cand) < budget_over)
    split |= stage2
    total_over = int(cand.sum())
    n_over = min(total_over, budget_over)
    k3, want, headroom = 0, 0, 0
    if int(cfg["iter"]) < int(cfg["growth_stop_iter"]):  # train.rs:589-623
        want = round_half_away(F(thr) * F(cfg["growth_select_fraction"]))
        headroom = max(0, max_splats - (n_keep + k1 + n_over))
        k3 = min(max(want - pruned, 0), headroom, npos3)
    stage3 = np.zeros(n, bool)
    stage3[smallest(c["key3"], k3)] = True
    n_high_new = int((stage3 & ~split).sum())
    split |= stage3
    n_split = int(split.sum())
    stats = dict(num_added=n_split, num_split_oversized=n_over, num_split_high_grad=n_high_new, num_pruned=n - n_keep,
                 num_pruned_non_finite=int(c["bad"].sum()), total_splats=n_keep + n_split, num_resampled=k1)
    return dict(keep=keep, split=split, new_row=_excl(keep), child_slot=_excl(split), stats=stats, n_keep=n_keep, pruned=pruned,
                k1=k1, k3=k3, want=want, headroom=headroom, budget_over=budget_over, total_over=total_over, n_over=n_over,
                npos1=npos1, npos3=npos3, thr=thr, stage1=stage1, stage2=stage2, stage3=stage3, over=c["over"], above=c["thr"],
                key1=c["key1"], key3=c["key3"], bad=c["bad"], replanned=replanned)


def minus_opac(cfg):
    """train.rs:808-811"""
    train_t = min(max(F(F(cfg["iter"]) / F(cfg["total_train_iters"])), F(0)), F(1))
    return F(F(cfg["opac_decay"]) * F(F(1) - train_t))


def decay_opacity(raw, minus):
    """train.rs:812-816; 1 - 1e-12 is 1.0f: an opacity whose sigmoid rounds to one comes out as +inf"""
    with np.errstate(all="ignore"):
        return inv_sigmoid(clampf((sigmoid(raw) - F(minus)).astype(F), F(1.0e-12), F(1.0) - F(1.0e-12)))


def powf_pos(x, y):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        return np.where(x > F(0), expf((F(y) * logf(x)).astype(F)), F(0)).astype(F)


def split_rows(t, raw, max_screen, cfg):
    """refine_splats (train.rs:665-806) for the rows t [r,10], raw [r], max_screen [r] -> (parent t, parent raw, child t, child raw),
    before the opacity decay; the arithmetic of refine_apply_kernel in its order of operations"""
    t = np.asarray(t, F).reshape(-1, 10)
    raw = np.asarray(raw, F).reshape(-1)
    with np.errstate(all="ignore"):
        q = t[:, 3:7]
        ss = ((((q[:, 0] * q[:, 0]) + (q[:, 1] * q[:, 1])) + (q[:, 2] * q[:, 2])) + (q[:, 3] * q[:, 3])).astype(F)
        qn = np.fmax(np.sqrt(ss).astype(F), F(1.0e-32))
        rot = (q / qn[:, None]).astype(F)
        s = expf(t[:, 7:10])
        inv_opac = (F(1) - sigmoid(raw)).astype(F)
        new_opac = (F(1) - powf_pos(inv_opac, FRAC_1_SQRT_2)).astype(F)
        new_raw = inv_sigmoid(clampf(new_opac, MIN_OPACITY, F(1) - MIN_OPACITY))
        sq = (s * s).astype(F)
        max_sq = np.fmax(np.fmax(np.fmax(sq[:, 0], sq[:, 1]), sq[:, 2]), F(1.0e-30))
        sass = F(cfg["split_at_screen_size"])
        if sass > F(0):
            k_max = np.fmin(((F(1) / np.fmax(np.asarray(max_screen, F), F(1.0e-6))).astype(F) * sass).astype(F), FRAC_1_SQRT_2)
        else:
            k_max = np.full(t.shape[0], FRAC_1_SQRT_2, F)
        ratio = (sq / max_sq[:, None]).astype(F)
        k_axis = (-(ratio * (-k_max + F(1))[:, None]).astype(F) + F(1)).astype(F)
        off = (np.sqrt(np.fmax((-(k_axis * k_axis).astype(F) + F(1)).astype(F), F(0))).astype(F) * s).astype(F)
        new_log = (t[:, 7:10] + logf(k_axis)).astype(F)
        # quaternion_vec_multiply (quat_vec.rs:4-45)
        qw, qx, qy, qz = rot[:, 0], rot[:, 1], rot[:, 2], rot[:, 3]
        vx, vy, vz = off[:, 0], off[:, 1], off[:, 2]
        qw2, qx2, qy2, qz2 = qw * qw, qx * qx, qy * qy, qz * qz
        xy, xz, yz, wx, wy, wz = qx * qy, qx * qz, qy * qz, qw * qx, qw * qy, qw * qz
        sx = (qw2 + qx2 - qy2 - qz2) * vx + (xy * vy + xz * vz + wy * vz - wz * vy) * F(2)
        sy = (qw2 - qx2 + qy2 - qz2) * vy + (xy * vx + yz * vz + wz * vx - wx * vz) * F(2)
        sz = (qw2 - qx2 - qy2 + qz2) * vz + (xz * vx + yz * vy + wx * vy - wy * vx) * F(2)
        smp = np.stack([sx, sy, sz], axis=1).astype(F)
        child = np.concatenate([(t[:, 0:3] + smp).astype(F), rot, new_log], axis=1).astype(F)
        parent = t.copy()
        parent[:, 0:3] = t[:, 0:3] + (-smp)             # scatter-ADD of (-samples) and of the differences (train.rs:738-752)
        parent[:, 7:10] = t[:, 7:10] + (new_log - t[:, 7:10]).astype(F)
        parent_raw = (raw + (new_raw - raw).astype(F)).astype(F)
    return parent, parent_raw, child, new_raw


def apply(state, pl, cfg):
    """bh_refine_apply for the plan pl (keep, split): kept rows in index order, then the children in ascending parent order; both
    halves of a split get +0.0 moments; decay_opacity on every output row; a fresh (zero) RefineRecord."""
    keep, split = np.asarray(pl["keep"], bool), np.asarray(pl["split"], bool)
    assert not (split & ~keep).any()
    idx = np.nonzero(keep)[0]
    n_keep = idx.size
    par_old = np.nonzero(split)[0]
    r = par_old.size
    par = (np.cumsum(keep) - 1)[par_old]
    out = {}
    for k in ("transforms", "sh", "raw_opac") + MOMENTS:
        v = np.asarray(state[k], F)
        out[k] = np.concatenate([v[idx], np.zeros((r,) + v.shape[1:], F)])
    if r:
        ms = np.asarray(state["max_screen_size"], F)[par_old]
        pt, praw, ct, craw = split_rows(out["transforms"][par], out["raw_opac"][par], ms, cfg)
        out["transforms"][par] = pt
        out["raw_opac"][par] = praw
        out["transforms"][n_keep:] = ct
        out["raw_opac"][n_keep:] = craw
        out["sh"][n_keep:] = out["sh"][par]
        for k in MOMENTS:                               # train.rs:762-806
            out[k][par] = F(0)
    out["raw_opac"] = decay_opacity(out["raw_opac"], minus_opac(cfg))
    for k in ("refine_weight_norm", "vis_weight", "max_screen_size"):
        out[k] = np.zeros(n_keep + r, F)
    return out


def total_order_key(v):
    """float -> u32 whose unsigned order is f32::total_cmp order (-0.0 before +0.0); non-finite values go last"""
    v = np.ascontiguousarray(v, F)
    b = v.view(U32)
    key = np.where(b & U32(0x80000000), ~b, b | U32(0x80000000)).astype(U32)
    return np.where(is_finite(v), key, U32(0xFFFFFFFF)).astype(U32)


def from_total_order_key(k):
    k = np.asarray(k, U32)
    return np.where(k & U32(0x80000000), k & U32(0x7FFFFFFF), ~k).astype(U32).view(F)


def bounds(percentile, means):
    """bh_splat_bounds (splat_init.rs:130-160) -> (center [3] f32, extent [3] f32); index arithmetic in f32; the unit box when any
    axis has no finite value"""
    means = np.asarray(means, F).reshape(-1, 3)
    pc = F(percentile)
    mn, mx = np.full(3, -1, F), np.full(3, 1, F)
    lo_v, hi_v, ok = [], [], means.shape[0] > 0
    for a in range(3):
        keys = np.sort(total_order_key(means[:, a]))
        n = int(is_finite(means[:, a]).sum())
        if n == 0:
            ok = False
            break
        lo = int(F(F(F(1) - pc) / F(2)) * F(n))
        hi = min(int(F(F(F(1) + pc) / F(2)) * F(n)), n - 1)
        lo_v.append(from_total_order_key(keys[min(lo, n - 1)]))
        hi_v.append(from_total_order_key(keys[hi]))
    if ok:
        mn, mx = np.array(lo_v, F).reshape(3), np.array(hi_v, F).reshape(3)
    with np.errstate(all="ignore"):
        return ((mx + mn) / F(2)).astype(F), ((mx - mn) / F(2)).astype(F)   # BoundingBox::from_min_max (bounding_box.rs:8-13)


def bits(x):
    """the uint32 view of an f32 array: equality on it counts the sign of zero and NaN payloads"""
    return np.ascontiguousarray(x, F).view(U32)
