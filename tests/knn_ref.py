"""numpy restatement of compute_knn_scales (brush-train/src/splat_init.rs:179-216), the reference tests/test_knn_init_abi.py and
tests/test_gpu_knn_init.py hold bh_knn_log_scales to, plus the seeded point clouds both use.

Contract (include/brush_hip.h, bh_knn_log_scales): d1 <= d2 are the two smallest f32 distances sqrt((dx*dx + dy*dy) + dz*dz) from
row i to rows j != i (duplicates at 0); ln(clamp((d1 + d2) / 4, 1e-3, 0.1 median_size)), median_size = max(2 * middle extent of
bounds_from_pos(0.75), 0.01); n < 3 gives 0.  A non-finite row is nobody's neighbour and a missing neighbour is at +inf."""
import numpy as np

F32 = np.float32


def sq_dist_f32(q, p):
    """(dx*dx + dy*dy) + dz*dz with every operation rounded to f32 (glam's Vec3A dot order); q [..., 3], p [..., 3] broadcast."""
    q = np.asarray(q, F32)
    p = np.asarray(p, F32)
    with np.errstate(all="ignore"):
        dx = q[..., 0] - p[..., 0]
        dy = q[..., 1] - p[..., 1]
        dz = q[..., 2] - p[..., 2]
        return (dx * dx + dy * dy) + dz * dz


def finite_rows(pos):
    return np.isfinite(np.asarray(pos, F32)).all(axis=1)


def nn2_brute(pos, queries=None, chunk=256):
    """Exact (d1, d2) [Q, 2] f32 by brute force over every finite row j != i (the rows `queries`, default all).  +inf where a
    neighbour is missing; a non-finite query row gets (+inf, +inf)."""
    pos = np.ascontiguousarray(np.asarray(pos, F32).reshape(-1, 3))
    n = pos.shape[0]
    q_idx = np.arange(n) if queries is None else np.asarray(queries, np.int64)
    fin = finite_rows(pos)
    cand = pos[fin]
    cand_idx = np.nonzero(fin)[0]
    out = np.full((q_idx.size, 2), np.inf, F32)
    if cand.shape[0] == 0:
        return out
    for a in range(0, q_idx.size, chunk):
        qi = q_idx[a:a + chunk]
        s = sq_dist_f32(pos[qi][:, None, :], cand[None, :, :])
        s[qi[:, None] == cand_idx[None, :]] = np.inf   # j != i
        s[~fin[qi]] = np.inf                           # a non-finite query has no neighbour
        k = min(2, s.shape[1])
        two = np.sort(np.partition(s, k - 1, axis=1)[:, :k], axis=1) if s.shape[1] > 2 else np.sort(s, axis=1)
        with np.errstate(all="ignore"):
            d = np.sqrt(two.astype(F32)).astype(F32)
        out[a:a + qi.size, :d.shape[1]] = d
    return out


def bounds_from_pos(pos, percentile=0.75):
    """bounds_from_pos (splat_init.rs:130-160) -> (center[3], extent[3]) f32: per-axis sorted finite values, picks at
    ((1 -+ p) / 2 * n) as usize, the unit box when an axis has no finite value."""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    p = F32(percentile)
    mn, mx = np.full(3, -1.0, F32), np.full(3, 1.0, F32)
    vals = [np.sort(pos[:, k][np.isfinite(pos[:, k])]) for k in range(3)]
    if all(v.size for v in vals):
        for k, v in enumerate(vals):
            n = v.size
            lo = int((F32(1.0) - p) / F32(2.0) * F32(n))
            hi = min(n - 1, int((F32(1.0) + p) / F32(2.0) * F32(n)))
            mn[k], mx[k] = v[lo], v[hi]
    with np.errstate(all="ignore"):
        return ((mx + mn) / F32(2.0)).astype(F32), ((mx - mn) / F32(2.0)).astype(F32)


def median_size(pos):
    """bounding_box.median_size().max(0.01) (bounding_box.rs:23-29, splat_init.rs:189)."""
    _, ext = bounds_from_pos(pos, 0.75)
    mid = np.sort(ext)[1]
    return F32(np.fmax(F32(mid * F32(2.0)), F32(0.01)))


def clamped_dist(nn, upper):
    """(d1 + d2) / 4 in f32, then f32::clamp(1e-3, upper)."""
    nn = np.asarray(nn, F32)
    with np.errstate(all="ignore"):
        dist = ((nn[:, 0] + nn[:, 1]) / F32(4.0)).astype(F32)
    dist = np.where(dist < F32(1e-3), F32(1e-3), dist)
    return np.where(dist > upper, upper, dist).astype(F32)


def log_scales(pos, nn=None):
    """compute_knn_scales' per-row value [N] f32 = float32(log(float64(clamped dist))) (the device's bh_logf is held to 2 ulp of
    it); 0 for n < 3.  nn: the (d1, d2) to use (default: the brute force)."""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    n = pos.shape[0]
    if n < 3:
        return np.zeros(n, F32)
    if nn is None:
        nn = nn2_brute(pos)
    upper = F32(median_size(pos) * F32(0.1))
    return np.log(clamped_dist(nn, upper).astype(np.float64)).astype(F32)


def ulp_diff(a, b):
    """|a - b| in units in the last place (f32, same-sign finite values; equal values incl. equal infinities give 0)."""
    a = np.asarray(a, F32).ravel()
    b = np.asarray(b, F32).ravel()
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.where(a == b, 0, np.abs(ia - ib))


# ---- seeded point clouds -------------------------------------------------------------------------------------------
def cloud(kind, n, seed=0):
    """[n, 3] f32 point clouds: uniform | surface | outliers | lattice | tripled | nonfinite | tiny."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        p = rng.uniform(-1.0, 1.0, (n, 3))
    elif kind == "surface":   # what a COLMAP cloud looks like: noisy planes and sphere shells
        k = rng.integers(0, 4, n)
        p = np.empty((n, 3))
        u, v = rng.uniform(-2.0, 2.0, n), rng.uniform(-2.0, 2.0, n)
        noise = rng.normal(0.0, 0.005, n)
        p[k == 0] = np.stack([u, v, noise], 1)[k == 0]                     # floor
        p[k == 1] = np.stack([u, np.full(n, 2.0) + noise, v], 1)[k == 1]    # wall
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        r = np.where(k == 2, 0.7, 0.3)[:, None] * (1.0 + 0.01 * rng.normal(size=(n, 1)))
        c = np.where((k == 2)[:, None], [[0.5, 0.5, 0.8]], [[-0.8, 0.3, 0.4]])
        sph = c + r * d
        p[k >= 2] = sph[k >= 2]
    elif kind == "outliers":   # a dense cluster and 1 % far outliers at 10^3 x its scale
        p = rng.normal(0.0, 0.1, (n, 3))
        m = rng.random(n) < 0.01
        p[m] = rng.uniform(-100.0, 100.0, (int(m.sum()), 3))
    elif kind == "lattice":   # integer lattice: exact ties everywhere
        side = int(np.ceil(n ** (1.0 / 3.0)))
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 3)
        p = g[rng.permutation(g.shape[0])[:n]].astype(np.float64)
    elif kind == "tripled":   # every point three times, plus a block of 100 identical points
        base = rng.uniform(-1.0, 1.0, ((n - 100) // 3, 3))
        p = np.concatenate([base, base, base, np.full((100, 3), 0.25)])
        p = np.concatenate([p, rng.uniform(-1.0, 1.0, (n - p.shape[0], 3))])[rng.permutation(n)]
    elif kind == "nonfinite":   # rows of NaN / +-inf sprinkled in
        p = rng.uniform(-1.0, 1.0, (n, 3))
        bad = rng.choice(n, max(3, n // 50), replace=False)
        vals = np.array([np.nan, np.inf, -np.inf])
        p[bad, rng.integers(0, 3, bad.size)] = vals[rng.integers(0, 3, bad.size)]
    elif kind == "tiny":   # everything inside a 1e-4 box: median_size floors at 0.01, distances hit the lower clamp
        p = 0.5 + rng.uniform(0.0, 1e-4, (n, 3))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(p.astype(F32))


KINDS = ("uniform", "surface", "outliers", "lattice", "tripled", "nonfinite", "tiny")


def points_ply(pos, rgb=None, extra_float=()):
    """A COLMAP-style point cloud PLY: float x y z [+ uchar red green blue] [+ float extras], binary little endian, no scale_*."""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    n = pos.shape[0]
    fields = [("x", "float", "<f4"), ("y", "float", "<f4"), ("z", "float", "<f4")]
    if rgb is not None:
        fields += [("red", "uchar", "u1"), ("green", "uchar", "u1"), ("blue", "uchar", "u1")]
    fields += [(nm, "float", "<f4") for nm in extra_float]
    rec = np.zeros(n, np.dtype([(nm, dt) for nm, _, dt in fields]))
    for k, nm in enumerate("xyz"):
        rec[nm] = pos[:, k]
    if rgb is not None:
        rgb = np.asarray(rgb, np.uint8).reshape(n, 3)
        for k, nm in enumerate(("red", "green", "blue")):
            rec[nm] = rgb[:, k]
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % n] + ["property %s %s" % (ty, nm) for nm, ty, _ in fields] + ["end_header"]
    return ("\n".join(head) + "\n").encode() + rec.tobytes()
