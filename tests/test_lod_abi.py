"""LOD decimation (brush-train/src/lod.rs) without a GPU: the four C-ABI entry points are declared, bound and exported,
lod_target_count follows train_stream.rs:261 in f32, and this file's numpy f32 restatements of the accumulate and of
log_det_6x6 — the references tests/test_gpu_lod.py holds the device to — are sanity-checked against float64."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOD_SYMBOLS = ("bh_pup_accumulate", "bh_pup_accumulate_view", "bh_pup_scores", "bh_decimate_to_count")
# lower triangle of the 6x6 H in planes: entry (i, k), i >= k, is plane i (i + 1) / 2 + k
PLANE = {(i, k): i * (i + 1) // 2 + k for i in range(6) for k in range(i + 1)}
J_COLS = (0, 1, 2, 7, 8, 9)   # dL/dmean, dL/dlog_scale in a v_transforms row


def accumulate_f32(hessian, v_transforms):
    """lod.rs:120-126 for one view, in f32: H[e] = H[e] + (j_i * j_k) — one rounded multiply, one rounded add (in place)."""
    j = np.asarray(v_transforms, np.float32).reshape(-1, 10)[:, J_COLS]
    with np.errstate(all="ignore"):
        for (i, k), e in PLANE.items():
            outer = (j[:, i] * j[:, k]).astype(np.float32)
            hessian[e] = (hessian[e] + outer).astype(np.float32)
    return hessian


def log_det_6x6_f32(hessian):
    """log_det_6x6 (lod.rs:44-70) restated over [21, N] planes: the Cholesky in the reference's loop order, every operation an f32
    operation (numpy rounds each one), -inf at the first pivot <= 0, NaN propagated.  -> [N] f32."""
    h = np.asarray(hessian, np.float32)
    n = h.shape[1]
    m = np.zeros((6, 6, n), np.float32)
    for (i, k), e in PLANE.items():
        m[i, k] = h[e]
    lo = np.zeros((6, 6, n), np.float32)
    failed = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for j in range(6):
            s = np.zeros(n, np.float32)
            for k in range(j):
                s = (s + (lo[j, k] * lo[j, k]).astype(np.float32)).astype(np.float32)
            diag = (m[j, j] - s).astype(np.float32)
            failed |= diag <= 0.0   # (NaN <= 0 is false: a NaN pivot propagates)
            lo[j, j] = np.sqrt(diag)
            for i in range(j + 1, 6):
                s = np.zeros(n, np.float32)
                for k in range(j):
                    s = (s + (lo[i, k] * lo[j, k]).astype(np.float32)).astype(np.float32)
                lo[i, j] = ((m[i, j] - s).astype(np.float32) / lo[j, j]).astype(np.float32)
        log_det = np.zeros(n, np.float32)
        for i in range(6):
            log_det = (log_det + np.log(lo[i, i]).astype(np.float32)).astype(np.float32)
    return np.where(failed, np.float32(-np.inf), (np.float32(2.0) * log_det).astype(np.float32)).astype(np.float32)


def planes_from_matrices(mats):
    """[N, 6, 6] symmetric -> [21, N] f32 planes."""
    mats = np.asarray(mats, np.float32)
    out = np.zeros((21, mats.shape[0]), np.float32)
    for (i, k), e in PLANE.items():
        out[e] = mats[:, i, k]
    return out


def reference_order(scores):
    """sort_by(|a, b| b.partial_cmp(a).unwrap_or(Equal)) (lod.rs:20), Rust's stable sort, with NaN after -inf (the library's
    documented choice): Python's stable sort on (is NaN, -score)."""
    s = [float(x) for x in np.asarray(scores, np.float32)]
    return sorted(range(len(s)), key=lambda i: (s[i] != s[i], -s[i] if s[i] == s[i] else 0.0))


def test_header_ffi_and_library_carry_the_lod_functions():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    src = open(os.path.join(ROOT, "include", "brush_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _ffi.load()
    for name in LOD_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _ffi.SYMBOLS, name
        assert getattr(lib, name) is not None
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    for name in ("pup_accumulate", "pup_accumulate_view", "pup_scores", "decimate_to_count", "lod_target_count"):
        assert re.search(r"\b%s\(" % name, hpp), name


def test_lod_target_count_follows_the_f32_formula():
    from brush_amd import host

    def ref(n, pct):
        v = np.float32(n) * np.float32(pct)
        v = np.float32(v / np.float32(100.0))
        return int(max(v, np.float32(1.0)))
    for n in (1, 3, 7, 1000, 16_777_217, 4_000_000_000):
        for pct in (1, 50, 100):
            assert host.lod_target_count(n, pct) == ref(n, pct), (n, pct)
    assert host.lod_target_count(1, 1) == 1 and host.lod_target_count(3, 50) == 1 and host.lod_target_count(3, 100) == 3
    assert host.lod_target_count(16_777_217, 100) == 16_777_216   # n as f32 rounds to even
    assert host.lod_target_count(16_777_217, 50) == 8_388_608


def test_lod_entry_points_reject_bad_arguments_without_a_device():
    """Argument checks run before the library touches the device (a NULL context is refused outright)."""
    from brush_amd import _ffi
    lib = _ffi.load()
    assert lib.bh_pup_accumulate(None, None, 0, None, 0, None) == -1
    assert lib.bh_pup_scores(None, None, 0, None) == -1
    assert lib.bh_pup_accumulate_view(None, None, 0, 0, None, None, None, None, 0, None, None) == -1
    assert lib.bh_decimate_to_count(None, None, 0, 0, 1, None, None, None, None, None, None, None, None, None) == -1


def test_numpy_log_det_restatement_agrees_with_float64():
    rng = np.random.default_rng(5)
    n = 400
    a = rng.normal(size=(n, 6, 6))
    spd = a @ a.transpose(0, 2, 1) + 6.0 * np.eye(6)   # well conditioned
    spd *= np.exp(rng.uniform(-6, 6, size=(n, 1, 1)))
    got = log_det_6x6_f32(planes_from_matrices(spd))
    sign, want = np.linalg.slogdet(planes_to64(planes_from_matrices(spd)))
    assert (sign > 0).all()
    assert np.all(np.abs(got - want) <= 1e-4 * np.maximum(1.0, np.abs(want))), np.abs(got - want).max()
    # singular (rank 0..5 built exactly in f32 planes) and indefinite matrices -> -inf
    v = rng.normal(size=(6, 6)).astype(np.float32)
    sing = np.zeros((6, 6, 6), np.float64)
    for r in range(6):
        for q in range(r):
            sing[r] += np.outer(v[q], v[q])
    sing[:, :, 5] = sing[:, 5, :] = 0.0   # a zero row and column: exactly singular whatever the rounding
    assert np.all(log_det_6x6_f32(planes_from_matrices(sing)) == -np.inf)
    indef = np.diag([1.0, 2.0, -1.0, 3.0, 1.0, 1.0])[None]
    assert log_det_6x6_f32(planes_from_matrices(indef))[0] == -np.inf
    nan = np.eye(6)[None].copy()
    nan[0, 3, 3] = np.nan
    assert np.isnan(log_det_6x6_f32(planes_from_matrices(nan))[0])


def planes_to64(planes):
    n = planes.shape[1]
    m = np.zeros((n, 6, 6), np.float64)
    for (i, k), e in PLANE.items():
        m[:, i, k] = m[:, k, i] = planes[e]
    return m


def test_numpy_accumulate_restatement_is_the_outer_product_sum():
    rng = np.random.default_rng(9)
    h = np.zeros((21, 50), np.float32)
    vts = [rng.normal(size=(50, 10)).astype(np.float32) for _ in range(3)]
    for vt in vts:
        accumulate_f32(h, vt)
    j = np.stack([vt[:, J_COLS].astype(np.float64) for vt in vts])
    want = np.einsum("vni,vnk->nik", j, j)
    assert np.allclose(planes_to64(h), want, rtol=1e-5, atol=1e-6)


def test_reference_order_is_the_stable_descending_sort():
    s = np.array([1.0, np.nan, -0.0, 0.0, -np.inf, 1.0, np.inf, np.nan, -np.inf, 0.0], np.float32)
    assert reference_order(s) == [6, 0, 5, 2, 3, 9, 4, 8, 1, 7]
