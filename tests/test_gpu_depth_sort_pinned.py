"""The fused depth sort (brush_amd/csrc/depth_sort.hip: dsort_hist / dsort_split / dsort_bucket and the sample run) called on its own
through bh_debug_depth_sort (the test-hooks library; api.hip), every path, and held to tests/dsort_ref.py bit for bit.  The renders
of test_gpu_depth_sort.py compare the order with the generic sort's; the permutation is the stable sort's whatever the split digits
are, so they cannot see a wrong splitter table, a wrong digit or a path that never ran.  Here every case compares, as uint32 with
np.array_equal:
    out_keys[:nv], out_vals[:nv], cum[:nv]            all nv entries
    out_*[nv : n + 64], cum[nv : n + 64]              still the fill pattern: entries behind the visible prefix are not written
    totals[0:255], totals[256:511]                    the split's digit totals of keys and of tile counts (SLOT_SORT_HIST's head)
    the table's 258 words (and the two behind them)   where the test owns the table
    the host's note for the table                     comes back 1 (own table)
and the inputs are unchanged.  counts reach 40 000, so cum wraps in the large cases; about a quarter of the keys is 0xFFFFFFFF.

Table modes:  "off"  spl = NULL on a context with dsort_splitters = 0: linear split, no table
              "own"  a table of the test's (fresh: zeros with the host's note set, so no sample run; or preloaded)
              "ctx"  spl = NULL on a fresh default context: its own table, of which only the digit totals show
Tables handed to the kernels are ones a frame could have written (ascending, sentinel in word 254); minmax covers the keys.

Cases (CASES below; test_dsort_ref.py checks without a GPU, from the restatement alone, that each reaches what it is named for):
  sizes     n = 1, 2, 63, 64, 65 | 2047, 2048, 2049 (DS_TILE) | 4096 + 5 | 32 * 2048 and + 1 (a second group) | 512 * 2048 + 1 (a
            seventeenth group: sort_group_offset's second trip) | 1024 * 2048 (32 groups, the last direct size) and + 1 (scanned group
            table), each "off" and "own"; at n = 4101 and 65537: all culled, one visible key first / last, all equal, descending, ascending,
            and keys / counts at addresses that are no multiple of 16 bytes (the histogram kernel's scalar loads for whole chunks).
  resident  one bucket of S in {1, 64, 1023, 1024, 1025, 7167, 7168} keys spanning exactly B bits: B in {0, 1, 8, 9, 10, 18, 19} by a
            cluster of width 2^B plus one key 255 * 2^B + 255 above its base (linear split: the cluster is bucket 0); B in {27, 28, 32}
            by a preloaded table whose 254 splitters are 0xFFFFFFFE (every smaller key is bucket 0; 255 * 2^27 does not fit 32 bits,
            so 27 goes this way too).  0 .. 4 counting passes.  Half the keys come from eight values: stability shows.
  chunked   S in {7169, 8192, 3 * 4096 + 1} x B in {0, 1, 8, 9, 24} (one and three passes; B = 0 is the stable copy); 20 000 keys below
            2^25 under a key 0xFFFFFFFE, linear split: half of them in bucket 0 with 25 bits (five passes); 9000 keys over 32 bits by the
            preloaded table (five passes of 7, 7, 6, 6, 6 bits).
  digits    a table with distinct splitters and runs of equal ones; keys on, one below and one above every splitter, below the first
            and above the last; the frame's range off the table's by tol and tol + 1 at either end and side (tol + 1: the totals are the
            linear formula's); word 255 zero; nv = 16383 / 16384 on a valid table (left / rewritten); key ranges of 0, 1, 254, 255, 256,
            2^24 and 0xFFFFFFFE with the first and last key of every linear digit.
  handover  three frames of different depth distributions on one table (linear, then each at the quantiles of the one before), own and ctx.
  sample    n = 2^17 - 1 and 2^17 without the host's note, 97 % of the depths in a thin shell: no sample / the sample's quantiles; a
            sample of fewer than 1024 visible keys leaves no table; the same on a context's own table."""
import ctypes as C
import time

import numpy as np
import pytest

import dsort_ref as R

gpu = pytest.mark.gpu   # (per test: test_dsort_ref.py imports the cases without a GPU)

PATTERN = 0xA5C3F00D
GUARD = 64
COUNT_MAX = 40000


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def _rng(*seed):
    return np.random.default_rng([0xD5, *seed])


def _counts(rng, n):
    return rng.integers(0, COUNT_MAX + 1, n).astype(np.uint32)


def _with_culled(vis, rng, share=0.25):
    """The visible keys in their order, with culled keys scattered between them: `share` of the result."""
    vis = np.asarray(vis, np.uint32)
    ncull = int(round(vis.size * share / (1.0 - share)))
    keys = np.full(vis.size + ncull, R.CULLED, np.uint32)
    at = np.ones(keys.size, bool)
    at[rng.permutation(keys.size)[:ncull]] = False
    keys[at] = vis
    return keys


def _fresh_table():
    t = np.zeros(R.SPL_STRIDE, np.uint32)
    t[258:] = PATTERN
    return t


def _table(splitters, tmin, tmax, valid=1):
    t = _fresh_table()
    t[:254] = splitters
    t[254], t[255], t[256], t[257] = R.M32, valid, tmin, tmax
    return t


def _top_table():
    """A frame nearly all of whose keys were 0xFFFFFFFE over the range [0, 0xFFFFFFFE] wrote this: every smaller key is bucket 0."""
    return _table(np.full(254, 0xFFFFFFFE, np.uint32), 0, 0xFFFFFFFE)


def _cluster(rng, s, span, base):
    """s keys in [base, base + span], both ends present (s >= 2), half of them from eight values."""
    k = rng.integers(0, span + 1, s, dtype=np.uint64)
    few = rng.integers(0, span + 1, 8, dtype=np.uint64)
    dup = rng.random(s) < 0.5
    k[dup] = few[rng.integers(0, 8, int(dup.sum()))]
    if s >= 2:
        i, j = rng.permutation(s)[:2]
        k[i], k[j] = 0, span
    else:
        k[0] = 0
    return (k + np.uint64(base)).astype(np.uint32)


class Case:
    """group, name, table mode, build() -> ([(keys, counts) per frame], table0 or None, written0), claims per frame (see check_claims)."""
    def __init__(self, group, name, mode, build, claims, offsets=(0, 0)):
        self.group, self.name, self.mode, self.build, self.claims = group, name, mode, build, claims
        self.offsets = offsets   # words by which the keys' and the counts' device pointers are moved off their 16-byte alignment

    @property
    def id(self):
        return "%s-%s-%s" % (self.group, self.name, self.mode)


CASES = []


def _add(group, name, mode, build, *claims, **kw):
    CASES.append(Case(group, name, mode, build, list(claims), **kw))


# ---- sizes ----
SIZES = (1, 2, 63, 64, 65, 2047, 2048, 2049, 4096 + 5, 32 * 2048, 32 * 2048 + 1, 512 * 2048 + 1, 1024 * 2048, 1024 * 2048 + 1)
SIZE_BASE, SIZE_SPAN = 0x40000000, 1 << 20


def _size_frame(n, kind="random"):
    rng = _rng(1, n, sum(map(ord, kind)))
    culled = rng.random(n) < 0.25
    if kind == "random":
        keys = (SIZE_BASE + rng.integers(0, SIZE_SPAN, n)).astype(np.uint32)
        culled[0] = False   # (n = 1, 2: something to sort)
    elif kind == "allculled":
        keys, culled[:] = np.zeros(n, np.uint32), True
    elif kind in ("onefirst", "onelast"):
        keys, culled[:] = np.full(n, SIZE_BASE + 77, np.uint32), True
        culled[0 if kind == "onefirst" else n - 1] = False
    elif kind == "equal":
        keys = np.full(n, SIZE_BASE + 77, np.uint32)
    elif kind == "descending":
        keys = (SIZE_BASE + 3 * (n - np.arange(n))).astype(np.uint32)
    elif kind == "ascending":
        keys = (SIZE_BASE + 3 * np.arange(n)).astype(np.uint32)
    else:
        raise KeyError(kind)
    keys[culled] = R.CULLED
    return keys, _counts(rng, n)


for _n in SIZES:
    _nb = (_n + 2047) // 2048
    for _mode in ("off", "own"):
        _add("sizes", "n%d" % _n, _mode, lambda n=_n, m=_mode: ([_size_frame(n)], _fresh_table() if m == "own" else None, 1),
             dict(used_table=False, sampled=False, nblocks=_nb, ngroups=(_nb + 31) // 32, scanned=_nb > 1024, tail=_n % 2048))
for _n in (4096 + 5, 32 * 2048 + 1):
    for _kind, _claim in (("allculled", dict(nv=0)), ("onefirst", dict(nv=1)), ("onelast", dict(nv=1)), ("equal", dict(buckets=1, bucket0=dict(bits=0))),
                          ("descending", {}), ("ascending", {})):
        _add("sizes", "n%d-%s" % (_n, _kind), "own", lambda n=_n, k=_kind: ([_size_frame(n, k)], _fresh_table(), 1), dict(used_table=False, sampled=False, **_claim))
# (the histogram kernel's 16-byte loads are taken for aligned pointers only: the scalar loop for whole chunks too)
for _n, _off in ((4096 + 5, (1, 0)), (32 * 2048 + 1, (2, 3))):
    _add("sizes", "n%d-unaligned" % _n, "own", lambda n=_n: ([_size_frame(n)], _fresh_table(), 1), dict(used_table=False, sampled=False), offsets=_off)


# ---- one bucket of S keys spanning B bits ----
def _bucket_frame(s, b, how):
    rng = _rng(2, s, b)
    if how == "cluster":   # linear split: the cluster is bucket 0, the far key bucket 254
        base = 0x3F000000 if b <= 19 else 0
        vis = np.concatenate([_cluster(rng, s, (1 << b) - 1, base), [base + 255 * (1 << b) + 255]])
        table = _fresh_table()
    else:                  # the preloaded table: every key below 0xFFFFFFFE is bucket 0
        vis = np.concatenate([_cluster(rng, s, min((1 << b) - 1, 0xFFFFFFFD), 0), [0xFFFFFFFE]])
        table = _top_table()
    vis = vis.astype(np.uint32)[rng.permutation(s + 1)]
    keys = _with_culled(vis, rng)
    return [(keys, _counts(rng, keys.size))], table, 1


def _bucket_claim(s, b, how):
    bits = b if s >= 2 else 0
    path, passes = R.bucket_plan(s, bits)
    return dict(used_table=how == "table", sampled=False, nv=s + 1, buckets=2, bucket0=dict(size=s, bits=bits, path=path, passes=passes))


RESIDENT_S, RESIDENT_B = (1, 64, 1023, 1024, 1025, 7167, 7168), (0, 1, 8, 9, 10, 18, 19, 27, 28, 32)
CHUNKED_S, CHUNKED_B = (7169, 8192, 3 * 4096 + 1), (0, 1, 8, 9, 24)
for _s in RESIDENT_S:
    for _b in RESIDENT_B:
        _how = "cluster" if _b <= 24 else "table"
        _add("resident", "S%d-B%d" % (_s, _b), "own", lambda s=_s, b=_b, h=_how: _bucket_frame(s, b, h), _bucket_claim(_s, _b, _how))
for _s in CHUNKED_S:
    for _b in CHUNKED_B:
        _add("chunked", "S%d-B%d" % (_s, _b), "own", lambda s=_s, b=_b: _bucket_frame(s, b, "cluster"), _bucket_claim(_s, _b, "cluster"))
_add("chunked", "S9000-B32", "own", lambda: _bucket_frame(9000, 32, "table"), _bucket_claim(9000, 32, "table"))


def _linear25():
    rng = _rng(3)
    vis = rng.integers(0, 1 << 25, 20000).astype(np.uint32)
    vis[:2] = 0, (1 << 25) - 1
    vis = np.concatenate([vis, [0xFFFFFFFE]]).astype(np.uint32)[rng.permutation(20001)]
    keys = _with_culled(vis, rng)
    return [(keys, _counts(rng, keys.size))], _fresh_table(), 1


_add("chunked", "linear-B25", "own", _linear25, dict(used_table=False, sampled=False, nv=20001, bucket0=dict(size_range=(9000, 11000), bits=25, path="chunked", passes=5)))

# ---- digit rules ----
T_MIN, T_MAX = 0x40000000, 0x40100000
T_TOL = (T_MAX - T_MIN) >> 4


def _rule_splitters():
    """254 ascending splitters strictly inside (T_MIN + 1, T_MAX - 1): 100 distinct, a run of 40, a run of 60, 54 distinct."""
    rng = _rng(4)
    d = np.sort(rng.permutation(np.arange(T_MIN + 1000, T_MAX - 1000, 7))[:156])
    return np.concatenate([d[:100], np.full(40, d[100]), np.full(60, d[101]), d[102:]]).astype(np.uint32)


def _rule_keys(kmin, kmax, rng):
    """Every splitter, one below and one above, three times each; keys below the first and above the last; the range's ends."""
    s = np.unique(_rule_splitters()).astype(np.int64)
    vis = np.concatenate([np.repeat(np.concatenate([s - 1, s, s + 1]), 3), rng.integers(T_MIN - T_TOL - 1, int(s[0]), 50),
                          rng.integers(int(s[-1]) + 1, T_MAX + T_TOL + 2, 50)])
    vis = vis[(vis >= kmin) & (vis <= kmax)]
    vis = np.concatenate([vis, [kmin, kmax]])
    return vis[rng.permutation(vis.size)].astype(np.uint32)


def _rule_frame(kmin, kmax, valid=1):
    rng = _rng(5, kmin, kmax)
    keys = _with_culled(_rule_keys(kmin, kmax, rng), rng)
    return [(keys, _counts(rng, keys.size))], _table(_rule_splitters(), T_MIN, T_MAX, valid), 1


_add("digits", "splitters", "own", lambda: _rule_frame(T_MIN, T_MAX), dict(used_table=True, sampled=False, buckets_at_least=150))
_add("digits", "word255-zero", "own", lambda: _rule_frame(T_MIN, T_MAX, 0), dict(used_table=False, sampled=False))
for _end in ("kmin", "kmax"):
    for _sign in (-1, 1):
        for _d in (T_TOL, T_TOL + 1):
            _lo, _hi = (T_MIN + _sign * _d, T_MAX) if _end == "kmin" else (T_MIN, T_MAX + _sign * _d)
            _add("digits", "%s%+d" % (_end, _sign * _d), "own", lambda lo=_lo, hi=_hi: _rule_frame(lo, hi), dict(used_table=_d == T_TOL, sampled=False))


def _nv_frame(nv):
    rng = _rng(6, nv)
    vis = rng.integers(T_MIN, T_MAX + 1, nv).astype(np.uint32)
    vis[:2] = T_MIN, T_MAX
    keys = _with_culled(vis[rng.permutation(nv)], rng)
    return [(keys, _counts(rng, keys.size))], _table(_rule_splitters(), T_MIN, T_MAX), 1


for _nv in (R.SPL_MIN_KEYS - 1, R.SPL_MIN_KEYS):
    _add("digits", "nv%d" % _nv, "own", lambda nv=_nv: _nv_frame(nv), dict(used_table=True, sampled=False, nv=_nv, table_valid_after=int(_nv >= R.SPL_MIN_KEYS)))

SCALE_RANGES = (0, 1, 254, 255, 256, 1 << 24, 0xFFFFFFFE)


def _scale_frame(rng_):
    rng = _rng(7, rng_)
    kmin = 0 if rng_ == 0xFFFFFFFE else 0x3F800000
    if rng_ <= 256:
        off = np.repeat(np.arange(rng_ + 1, dtype=np.int64), 5)
    else:   # the first key of every linear digit and the one in front of it, from the definition of the scale alone
        scale = R.make_scale(True, kmin, kmin + rng_)
        first = np.array([((d << 32) + scale - 1) // scale for d in range(1, 255)], np.int64)
        off = np.concatenate([first, first - 1, rng.integers(0, rng_ + 1, 3000), [0, rng_]])
        off = off[(off >= 0) & (off <= rng_)]
    vis = (off[rng.permutation(off.size)] + kmin).astype(np.uint32)
    keys = _with_culled(vis, rng)
    return [(keys, _counts(rng, keys.size))], _fresh_table(), 1


for _r in SCALE_RANGES:
    _add("digits", "range%d" % _r, "own", lambda r=_r: _scale_frame(r), dict(used_table=False, sampled=False, key_range=_r, **(dict(buckets=255) if _r > 256 else {})))


# ---- the table from frame to frame ----
def _shaped(rng, nv, shape, lo, hi):
    u = rng.random(nv)
    if shape == "uniform":
        z = u
    elif shape == "shell":     # 97 % of the depths in a thousandth of the range
        z = np.where(rng.random(nv) < 0.97, 0.6 + 0.001 * u, u)
    elif shape == "bimodal":
        z = np.where(rng.random(nv) < 0.5, 0.1 + 0.02 * u, 0.85 + 0.05 * u)
    else:
        raise KeyError(shape)
    vis = (lo + z * (hi - lo)).astype(np.int64)
    vis[:2] = lo, hi
    return vis[rng.permutation(nv)].astype(np.uint32)


def _handover(mode):
    rng = _rng(8)
    lo, hi = 0x40000000, 0x41000000
    tol = (hi - lo) >> 4
    frames = []
    for shape, a, b in (("uniform", lo, hi), ("shell", lo + tol // 2, hi - tol // 3), ("bimodal", lo + tol // 2 - tol // 4, hi - tol // 3 + tol // 5)):
        keys = _with_culled(_shaped(rng, 30000, shape, a, b), rng)
        frames.append((keys, _counts(rng, keys.size)))
    return frames, _fresh_table() if mode == "own" else None, 1


for _mode in ("own", "ctx"):
    _add("handover", "three-frames", _mode, lambda m=_mode: _handover(m), *[dict(used_table=u, sampled=False, table_valid_after=1) for u in (False, True, True)])


# ---- the sample run ----
def _sample_frame(n, share, mode):
    rng = _rng(9, n, int(share * 100))
    nv = int(round(n * (1.0 - share)))
    vis = _shaped(rng, nv, "shell", 0x40000000, 0x41000000)
    keys = np.full(n, R.CULLED, np.uint32)
    keys[np.sort(rng.permutation(n)[:nv])] = vis
    return [(keys, _counts(rng, n))], _fresh_table() if mode == "own" else None, 0


_add("sample", "n131071", "own", lambda: _sample_frame((1 << 17) - 1, 0.25, "own"), dict(used_table=False, sampled=False, table_valid_after=1, largest_bucket_at_least=40000))
_add("sample", "n131072", "own", lambda: _sample_frame(1 << 17, 0.25, "own"),
     dict(used_table=True, sampled=True, sample_valid=1, table_valid_after=1, largest_bucket_at_most=7168))
_add("sample", "n131072", "ctx", lambda: _sample_frame(1 << 17, 0.25, "ctx"), dict(used_table=True, sampled=True, sample_valid=1, largest_bucket_at_most=7168))
_add("sample", "n131072-few-visible", "own", lambda: _sample_frame(1 << 17, 0.65, "own"),
     dict(used_table=False, sampled=True, sample_valid=0, sample_nv_below=R.SPL_SAMPLE_MIN_KEYS, nv_at_least=R.SPL_MIN_KEYS, table_valid_after=1))


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement of a case, and what the case claims about it
# ---------------------------------------------------------------------------------------------------------------------------
def reference_runs(case, frames, table, written):
    """dsort_ref.run of every frame in turn -> [Run]; "ctx": the context's own table starts as zeros without the host's note."""
    if case.mode == "ctx":
        table, written = np.zeros(R.SPL_STRIDE, np.uint32), False
    if case.mode == "off":
        table = None
    runs = []
    for keys, counts in frames:
        r = R.run(keys, counts, table, bool(written))
        runs.append(r)
        table, written = r.table, r.written
    return runs


def check_claims(case, frames, runs):
    assert len(runs) == len(case.claims) == len(frames), case.id
    for (keys, counts), r, claim in zip(frames, runs, case.claims):
        f, what = r.frame, (case.id, claim)
        assert keys.dtype == counts.dtype == np.uint32 and keys.shape == counts.shape
        assert f.used_table == claim["used_table"] and (r.sample is not None) == claim["sampled"], what
        sizes = [b["size"] for b in f.buckets.values()]
        for k, v in claim.items():
            if k in ("used_table", "sampled"):
                continue
            elif k in ("nblocks", "ngroups", "scanned"):
                assert getattr(r, k) == v, what
            elif k == "tail":
                assert keys.size % R.DS_TILE == v, what
            elif k == "nv":
                assert f.nv == v, what
            elif k == "nv_at_least":
                assert f.nv >= v, what
            elif k == "buckets":
                assert len(f.buckets) == v, (what, len(f.buckets))
            elif k == "buckets_at_least":
                assert len(f.buckets) >= v, (what, len(f.buckets))
            elif k == "bucket0":
                b0 = f.buckets[0]
                for kk, vv in v.items():
                    if kk == "size_range":
                        assert vv[0] <= b0["size"] <= vv[1], (what, b0)
                    else:
                        assert b0[kk] == vv, (what, b0)
            elif k == "key_range":
                vis = keys[keys != R.CULLED]
                assert int(vis.max()) - int(vis.min()) == v, what
            elif k == "table_valid_after":
                assert r.table is None or int(r.table[255]) == v, what
            elif k == "sample_valid":
                assert int(r.sample.table[255]) == v, what
            elif k == "sample_nv_below":
                assert r.sample.nv < v, (what, r.sample.nv)
            elif k == "largest_bucket_at_least":
                assert max(sizes) >= v, (what, max(sizes))
            elif k == "largest_bucket_at_most":
                assert max(sizes) <= v, (what, max(sizes))
            else:
                raise KeyError(k)


# ---------------------------------------------------------------------------------------------------------------------------
# the GPU side
# ---------------------------------------------------------------------------------------------------------------------------
def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(dev)


def _filled(n, dev):
    import torch
    return torch.full((n + GUARD,), int(np.uint32(PATTERN).view(np.int32)), dtype=torch.int32, device=dev)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def gpu_run(ctx, dev, keys, counts, table_dev, written, offsets=(0, 0)):
    """One bh_debug_depth_sort -> dict of everything it left, as numpy uint32."""
    n = keys.size
    minmax = R.minmax_of(keys)
    k, c, mm = _dev(np.concatenate([np.zeros(offsets[0], np.uint32), keys]), dev)[offsets[0]:], _dev(np.concatenate([np.zeros(offsets[1], np.uint32), counts]), dev)[offsets[1]:], \
        _dev(minmax, dev)
    assert k.data_ptr() % 16 == 4 * offsets[0] and c.data_ptr() % 16 == 4 * offsets[1]
    ok, ov, cum = _filled(n, dev), _filled(n, dev), _filled(n, dev)
    flag = C.c_int(int(written))
    totals = (C.c_uint32 * 512)()
    ctx.check(ctx.lib.bh_debug_depth_sort(ctx._h, _ptr(k), _ptr(mm), _ptr(c), n, _ptr(ok), _ptr(ov), _ptr(cum), _ptr(table_dev), C.byref(flag), totals))
    return dict(out_keys=_u32(ok), out_vals=_u32(ov), cum=_u32(cum), totals=np.frombuffer(totals, np.uint32).copy(), written=flag.value,
                table=None if table_dev is None else _u32(table_dev), inputs=(_u32(k), _u32(c), _u32(mm)), minmax=minmax)


def _first_bad(a, b):
    i = int(np.flatnonzero(a != b)[0])
    return "first of %d differences at %d: got 0x%08X, want 0x%08X" % (int((a != b).sum()), i, int(a[i]), int(b[i]))


def _same(got, want, what):
    got, want = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, _first_bad(got, want))


def assert_run(case, step, keys, counts, got, ref):
    f, n, nv = ref.frame, keys.size, ref.frame.nv
    what = "%s frame %d" % (case.id, step)
    pattern = np.full(n + GUARD - nv, PATTERN, np.uint32)
    for name, want in (("out_keys", f.out_keys), ("out_vals", f.order), ("cum", f.cum)):
        assert got[name].size == n + GUARD
        _same(got[name][:nv], want, what + ": " + name)
        _same(got[name][nv:], pattern, what + ": %s behind the visible prefix (nv = %d, n = %d)" % (name, nv, n))
    _same(got["totals"][0:255], f.totals[0:255], what + ": digit totals of keys (%s split)" % ("table" if f.used_table else "linear"))
    _same(got["totals"][256:511], f.totals[256:511], what + ": digit totals of tile counts")
    if case.mode == "own":
        _same(got["table"], ref.table, what + ": the table afterwards")
        assert got["written"] == 1, what
    if case.mode == "ctx":
        assert got["written"] == 1, what
    for g, w, name in zip(got["inputs"], (keys, counts, got["minmax"]), ("keys", "counts", "minmax")):
        _same(g, w, what + ": input " + name)


@pytest.fixture(scope="module")
def contexts(dev):
    """One context per table mode for the whole file (scratch of every size is reused, as in a training run); "ctx" cases make their own."""
    import brush_amd as ba
    from brush_amd import _ffi
    lib = _ffi.load_test_hooks()
    made = {"off": ba.Context(dev, lib=lib, options={"dsort_splitters": 0}), "own": ba.Context(dev, lib=lib)}
    yield made
    for c in made.values():
        c.close()


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_depth_sort_equals_the_restatement(dev, contexts, case):
    import brush_amd as ba
    from brush_amd import _ffi
    t0 = time.perf_counter()
    frames, table, written = case.build()
    runs = reference_runs(case, frames, table, written)
    check_claims(case, frames, runs)
    ctx = contexts[case.mode] if case.mode != "ctx" else ba.Context(dev, lib=_ffi.load_test_hooks())
    try:
        table_dev = _dev(table, dev) if case.mode == "own" else None
        for step, ((keys, counts), ref) in enumerate(zip(frames, runs)):
            got = gpu_run(ctx, dev, keys, counts, table_dev, written, case.offsets)
            assert_run(case, step, keys, counts, got, ref)
            written = got["written"]
    finally:
        if case.mode == "ctx":
            ctx.close()
    f = runs[-1].frame
    print("%s: n %d, nv %d, %d buckets (largest %d), %s split, %.2f s" % (case.id, frames[-1][0].size, f.nv, len(f.buckets), max([b["size"] for b in f.buckets.values()] or [0]),
                                                                          "table" if f.used_table else "linear", time.perf_counter() - t0))


@gpu
def test_hook_refuses_what_the_fused_sort_does_not_take(dev, contexts):
    import torch
    ctx = contexts["own"]
    lib = ctx.lib
    t = torch.zeros(512, dtype=torch.int32, device=dev)
    p, flag, totals = _ptr(t), C.c_int(1), (C.c_uint32 * 512)()
    args = [p, p, p, 16, p, p, p, p, C.byref(flag), totals]
    for i in (0, 1, 2, 4, 5, 6, 8, 9):   # each pointer that must be there (8: the note of a table that is given)
        bad = list(args)
        bad[i] = None
        assert lib.bh_debug_depth_sort(ctx._h, *bad) == -1, i
    for n in (0, (16 << 20) + 1):
        bad = list(args)
        bad[3] = n
        assert lib.bh_debug_depth_sort(ctx._h, *bad) == -1, n
    assert lib.bh_debug_depth_sort(None, *args) == -1
    torch.cuda.synchronize(dev)
    assert not t.any().item()   # nothing ran
