"""The dealing path of the depth order (brush_amd/csrc/depth_deal.h: K1 puts every listed splat into its depth-sort bucket, one bucket
launch follows) restated on top of tests/dsort_ref.py, and the cases test_gpu_depth_deal.py runs through bh_debug_depth_deal.
test_depth_deal_ref.py shows without a GPU that every case reaches the path it is named for.

What the path leaves is what depth_sort_scan leaves (dsort_ref.run with the host's note set: the stable argsort of the listed keys, the
scan, the table of the frame's quantiles) whatever the digits were; the digits decide only WHICH way it is reached:
    bucket of a key      number of the table's splitters <= key — always, no key-range rule
    sizes                the 255 counter words: low half = keys of the bucket, high half = sum of their tile counts (mod 2^32)
    overflow             a bucket with more keys than `cap` slots, or a table whose word 255 is zero: the three launches run
    resident / chunked   a bucket of at most / more than FAST_CAP keys
    tie path             a resident bucket whose longest run of equal keys is 2 .. TIE_RUN_MAX has the runs' ids put in order where they lie;
                         a longer run sends it through passes by id and by key again; a chunked bucket always leads with the id passes"""
import numpy as np

import dsort_ref as R

DEAL_BUCKETS = 255
TIE_RUN_MAX = 8   # depth_sort.hip


def deal_capacity(n):
    """depth_deal.h"""
    return (n + 127) // 128 if n // 128 > 2048 else 2048


def base_table(seed=1, nv=20000, lo=1.0, hi=50.0):
    """A table a frame of nv uniformly spread depths has written."""
    rng = np.random.default_rng([0xDEA1, seed])
    keys = rng.uniform(lo, hi, nv).astype(np.float32).view(np.uint32)
    t = np.zeros(R.SPL_STRIDE, np.uint32)
    return R.run(keys, np.ones(nv, np.uint32), t, written=True).table


def top_table():
    """254 equal splitters above every key used here: everything is bucket 0."""
    t = np.zeros(R.SPL_STRIDE, np.uint32)
    t[:254] = 0xFFFFFFFE
    t[254] = R.M32
    t[255] = 1
    t[256], t[257] = 1, 0xFFFFFFFE
    return t


class Plan:
    """Which way the dealing path takes a frame."""
    def __init__(self, keys, counts, table, cap):
        keys, counts = np.asarray(keys, np.uint32), np.asarray(counts, np.uint32)
        listed = keys != R.CULLED
        self.cap = cap
        self.valid = int(table[255]) != 0
        self.sizes = np.zeros(DEAL_BUCKETS, np.int64)
        self.tiles = np.zeros(DEAL_BUCKETS, np.int64)
        self.tied, self.paths, self.longest_run = {}, {}, {}
        if self.valid:
            d = R.table_digits(keys, table)
            self.sizes = np.bincount(d[listed], minlength=256)[:DEAL_BUCKETS]
            self.tiles = np.bincount(d[listed], weights=counts[listed].astype(np.float64), minlength=256)[:DEAL_BUCKETS].astype(np.int64) & R.M32
            for b in np.flatnonzero(self.sizes):
                kb = keys[listed & (d == b)]
                self.paths[int(b)] = "resident" if kb.size <= R.FAST_CAP else "chunked"
                self.tied[int(b)] = np.unique(kb).size < kb.size
                self.longest_run[int(b)] = int(np.unique(kb, return_counts=True)[1].max())
        self.overflow = (not self.valid) or int(self.sizes.max()) > cap

    def words(self):
        """The 255 bucket words as the kernels leave them (a frame that overflowed: still every listed key counted)."""
        return (self.tiles.astype(np.uint64) << np.uint64(32)) | self.sizes.astype(np.uint64)


class Case:
    def __init__(self, name, frames, table, cap=0, claims=(), strides=(1,)):
        self.id, self.frames, self.table, self.cap, self.claims, self.strides = name, frames, table, cap, claims, strides


def _rng(*seed):
    return np.random.default_rng([0xDEA2, *seed])


def _counts(rng, n):
    return rng.integers(0, 40001, n).astype(np.uint32)


def _interleave(vis, n, rng):
    """n keys: the listed ones in their order at random places, culled keys between them."""
    keys = np.full(n, R.CULLED, np.uint32)
    keys[np.sort(rng.permutation(n)[:vis.size])] = vis
    return keys


def _depths(rng, nv, lo=1.0, hi=50.0):
    return rng.uniform(lo, hi, nv).astype(np.float32).view(np.uint32)


def _coprime_strides(n, k, rng):
    out = [1]
    while len(out) < k:
        s = int(rng.integers(2, max(3, n)))
        if np.gcd(s, n) == 1:
            out.append(s)
    return tuple(out)


def build_cases():
    cases = []
    T0 = base_table()
    # listed counts, culled splats interleaved
    for nv, n in ((0, 4101), (1, 4101), (63, 4101), (64, 65537), (65, 65537), (16383, 65537), (16384, 65537), (200000, (1 << 20) + 1)):
        rng = _rng(1, nv)
        keys = _interleave(_depths(rng, nv), n, rng)
        cases.append(Case("listed-%d-of-%d" % (nv, n), [(keys, _counts(rng, n))], T0, claims=("no-overflow",) + (("resident",) if nv else ())))
    # all keys equal: one bucket, nothing but ties
    for nv, n, path in ((5000, 20001, "resident"), (9000, 20001, "chunked")):
        rng = _rng(2, nv)
        keys = _interleave(np.full(nv, np.float32(7.25).view(np.uint32), np.uint32), n, rng)
        cases.append(Case("all-equal-%d" % nv, [(keys, _counts(rng, n))], T0, cap=16384, claims=("no-overflow", "tied", path, "one-bucket")))
    # runs of equal keys on and beside splitters
    rng = _rng(3)
    spl = T0[:254].astype(np.int64)
    vals = np.concatenate([spl[j] + np.array([-1, 0, 1]) for j in (0, 1, 100, 101, 252, 253)]).astype(np.uint32)
    vis = rng.permutation(np.repeat(vals, 300))
    keys = _interleave(vis, 20001, rng)
    cases.append(Case("runs-at-splitters", [(keys, _counts(rng, keys.size))], T0, claims=("no-overflow", "tied", "resident", "on-splitter")))
    # short runs: 2 .. TIE_RUN_MAX equal keys (ordered where they lie), and TIE_RUN_MAX + 1 (the id passes), in buckets of their own
    for name, runs in (("short-runs", range(2, TIE_RUN_MAX + 1)), ("run-one-over", (TIE_RUN_MAX + 1,))):
        rng = _rng(12, len(name))
        vis = np.unique(_depths(rng, 6000))
        picks = vis[rng.permutation(vis.size)[:40]]
        vis = rng.permutation(np.concatenate([vis] + [np.repeat(picks[j], runs[j % len(runs)] - 1) for j in range(40)]))
        keys = _interleave(vis, 20001, rng)
        cases.append(Case(name, [(keys, _counts(rng, keys.size))], T0, claims=("no-overflow", "resident", "tied", "runs-short" if name == "short-runs" else "runs-long")))
    # monotone and reversed
    for name, step in (("ascending", 1), ("descending", -1)):
        rng = _rng(4, step + 1)
        vis = np.sort(np.unique(_depths(rng, 30000)))[::step]
        keys = _interleave(vis, 50001, rng)
        cases.append(Case(name, [(keys, _counts(rng, keys.size))], T0, claims=("no-overflow", "resident", "untied")))
    # everything in one bucket, beyond FAST_CAP: the chunked path (distinct keys and keys with ties)
    for name, ties in (("one-bucket-chunked", False), ("one-bucket-chunked-ties", True)):
        rng = _rng(5, int(ties))
        vis = _depths(rng, 20000)
        if ties:
            vis[rng.permutation(20000)[:8000]] = rng.choice(vis[:8], 8000)
        keys = _interleave(vis, 40001, rng)
        cases.append(Case(name, [(keys, _counts(rng, keys.size))], top_table(), cap=32768, claims=("no-overflow", "chunked", "one-bucket") + (("tied",) if ties else ())))
    # a bucket exactly at capacity and one over it (capacity forced small)
    for nv, over in ((3000, False), (3001, True)):
        rng = _rng(6, nv)
        keys = _interleave(_depths(rng, nv), 9001, rng)
        cases.append(Case("capacity-%d-of-3000" % nv, [(keys, _counts(rng, keys.size))], top_table(), cap=3000, claims=("overflow" if over else "no-overflow", "at-capacity")))
    # ... and with the even buckets of the frame's own distribution: one bucket one over
    rng = _rng(7)
    keys = _interleave(_depths(rng, 40000), 60001, rng)
    own_cap = int(Plan(keys, np.zeros(keys.size, np.uint32), T0, 1 << 30).sizes.max())
    cases.append(Case("capacity-largest-bucket-fits", [(keys, _counts(rng, keys.size))], T0, cap=own_cap, claims=("no-overflow", "at-capacity")))
    cases.append(Case("capacity-largest-bucket-one-over", [(keys, _counts(rng, keys.size))], T0, cap=own_cap - 1, claims=("overflow",)))
    # a table that holds no quantiles: the same answer as an overflow
    t = np.array(T0)
    t[255] = 0
    rng = _rng(8)
    keys = _interleave(_depths(rng, 5000), 20001, rng)
    cases.append(Case("table-not-valid", [(keys, _counts(rng, keys.size))], t, claims=("overflow",)))
    # three frames handing one table on (a range that moves: no key-range rule on this path)
    rng = _rng(9)
    frames = []
    for lo, hi, nv in ((1.0, 50.0, 30000), (2.0, 9.0, 25000), (0.5, 300.0, 40000)):
        keys = _interleave(_depths(rng, nv, lo, hi), 65537, rng)
        frames.append((keys, _counts(rng, keys.size)))
    cases.append(Case("handover", frames, T0, cap=65536, claims=("no-overflow", "last-frame-chunked")))
    # the same input dealt in five arrival orders
    rng = _rng(10)
    vis = _depths(rng, 60000)
    vis[rng.permutation(60000)[:20000]] = rng.choice(vis[:16], 20000)
    keys = _interleave(vis, 100003, rng)
    cases.append(Case("five-arrival-orders", [(keys, _counts(rng, keys.size))], T0, cap=8192, claims=("no-overflow", "tied"), strides=_coprime_strides(100003, 5, rng)))
    rng = _rng(11)
    keys = _interleave(np.full(9000, np.float32(3.5).view(np.uint32), np.uint32), 20011, rng)
    cases.append(Case("five-arrival-orders-chunked", [(keys, _counts(rng, keys.size))], T0, cap=16384, claims=("no-overflow", "tied", "chunked"),
                      strides=_coprime_strides(20011, 5, rng)))
    return cases


def reference(case):
    """-> per frame (Plan, dsort_ref.Run): the path the frame takes, and what it must leave (the table goes from frame to frame)."""
    out, table = [], np.array(case.table)
    for keys, counts in case.frames:
        plan = Plan(keys, counts, table, case.cap if case.cap else deal_capacity(keys.size))
        run = R.run(keys, counts, table, written=True)
        out.append((plan, run))
        table = run.table
    return out


def check_claims(case, refs):
    for (keys, counts), (plan, run) in zip(case.frames, refs):
        c = case.claims
        assert ("overflow" in c) == plan.overflow and ("no-overflow" in c) != plan.overflow, (case.id, plan.overflow, int(plan.sizes.max()), plan.cap)
        if "resident" in c:
            assert plan.paths and set(plan.paths.values()) == {"resident"}, case.id
        if "chunked" in c:
            assert "chunked" in plan.paths.values(), case.id
        if "last-frame-chunked" in c and keys is case.frames[-1][0]:   # (the table of the narrow frame before: most keys lie behind its last splitter)
            assert "chunked" in plan.paths.values(), case.id
        if "tied" in c:
            assert any(plan.tied[b] for b in plan.paths), case.id
            if "chunked" in c:
                assert any(plan.tied[b] and plan.paths[b] == "chunked" for b in plan.paths), case.id
        if "runs-short" in c:   # every run is ordered in place, and runs of every length up to the limit are there
            assert max(plan.longest_run.values()) == TIE_RUN_MAX and min(v for b, v in plan.longest_run.items() if plan.tied[b]) == 2, case.id
        if "runs-long" in c:
            assert max(plan.longest_run.values()) == TIE_RUN_MAX + 1, case.id
        if "untied" in c:
            assert not any(plan.tied.values()), case.id
        if "one-bucket" in c:
            assert len(plan.paths) == 1, case.id
        if "at-capacity" in c:
            assert abs(int(plan.sizes.max()) - plan.cap) <= 1 and (int(plan.sizes.max()) == plan.cap) != plan.overflow, case.id
        if "on-splitter" in c:
            spl = set(int(x) for x in case.table[:254])
            listed = keys[keys != R.CULLED]
            assert any(int(k) in spl for k in listed[:2000]) and any(int(k) + 1 in spl for k in listed[:2000]), case.id
        assert int(plan.sizes.sum()) == run.frame.nv or not plan.valid
