"""tests/dsort_ref.py (the restatement of the fused depth sort) tied to the oracle's radix_argsort + prefix_sum, and the cases of
test_gpu_depth_sort_pinned.py held to what they are named for — bucket size against FAST_CAP, bits, pass count, table used or
ignored, sampled or not — from the restatement alone.  No GPU."""
import os
import re

import numpy as np
import pytest

import dsort_ref as R
import test_gpu_depth_sort_pinned as P

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "brush_amd", "csrc")


def test_constants_are_the_sources():
    src = open(os.path.join(CSRC, "depth_sort.hip")).read()
    ctx = open(os.path.join(CSRC, "context.h")).read()

    def const(text, name):
        return re.search(r"constexpr \w+ %s = ([^;]+);" % name, text).group(1).strip()
    assert (const(src, "DS_WG"), src.count("#define BH_DS_KPT 8 "), const(src, "DS_TILE")) == ("256", 1, "DS_WG * DS_KPT") and R.DS_TILE == 256 * 8
    assert src.count("#define BH_BK_WG 1024 ") == 1 and const(src, "FAST_CAP") == "BK_WG <= 512 ? 8192 : 7168" and R.FAST_CAP == 7168
    assert (const(src, "SPL_WORDS"), const(src, "SPL_MIN_KEYS"), const(src, "SPL_SAMPLE_STRIDE"), const(src, "SPL_SAMPLE_MIN_N"), const(src, "SPL_SAMPLE_MIN_KEYS")) == \
        ("258", "16384", "64", "1u << 17", "1024")
    assert (R.SPL_WORDS, R.SPL_MIN_KEYS, R.SPL_SAMPLE_STRIDE, R.SPL_SAMPLE_MIN_N, R.SPL_SAMPLE_MIN_KEYS) == (258, 16384, 64, 1 << 17, 1024)
    assert (const(ctx, "COUNTER_SLOTS"), const(ctx, "SORT_GROUP_BLOCKS"), const(ctx, "SORT_DIRECT_GROUPS"), const(ctx, "DSORT_SPL_STRIDE")) == ("128", "32", "32", "260")
    assert (R.COUNTER_SLOTS, R.SORT_GROUP_BLOCKS, R.SORT_DIRECT_GROUPS, R.SPL_STRIDE) == (128, 32, 32, 260)
    # the pass rules restated in bucket_plan
    assert "const uint32_t passes = (bits + 8u) / 9u;" in src and "const uint32_t passes = bits <= 8u ? 1u : (bits <= 24u ? 3u : 5u);" in src
    assert "if (size <= (uint32_t)FAST_CAP) {" in src


@pytest.mark.parametrize("n,shape", [(1, "random"), (65, "random"), (4101, "random"), (70001, "dups"), (70001, "narrow"), (20000, "wide")])
def test_restatement_equals_the_oracles_sort_and_scan(oracle_lib, n, shape):
    """render.rs:177-187: radix_argsort(depths, 32 bits), then the prefix sum of the gathered tile counts; the culled keys sort last
    and the fused sort leaves them out."""
    rng = np.random.default_rng([n, len(shape)])
    keys = {"random": lambda: rng.integers(0x3F000000, 0x42000000, n), "dups": lambda: 0x40000000 + rng.integers(0, 50, n),
            "narrow": lambda: 0x40000000 + rng.integers(0, 1 << 14, n), "wide": lambda: rng.integers(0, 0xFFFFFFFF, n)}[shape]().astype(np.uint32)
    keys[rng.random(n) < 0.25] = R.CULLED
    keys[0] = 0x40000000
    counts = rng.integers(0, 40001, n).astype(np.uint32)
    rk, rv = oracle_lib.radix_argsort(keys, np.arange(n, dtype=np.uint32), 32)
    rcum = oracle_lib.prefix_sum(counts[rv])
    table = np.zeros(R.SPL_STRIDE, np.uint32)
    for tab, written in ((None, False), (table, True)):
        f = R.run(keys, counts, tab, written).frame
        assert f.nv == int((keys != R.CULLED).sum())
        assert np.array_equal(f.out_keys, rk[:f.nv]) and np.array_equal(f.order, rv[:f.nv]) and np.array_equal(f.cum, rcum[:f.nv])
        assert np.all(rk[f.nv:] == R.CULLED)
        assert int(f.totals[:256].sum()) == f.nv and int(f.totals[256:].astype(np.uint64).sum()) & R.M32 == (int(f.cum[-1]) if f.nv else 0)


def test_digit_rules_by_hand():
    # the scale: the range's last key takes digit 254 (253 where the clamp to 32 bits bites), never 255
    for rng_ in (0, 1, 2, 254, 255, 256, 1000, 1 << 24, (1 << 31) + 5, 0xFFFFFFFE):
        s = R.make_scale(True, 0, rng_)
        assert s == min(R.M32, (255 << 32) // (rng_ + 1)) and (rng_ * s) >> 32 == (254 if rng_ >= 255 else max(rng_ - 1, 0)), rng_
    assert R.make_scale(False, R.M32, 0) == R.M32
    d = R.linear_digits(np.array([10, 11, 264, 265, R.CULLED], np.uint32), 10, R.make_scale(True, 10, 265))
    assert d.tolist() == [0, 0, 253, 254, 255]
    # the table digit: the number of splitters <= key
    t = np.zeros(R.SPL_STRIDE, np.uint32)
    t[:254] = np.concatenate([[100, 200, 200, 200, 300], np.full(249, 1000)])
    t[254:258] = R.M32, 1, 50, 2000
    assert R.table_digits(np.array([50, 99, 100, 101, 199, 200, 201, 300, 999, 1000, 2000, R.CULLED], np.uint32), t).tolist() == [0, 0, 1, 1, 1, 4, 4, 5, 5, 254, 254, 255]
    # depth_split's rule: tol = (2000 - 50) >> 4 = 121
    assert [R.table_is_used(t, True, a, b) for a, b in ((50, 2000), (171, 2000), (172, 2000), (0, 2000), (50, 2121), (50, 2122), (50, 1879), (50, 1878))] == \
        [True, True, False, True, True, False, True, False]
    assert not R.table_is_used(t, False, 50, 2000) and not R.table_is_used(None, True, 50, 2000)
    t[255] = 0
    assert not R.table_is_used(t, True, 50, 2000)
    assert [R.bucket_plan(s, b) for s, b in ((7168, 0), (7168, 9), (7168, 10), (7168, 27), (7168, 28), (7168, 32), (7169, 0), (7169, 8), (7169, 9), (7169, 24), (7169, 25), (7169, 32))] == \
        [("resident", 0), ("resident", 1), ("resident", 2), ("resident", 3), ("resident", 4), ("resident", 4), ("chunked", 1), ("chunked", 1), ("chunked", 3), ("chunked", 3),
         ("chunked", 5), ("chunked", 5)]
    assert R.pass_widths(32, 5) == [7, 7, 6, 6, 6] and R.pass_widths(28, 4) == [7, 7, 7, 7] and R.pass_widths(25, 5) == [5] * 5


def test_table_a_run_leaves_and_the_sample_rule():
    rng = np.random.default_rng(11)
    fresh = np.zeros(R.SPL_STRIDE, np.uint32)
    keys = rng.integers(1000, 5000, 20000).astype(np.uint32)
    keys[:2] = 1000, 4999
    r = R.run(keys, keys, fresh, True)
    srt = np.sort(keys)
    assert r.sample is None and r.written and [int(r.table[j]) for j in (0, 1, 253)] == [int(srt[20000 // 255]), int(srt[2 * 20000 // 255]), int(srt[254 * 20000 // 255])]
    assert r.table[254:258].tolist() == [R.M32, 1, 1000, 4999] and not fresh.any()
    small = R.run(keys[:16383], keys[:16383], r.table, True)   # too few keys: only words 254 .. 257 change
    assert np.array_equal(small.table[:254], r.table[:254]) and small.table[254:258].tolist() == [R.M32, 0, int(keys[:16383].min()), int(keys[:16383].max())]
    big = np.tile(keys, 7)[:1 << 17]
    assert R.run(big[:-1], big[:-1], fresh, False).sample is None and R.run(big, big, fresh, True).sample is None and R.run(big, big, None, False).sample is None
    s = R.run(big, big, fresh, False)
    assert s.sample.nv == 2048 and np.array_equal(np.sort(big[::64][:2048]), s.sample.out_keys) and s.frame.used_table and s.sample.table[255] == 1


def by_id(cases, word):
    return [c for c in cases if word in c.id]


def test_every_named_case_is_there():
    ids = [c.id for c in P.CASES]
    assert len(ids) == len(set(ids))
    by = {}
    for c in P.CASES:
        by.setdefault(c.group, []).append(c)
    assert [c.offsets for c in by_id(P.CASES, "unaligned")] == [(1, 0), (2, 3)] and all(c.offsets == (0, 0) for c in P.CASES if "unaligned" not in c.name)
    assert set(by) == {"sizes", "resident", "chunked", "digits", "handover", "sample"}
    want_sizes = (1, 2, 63, 64, 65, 2047, 2048, 2049, 4096 + 5, 32 * 2048, 32 * 2048 + 1, 512 * 2048 + 1, 1024 * 2048, 1024 * 2048 + 1)
    assert P.SIZES == want_sizes
    assert {(c.name, c.mode) for c in by["sizes"] if "-" not in c.name} == {("n%d" % n, m) for n in want_sizes for m in ("off", "own")}
    assert {c.name.split("-")[1] for c in by["sizes"] if "-" in c.name} == {"allculled", "onefirst", "onelast", "equal", "descending", "ascending", "unaligned"}
    assert {c.name for c in by["resident"]} == {"S%d-B%d" % (s, b) for s in (1, 64, 1023, 1024, 1025, 7167, 7168) for b in (0, 1, 8, 9, 10, 18, 19, 27, 28, 32)}
    assert {c.name for c in by["chunked"]} == {"S%d-B%d" % (s, b) for s in (7169, 8192, 3 * 4096 + 1) for b in (0, 1, 8, 9, 24)} | {"linear-B25", "S9000-B32"}
    names = {c.name for c in by["digits"]}
    assert {"splitters", "word255-zero", "nv16383", "nv16384"} <= names and {"range%d" % r for r in (0, 1, 254, 255, 256, 1 << 24, 0xFFFFFFFE)} <= names
    assert {"%s%+d" % (e, s * d) for e in ("kmin", "kmax") for s in (-1, 1) for d in (P.T_TOL, P.T_TOL + 1)} <= names and P.T_TOL == (P.T_MAX - P.T_MIN) >> 4
    assert {c.mode for c in by["handover"]} == {"own", "ctx"} and all(len(c.claims) == 3 for c in by["handover"])
    assert {c.id for c in by["sample"]} == {"sample-n131071-own", "sample-n131072-own", "sample-n131072-ctx", "sample-n131072-few-visible-own"}
    # the group-table edges of sort_group_offset: blocks 32 / 33, groups 16 / 17 (GB = 16), 32 / 33 groups (direct / scanned)
    claims = {c.name: c.claims[0] for c in by["sizes"] if c.mode == "own" and "-" not in c.name}
    assert [(claims["n%d" % n]["nblocks"], claims["n%d" % n]["ngroups"], claims["n%d" % n]["scanned"]) for n in want_sizes[-5:]] == \
        [(32, 1, False), (33, 2, False), (513, 17, False), (1024, 32, False), (1025, 33, True)]
    pass_counts = {c.claims[0]["bucket0"]["passes"] for c in by["resident"]}, {c.claims[0]["bucket0"]["passes"] for c in by["chunked"]}
    assert pass_counts == ({0, 1, 2, 3, 4}, {1, 3, 5})


SMALL = [c for c in P.CASES if not (c.group == "sizes" and int(re.match(r"n(\d+)", c.name).group(1)) > (1 << 17))]
LARGE = [c for c in P.CASES if c not in SMALL]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.id)
def test_case_reaches_what_it_is_named_for(case):
    frames, table, written = case.build()
    assert case.mode != "own" or (table is not None and table.shape == (R.SPL_STRIDE,) and table.dtype == np.uint32)
    for keys, counts in frames:
        assert int(counts.max()) <= P.COUNT_MAX and (case.group in ("sizes", "sample") or keys.size < 400 or abs(float((keys == R.CULLED).mean()) - 0.25) < 0.02)
    runs = P.reference_runs(case, frames, table, written)
    P.check_claims(case, frames, runs)
    if case.group in ("resident", "chunked") and case.name.startswith("S"):   # stability shows: equal keys, many of them
        f = runs[0].frame
        assert f.buckets[0]["size"] == 1 or int((np.diff(f.out_keys[:f.buckets[0]["size"]].astype(np.int64)) == 0).sum()) >= f.buckets[0]["size"] // 4
    if case.name == "splitters":   # keys on, below and above every distinct splitter; runs of equal splitters leave empty buckets
        f, spl, vis = runs[0].frame, np.unique(table[:254]), frames[0][0]
        assert all(np.isin([s - 1, s, s + 1], vis).all() for s in spl) and vis.min() < table[0] and vis[vis != R.CULLED].max() > table[253]
        assert spl.size == 156 and int(f.totals[101:140].sum()) == 0 and f.totals[100] and f.totals[140]


@pytest.mark.parametrize("case", LARGE, ids=lambda c: c.id)
def test_large_size_case_is_what_it_claims(case):
    """(the full restatement of these runs with the GPU test; here only the sizes' arithmetic and the scan's wrap)"""
    (keys, counts), = case.build()[0]
    claim = case.claims[0]
    nb = (keys.size + R.DS_TILE - 1) // R.DS_TILE
    ng = (nb + R.SORT_GROUP_BLOCKS - 1) // R.SORT_GROUP_BLOCKS
    assert (nb, ng, ng > R.SORT_DIRECT_GROUPS) == (claim["nblocks"], claim["ngroups"], claim["scanned"])
    vis = keys != R.CULLED
    assert int(counts[vis].astype(np.uint64).sum()) > 1 << 32   # cum wraps
    assert 0.7 < vis.mean() < 0.8
