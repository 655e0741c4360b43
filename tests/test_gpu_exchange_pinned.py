"""The mask-keyed gradient exchange (exchange.hip; step_flag_exchange and step_grad_exchange in train.hip), row for row and bit for
bit, in one process.  Every multi-GPU step takes this path by default, and before this file only end-to-end trajectories under
util.assert_adam_close saw it: one dropped or misplaced row moves a few entries by at most lr and passes there.

The lever is bh_grad_hook with exchange_mode = 1 (SplatTrainer: pg set, sparse_exchange = True).  The step then calls the hook
    1. in front of the backward, with the base of the exchange buffer
           visible[N] | v_transforms[10N] | v_sh[3CN] | v_raw_opac[N] | refine_weight[N]     (each section padded to 4 floats)
       and sum_count = pad4(N): "sum the visible flags over the ranks".  The library then lists U = { i : summed flag > 0 },
    2. behind the backward, with  rows = |U|,  k = 11 + 3C (+ 1, the refine weight, on a tile-partitioned frame):
           rows == 0          no second call
           2 rows <= N        a compact block of its own, sum_count = rows k, row r = (v_transforms | v_sh | v_raw_opac [| refine])
                              of splat U[r]; the library scatters the block back to the rows of U behind the call
           else               the dense span from v_transforms on: sum_count = o_ref - o_tr, or exch_count - o_tr with the refine column.
brush_amd.host._view of either pointer is writable, so a hook plays any number of other ranks: on call 1 it adds flags P of the
test's choosing — that decides U —, on call 2 it compares the compact block with the dense rows the gather copied from (behind the
first pointer, on the device, the verdict is read after the step) and adds a second rank's payload Q to it, or replaces it by Q.
Every Context here is the default one (ctx.uses_torch_stream, asserted): the library's kernels and the hook's torch work share one
stream, nothing synchronises inside the keyed trainer's hook.

The reference is numpy: U = flatnonzero(V0 + P > 0) from the flags V0 the hook saw, the path from 2 |U| <= N, the sequence of
(pointer offset, sum_count) the hook must be given, stats().exchange_rows.  The twin is the same step from the same start with
sparse_exchange = False: ONE hook call over the dense buffer, in which the summed flags are written and Q is added to (written
over) the dense rows of U with the same float32 g + q, every other row left alone.  The twin's update is pinned to the oracle by
test_gpu_update_pinned.py; after each of 3 steps the keyed trainer must equal the twin in parameters, the six moments, the three
statistics and the whole exchange buffer, bit for bit.  P and Q change from step to step (the union grows, then shrinks: the index
list and the compact slot are reused at other sizes).  The frame is ONE 16 x 16 tile (test_gpu_update_sparse.py): at most one
(splat, tile) pair per splat, so the backward's atomics add once into a zero and two runs agree to the bit.

Q: word (splat i, column j) of step t is +-10^(-3 u), u = (i k + j + t / 4) / (N k) in [0, 1), the sign alternating with i k + j:
finite, 1e-3 < |q| <= 1, every word distinct (checked), so a misplaced word names where it came from.  The refine column is |q|.

Cases (exchange.hip: EX_WG = 256 threads a block, EX_EPT = 16 consecutive splats a thread, EX_TILE = 4096 splats a block, waves of
64 threads = 1024 splats, EX_SELF_SPINE_MAX = 1024 blocks for the place kernel's own spine):
  listing   SH degree 0, camera mode, n in {2, 17, 4095, 4096, 4097, 3 * 4096 + 5}; all but a thirty-seventh of the splats behind
            the camera, so P decides U.  P: splat 0 alone; n - 1 alone; both neighbours of every 16-splat edge (which holds every
            1024- and 4096-splat edge); the 1024-splat edges alone; the 4096 edges alone; one thread's 16 splats beside empty threads
            (at a thread, a wave and a block edge); blocks with members around a block with none; a seeded 20 %; and P = 0 on a
            scene whose own flags cover a third (no splat hidden, see layouts).
  threshold n in {300, 301}, camera and tile mode: rows = n // 2 exactly (compact at both sizes), rows = n // 2 + 1 (the dense
            fallback, exchange_rows 0), rows = 0 (all splats behind the camera, P = 0: one hook call).
  layouts   n = 300, SH degree 0, 1, 3, 4 (k = 14, 23, 59, 86; 15, 24, 60, 87 with the refine column), camera and tile mode, Q
            added and Q written; no splat is hidden and the means are pulled towards the axis (x, y times 0.91), so that V0 covers
            30 - 45 % of the splats at every step (asserted) and the gathered rows are real gradients.
            Tile mode: a do-nothing image hook on the batch (tr.batch_patch), the whole tile-row window, strip_loss = 0,
            grad_scale 1; `visible` is clamped to 1 by the update.
  spines    n = 1024 * 4096 (nb = 1024, the largest self-spine) and n = 1024 * 4096 + 1 (nb = 1025: union_spine_kernel takes five
            passes, the last with one live element; the last block holds one splat).  Block b has (7 b) mod 13 members at seeded
            places, every 13th block none, n - 1 and the last block's first splat always; one step, Q written.
  communicator  n = 6000, SH degree 2, three views, 5 steps: a one-rank communicator with option force_exchange = 1 (side stream,
            readback event, compact path, degenerate collectives) and an identity hook in keyed mode, each against a plain trainer.
test_the_cases_are_what_they_claim (no GPU) computes U of every case from its P alone and checks the path and every edge above."""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest
import torch

from brush_amd import synth
import update_ref as ur
import util
from test_gpu_update_pinned import MEDIAN, _assert_bits, _download, _offsets, _pad4
from test_gpu_update_sparse import _scene, _views

gpu = pytest.mark.gpu   # (per test: the guard needs no GPU)

W = H = 16
STEPS = 3
# brush_amd/csrc/exchange.hip (test_the_cases_are_what_they_claim reads them there)
EX_WG = 256                        # constexpr int EX_WG
EX_EPT = 16                        # constexpr int EX_EPT: consecutive splats per thread of union_place_kernel
EX_TILE = EX_WG * EX_EPT           # constexpr int EX_TILE: splats per block
EX_WAVE = 64 * EX_EPT              # splats per wave (ex_wave_incl_scan: 64 lanes)
EX_SELF_SPINE_MAX = 4 * EX_WG      # constexpr uint32_t EX_SELF_SPINE_MAX: blocks up to which union_place_kernel<true> runs


def _k(words, tile):
    return 11 + words + (1 if tile else 0)


# ---------------------------------------------------------------------------------------------------------------------------
# the other ranks: flags P and payload Q
# ---------------------------------------------------------------------------------------------------------------------------
def _flags(n, ids):
    """P: the splats `ids` carry 1, 2 or 3 (a sum over other ranks), everyone else 0."""
    p = np.zeros(n, np.float32)
    ids = np.asarray(ids, np.int64)
    ids = ids[(ids >= 0) & (ids < n)]
    p[ids] = (ids % 3 + 1).astype(np.float32)
    return p


def _random_ids(n, share, seed):
    return np.sort(np.random.default_rng([0xE7, n, seed]).permutation(n)[:max(1, int(round(share * n)))])


def _edge_ids(n, period):
    e = np.arange(period, n, period)
    return np.concatenate([e - 1, e])


def _pattern(name, n):
    if name == "first":
        return np.array([0])
    if name == "last":
        return np.array([n - 1])
    if name == "edges16":
        return _edge_ids(n, EX_EPT)
    if name == "edges1024":
        return _edge_ids(n, EX_WAVE)
    if name == "edges4096":
        return _edge_ids(n, EX_TILE)
    if name == "thread":   # threads 1, 63 and 255 of block 0 full, their neighbours empty
        return np.concatenate([np.arange(t * EX_EPT, (t + 1) * EX_EPT) for t in (1, 63, 255)])
    if name == "gap":      # members in blocks 0, 2 and 3, none in block 1
        return np.concatenate([[5, 4000, EX_TILE - 1], 2 * EX_TILE + np.array([0, 17, 4095]), [3 * EX_TILE, n - 1]])
    if name == "random":
        return _random_ids(n, 0.2, 1)
    if name == "own":
        return np.zeros(0, np.int64)
    raise KeyError(name)


def _q_rows(ids, k, n, step, tile):
    """The payload rows of the splats `ids` (module docstring)."""
    w = np.asarray(ids, np.int64)[:, None] * k + np.arange(k, dtype=np.int64)[None, :]
    q = 10.0 ** (-3.0 * (w + 0.25 * step) / float(n * k))
    q = np.where(w % 2 == 0, q, -q).astype(np.float32)
    if tile:
        q[:, -1] = np.abs(q[:, -1])
    return q


class Case:
    """kind, n, SH degree, tile mode, whether Q replaces the block, the declared path of each step, and flags(step, V0) -> P."""
    def __init__(self, kind, name, n, sh_degree=0, tile=False, replace=False, paths=("compact",) * STEPS, hidden="most"):
        self.kind, self.name, self.n, self.sh_degree, self.tile, self.replace, self.paths, self.hidden = kind, name, n, sh_degree, tile, replace, paths, hidden
        self.words = 3 * (sh_degree + 1) ** 2
        self.k = _k(self.words, tile)
        self.steps = len(paths)

    @property
    def id(self):
        return "%s-%s-n%d-sh%d-%s-%s" % (self.kind, self.name, self.n, self.sh_degree, "tile" if self.tile else "camera", "write" if self.replace else "add")

    def flags(self, step, v0):
        n = self.n
        if self.kind == "listing":
            if self.name == "random":   # 20 %, then another 30 %, then 10 %
                return _flags(n, _random_ids(n, (0.2, 0.3, 0.1)[step - 1], step))
            ids = _pattern(self.name, n)
            if step == 2 and self.name != "own":   # the union grows (at n = 2 to both splats: the dense span), then shrinks again
                ids = np.concatenate([ids, np.arange(2) if n == 2 else _random_ids(n, 0.2, 7)])
            return _flags(n, ids)
        if self.kind == "threshold":
            if self.name == "zero":
                return np.zeros(n, np.float32)
            target = n // 2 + (1 if self.name == "over" else 0)
            own = np.flatnonzero(v0 > 0)
            rest = np.setdiff1d(np.random.default_rng([0x7E, n, step]).permutation(n), own, assume_unique=True)   # (keeps the permutation's order)
            assert own.size <= target, ("the scene's own flags leave no room to choose the union's size", own.size, target)
            return _flags(n, rest[:target - own.size])
        if self.kind == "layouts":
            return _flags(n, _random_ids(n, (0.04, 0.06, 0.02)[step - 1], 10 + step))
        if self.kind == "spines":
            return _flags(n, _spine_ids(n))
        raise KeyError(self.kind)

    def scene(self):
        if self.kind == "spines":
            return _big_scene(self.n)
        sc = _scene(self.n, self.sh_degree)
        i = np.arange(self.n)
        if self.hidden == "none":   # _scene's own flags cover 26 - 35 % of 300 splats; pulled towards the axis, 30 - 45 % (asserted on the GPU)
            sc["transforms"][:, :2] *= np.float32(INWARD)
            return sc
        hide = {"most": (i + 13) % 37 != 0, "all": np.ones(self.n, bool)}[self.hidden]
        sc["transforms"][hide, :3] = np.array([0.0, 0.0, -5.0], np.float32)   # behind every camera of _views
        return sc


INWARD = 0.91


def _spine_ids(n):
    """Block b: (7 b) mod 13 members, one in each of its first strata of 341 splats, at a seeded place; n - 1 and the last block's first."""
    nb = (n + EX_TILE - 1) // EX_TILE
    b = np.arange(nb, dtype=np.int64)
    count = (7 * b) % 13
    place = np.arange(12, dtype=np.int64)[None, :] * 341 + np.random.default_rng([0x5B, n]).integers(0, 341, (nb, 12))
    ids = (b[:, None] * EX_TILE + place)[np.arange(12)[None, :] < count[:, None]]
    return np.unique(np.concatenate([ids[ids < n], [n - 1, (nb - 1) * EX_TILE]]))


def _big_scene(n):
    """Splats 0 .. 255 are _scene(256, 0); every other one sits behind the camera."""
    front = _scene(256, 0)
    tr = np.empty((n, 10), np.float32)
    tr[:] = np.array([0.0, 0.0, -5.0, 1.0, 0.0, 0.0, 0.0, -2.3, -2.3, -2.3], np.float32)
    tr[:256] = front["transforms"]
    sh = np.full((n, 1, 3), 0.5, np.float32)
    sh[:256] = front["sh"]
    op = np.zeros(n, np.float32)
    op[:256] = front["raw_opac"]
    return {"transforms": tr, "sh": sh, "raw_opac": op}


def _listing_cases():
    out = []
    names = {2: ("first", "last", "random"), 17: ("first", "last", "edges16", "random"),
             4095: ("first", "last", "edges16", "edges1024", "thread", "random"),
             4096: ("first", "last", "edges16", "edges1024", "thread", "random"),
             4097: ("first", "last", "edges16", "edges1024", "edges4096", "thread", "random"),
             3 * 4096 + 5: ("first", "last", "edges16", "edges1024", "edges4096", "thread", "gap", "random")}
    for n, ns in names.items():
        for j, name in enumerate(ns):
            paths = ("compact", "dense", "compact") if n == 2 and name != "random" else ("compact",) * STEPS
            out.append(Case("listing", name, n, replace=bool(j % 2), paths=paths))
    out.append(Case("listing", "own", 4097, hidden="none"))
    return out


def _threshold_cases():
    out = []
    for n in (300, 301):
        for tile in (False, True):
            out.append(Case("threshold", "half", n, tile=tile, hidden="none", replace=tile))
            out.append(Case("threshold", "over", n, tile=tile, hidden="none", replace=not tile, paths=("dense",) * STEPS))
            out.append(Case("threshold", "zero", n, tile=tile, hidden="all", paths=("none",) * STEPS))
    return out


def _layout_cases():
    return [Case("layouts", "rows", 300, sh_degree=d, tile=tile, replace=replace, hidden="none")
            for d in (0, 1, 3, 4) for tile in (False, True) for replace in (False, True)]


def _spine_cases():
    return [Case("spines", "blocks", EX_SELF_SPINE_MAX * EX_TILE + extra, replace=True, paths=("compact",)) for extra in (0, 1)]


SMALL_CASES = _listing_cases() + _threshold_cases() + _layout_cases()
SPINE_CASES = _spine_cases()


def _path(rows, n):
    return "none" if rows == 0 else ("compact" if 2 * rows <= n else "dense")


# ---------------------------------------------------------------------------------------------------------------------------
# the guard: the cases are what they claim (no GPU)
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_cases_are_what_they_claim():
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "brush_amd", "csrc")
    with open(os.path.join(csrc, "exchange.hip")) as f:
        src = f.read()
    consts = dict(re.findall(r"constexpr (?:int|uint32_t) (EX_\w+) = ([^;]+);", src))
    assert consts == {"EX_WG": "256", "EX_EPT": "16", "EX_TILE": "EX_WG * EX_EPT", "EX_SELF_SPINE_MAX": "4 * EX_WG"}, consts
    assert (EX_WG, EX_EPT, EX_TILE, EX_WAVE, EX_SELF_SPINE_MAX) == (256, 16, 4096, 1024, 1024)
    assert "nb <= EX_SELF_SPINE_MAX" in src   # which spine a size takes
    assert len({c.id for c in SMALL_CASES + SPINE_CASES}) == len(SMALL_CASES + SPINE_CASES)
    assert {c.n for c in SMALL_CASES if c.kind == "listing"} == {2, 17, 4095, 4096, 4097, 3 * 4096 + 5}
    assert {(c.sh_degree, c.tile, c.replace) for c in SMALL_CASES if c.kind == "layouts"} == {(d, t, r) for d in (0, 1, 3, 4) for t in (False, True) for r in (False, True)}
    assert sorted({c.k for c in SMALL_CASES if c.kind == "layouts"}) == [14, 15, 23, 24, 59, 60, 86, 87]
    touched = {}
    for c in SMALL_CASES + SPINE_CASES:
        sizes = []
        for step in range(1, c.steps + 1):
            p = c.flags(step, np.zeros(c.n, np.float32))
            assert p.shape == (c.n,) and p.dtype == np.float32 and set(np.unique(p)) <= {0.0, 1.0, 2.0, 3.0}
            u = np.flatnonzero(p > 0)
            sizes.append(u.size)
            want = "compact" if c.name == "own" else c.paths[step - 1]   # (P = 0: the scene's own flags are the union, judged on the GPU)
            assert _path(u.size, c.n) == want or c.name == "own", (c.id, step, u.size)
            if u.size == 0:
                continue
            q = _q_rows(u, c.k, c.n, step, c.tile)
            assert np.isfinite(q).all() and float(np.abs(q).min()) >= 1e-3 and float(np.abs(q).max()) <= 1.0
            assert np.unique(q).size == q.size, (c.id, "the payload's words are not distinct")
            if step == 1:
                touched.setdefault((c.kind, c.n), []).append((c.name, u))
        if c.kind == "listing" and c.name != "own" and c.n > 17:
            assert sizes[1] > sizes[0] and sizes[2] < sizes[1], (c.id, sizes)   # the union grows, then shrinks
        if c.kind == "threshold" and c.name != "zero":
            assert sizes == [c.n // 2 + (c.name == "over")] * STEPS
    # every edge the docstring names has a member on both sides, in a case of its own, at every listing size where it exists
    for n in (17, 4095, 4096, 4097, 3 * 4096 + 5):
        by = dict(touched[("listing", n)])
        assert by["first"].tolist() == [0] and by["last"].tolist() == [n - 1]
        for name, period in (("edges16", EX_EPT), ("edges1024", EX_WAVE), ("edges4096", EX_TILE)):
            edges = np.arange(period, n, period)
            if edges.size == 0:
                assert name not in by
                continue
            assert np.isin(edges, by[name]).all() and np.isin(edges - 1, by[name]).all(), (n, name)
            assert np.isin(edges, by["edges16"]).all() and np.isin(edges - 1, by["edges16"]).all()
        if "thread" in by:
            t = by["thread"] // EX_EPT
            # full threads beside empty ones (at n = 4095 the block's last thread stops one splat short)
            assert set(t) == {1, 63, 255} and all(int((t == x).sum()) == min(EX_EPT, n - x * EX_EPT) for x in (1, 63, 255))
    gap = dict(touched[("listing", 3 * 4096 + 5)])["gap"] // EX_TILE
    assert set(gap) == {0, 2, 3}   # block 1 is empty between blocks with members
    assert 4095 in dict(touched[("listing", 4097)])["edges4096"] and 4096 in dict(touched[("listing", 4097)])["edges4096"]
    for c, nb in zip(SPINE_CASES, (EX_SELF_SPINE_MAX, EX_SELF_SPINE_MAX + 1)):
        assert (c.n + EX_TILE - 1) // EX_TILE == nb
        u = np.flatnonzero(c.flags(1, np.zeros(c.n, np.float32)) > 0)
        per_block = np.bincount(u // EX_TILE, minlength=nb)
        want = (7 * np.arange(nb)) % 13
        assert np.array_equal(per_block[:-1], want[:-1]) and per_block[-1] >= 1
        assert (per_block == 0).sum() >= 50 and u[-1] == c.n - 1 and (nb - 1) * EX_TILE in u and 2 * u.size < c.n // 100


# ---------------------------------------------------------------------------------------------------------------------------
# the two trainers
# ---------------------------------------------------------------------------------------------------------------------------
class _Plan:
    """One step's other ranks: P, U, Q — on the host and on the device."""
    def __init__(self, case, step, v0, dev):
        self.v0 = v0
        self.p = case.flags(step, v0)
        self.u = np.flatnonzero(v0 + self.p > 0)
        self.rows = int(self.u.size)
        self.q = _q_rows(self.u, case.k, case.n, step, case.tile)
        self.p_dev = torch.from_numpy(self.p).to(dev)
        self.u_dev = torch.from_numpy(self.u).to(dev)
        self.q_dev = torch.from_numpy(self.q).to(dev)


class _Side:
    """A trainer on a context of its own whose steps go through a hook of this file: keyed (sparse_exchange) or the dense twin."""
    def __init__(self, ba, dev, case, sc, keyed):
        from brush_amd import _ffi
        self.case, self.dev, self.keyed = case, dev, keyed
        self.o_tr, self.o_sh, self.o_op, self.o_ref, self.total = _offsets(case.n, case.words)
        self.ctx = ba.Context(dev)
        assert self.ctx.uses_torch_stream   # the hook's work is ordered by the stream (module docstring)
        self.spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
        self.tr = tr = ba.SplatTrainer(ba.TrainConfig(mean_noise_weight=0.0), median_scene_scale=MEDIAN, ctx=self.ctx)
        tr.pg = object()   # (only its presence matters: the step takes the hook below, partition "cameras")
        tr._world = 1      # grad_scale 1
        tr.sparse_exchange = keyed
        tr._hook = self._c_hook = _ffi.GRAD_HOOK(self._keyed_hook if keyed else self._twin_hook)
        if case.tile:   # a do-nothing image hook: the frame stays whole, the step runs in tile mode
            self._img_hook = _ffi.IMAGE_HOOK(lambda _u, _p, _h, _w, _r0, _r1: 0)

            def patch(b):
                b.image_hook = C.cast(self._img_hook, C.c_void_p)
                b.strip_loss = 0
            tr.batch_patch = patch
        self.errors, self.calls, self.plan, self.make_plan = [], [], None, None
        self.base = self.v0_dev = self.gather_bad = self.gathered = None

    def close(self):
        self.ctx.close()

    def _sections(self, buf):
        n, words = self.case.n, self.case.words
        return (buf[self.o_tr:self.o_tr + n * 10].view(n, 10), buf[self.o_sh:self.o_sh + n * words].view(n, words),
                buf[self.o_op:self.o_op + n], buf[self.o_ref:self.o_ref + n])

    def _rows_of(self, buf, u):
        """dense[U] laid out as the compact block"""
        g_tr, g_sh, g_op, g_ref = self._sections(buf)
        cols = [g_tr[u], g_sh[u], g_op[u, None]] + ([g_ref[u, None]] if self.case.tile else [])
        return torch.cat(cols, 1)

    def _other_rank_dense(self, buf, plan):
        """The second rank's rows, summed into (written over) the dense rows of U; every other row is left alone."""
        if plan.rows == 0:
            return
        words, u, q = self.case.words, plan.u_dev, plan.q_dev
        parts = list(zip(self._sections(buf), (q[:, :10], q[:, 10:10 + words], q[:, 10 + words], q[:, -1])))
        for sec, qs in parts[:4 if self.case.tile else 3]:
            sec[u] = qs if self.case.replace else sec[u] + qs

    def _view(self, ptr, count):
        from brush_amd.host import _view
        return _view(ptr, (count,), torch.float32, self.dev)

    def _twin_hook(self, _user, ptr, count):
        try:
            ptr, count, n = int(ptr), int(count), self.case.n
            self.calls.append((0, count))
            self.base = ptr
            assert count == (self.total if self.case.tile else self.o_ref), (count, self.total, self.o_ref)
            buf = self._view(ptr, self.total)
            self.plan = plan = self.make_plan(buf[:n].cpu().numpy().copy())   # (the twin may wait for its flags: P can depend on them)
            buf[:n] += plan.p_dev
            self._other_rank_dense(buf, plan)
            return 0
        except Exception as e:  # never unwind across the C boundary
            self.errors.append(e)
            return 1

    def _keyed_hook(self, _user, ptr, count):
        try:
            ptr, count, case, plan = int(ptr), int(count), self.case, self.plan
            n, k = case.n, case.k
            if not self.calls:
                self.base = ptr
            assert (ptr - self.base) % 4 == 0
            self.calls.append(((ptr - self.base) // 4, count))
            if len(self.calls) == 1:
                assert count == _pad4(n), (count, n)
                flags = self._view(ptr, n)
                self.v0_dev = flags.clone()
                flags += plan.p_dev
            elif len(self.calls) == 2 and ptr == self.base + 4 * self.o_tr:   # the dense span
                assert count == (self.total if case.tile else self.o_ref) - self.o_tr, count
                self._other_rank_dense(self._view(self.base, self.total), plan)
            elif len(self.calls) == 2:                                          # the compact block
                assert count == plan.rows * k and plan.rows > 0, (count, plan.rows, k)
                assert not (self.base - 4 * count < ptr < self.base + 4 * self.total), "the compact block overlaps the exchange buffer"
                block = self._view(ptr, count).view(plan.rows, k)
                self.gathered = self._rows_of(self._view(self.base, self.total), plan.u_dev)
                self.gather_bad = block.view(torch.int32) != self.gathered.view(torch.int32)
                if case.replace:
                    block.copy_(plan.q_dev)
                else:
                    block += plan.q_dev
            return 0
        except Exception as e:  # never unwind across the C boundary
            self.errors.append(e)
            return 1

    def step(self, ba, gt, cam):
        self.calls, self.gather_bad, self.gathered, self.v0_dev = [], None, None, None
        self.tr.step(ba.SceneBatch(gt, cam), self.spl)

    def buffer(self):
        """The exchange buffer as the step left it."""
        return self._view(self.base, self.total).clone()


def _run_case(ba, dev, case, judge_v0=None):
    """case.steps steps of the twin and of the keyed trainer in lockstep; every claim of the module docstring after every step."""
    sc = case.scene()
    gt = torch.from_numpy(synth.synthetic_gt_packed(W, H).view(np.int32)).to(dev)
    cams = _views(W, H, 3)
    n, k = case.n, case.k
    twin, keyed = _Side(ba, dev, case, sc, False), _Side(ba, dev, case, sc, True)
    try:
        shares, nonzero_rows = [], []
        for t in range(1, case.steps + 1):
            cam = util.hip_camera(ba, cams[(t - 1) % len(cams)])
            twin.make_plan = lambda v0, _t=t: _Plan(case, _t, v0, dev)
            twin.step(ba, gt, cam)
            twin.ctx.sync()
            assert not twin.errors, twin.errors
            keyed.plan = plan = twin.plan
            keyed.step(ba, gt, cam)
            keyed.ctx.sync()
            assert not keyed.errors, keyed.errors
            what = "%s step %d" % (case.id, t)
            # the flags the keyed hook saw are the twin's; from them, everything else
            v0 = keyed.v0_dev.cpu().numpy()
            assert np.array_equal(v0, plan.v0) and set(np.unique(v0)) <= {0.0, 1.0}, what
            shares.append(float((v0 > 0).mean()))
            u = np.flatnonzero(v0 + plan.p > 0)
            rows, path = int(u.size), _path(int(u.size), n)
            print("%s: own flags %d of %d, union %d rows, %s" % (what, int((v0 > 0).sum()), n, rows, path))
            assert path == case.paths[t - 1], (what, rows, "the case does not take the path it claims")
            if case.name == "zero":
                assert not (v0 > 0).any(), what
            # 1. union and counts
            second = {"none": [], "compact": [rows * k], "dense": [(keyed.total if case.tile else keyed.o_ref) - keyed.o_tr]}[path]
            assert [c for _, c in keyed.calls] == [_pad4(n)] + second, (what, keyed.calls)
            assert keyed.calls[0][0] == 0 and (path != "dense" or keyed.calls[1][0] == keyed.o_tr), (what, keyed.calls)
            assert path != "compact" or not (-rows * k < keyed.calls[1][0] < keyed.total), (what, keyed.calls)
            assert keyed.tr.stats(keyed.ctx).exchange_rows == (rows if path == "compact" else 0), what
            assert twin.tr.stats(twin.ctx).exchange_rows == 0 and len(twin.calls) == 1, what
            # 2. gather
            if path == "compact":
                bad = keyed.gather_bad.cpu().numpy()
                if bad.any():
                    r, j = np.argwhere(bad)[0]
                    raise AssertionError((what, "gather: %d words differ, first at row %d (splat %d) column %d" % (int(bad.sum()), r, u[r], j)))
                nonzero_rows.append(int((keyed.gathered != 0).any(1).sum().item()))
            # 3. scatter, and what the update saw
            d = ur.first_difference(keyed.buffer().cpu().numpy(), twin.buffer().cpu().numpy())
            assert d is None, (what, "exchange buffer", d, _name_word(keyed, d))
            _assert_bits(_download(keyed.spl, keyed.tr), _download(twin.spl, twin.tr), what)
        if judge_v0 is not None:
            judge_v0(shares, nonzero_rows)
        return shares
    finally:
        twin.close()
        keyed.close()


def _name_word(side, d):
    """Which section and splat a flat index of the exchange buffer (ur.first_difference's line) lies in."""
    i = int(re.search(r"flat index (\d+)", d).group(1))
    for name, o, width in (("refine", side.o_ref, 1), ("v_raw_opac", side.o_op, 1), ("v_sh", side.o_sh, side.case.words), ("v_transforms", side.o_tr, 10), ("visible", 0, 1)):
        if i >= o:
            return "%s of splat %d, element %d" % (name, (i - o) // width, (i - o) % width)


# ---------------------------------------------------------------------------------------------------------------------------
# the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", SMALL_CASES, ids=lambda c: c.id)
def test_keyed_exchange_equals_the_reference_and_the_dense_twin(dev, case):
    import brush_amd as ba

    def judge(shares, nonzero_rows):
        if case.hidden == "none" and case.kind != "threshold":   # the gathered rows are real gradients, spread over the splats
            assert all(0.30 <= s <= 0.45 for s in shares), shares
            assert min(nonzero_rows) >= 0.1 * case.n, nonzero_rows
        if case.hidden == "most":                                 # P decides U
            assert max(shares) <= 0.05, shares
    _run_case(ba, dev, case, judge)


@gpu
@pytest.mark.parametrize("case", SPINE_CASES, ids=lambda c: c.id)
def test_both_spines_at_their_boundary(dev, case):
    """nb = EX_SELF_SPINE_MAX (union_place_kernel<true>) and nb = EX_SELF_SPINE_MAX + 1 (union_spine_kernel, five passes, and
    union_place_kernel<false>).  The gathered rows are mostly zero here; the weight lies on the counts and the scatter."""
    import brush_amd as ba
    t0 = time.perf_counter()
    shares = _run_case(ba, dev, case)
    torch.cuda.empty_cache()   # (one pair of 4 M-splat trainers at a time)
    print("%s: %.1f s" % (case.id, time.perf_counter() - t0))
    assert 0 < shares[0] < 1e-3   # a few of splats 0 .. 255 are in the frame


STEPS_COMM = 5
_PLAIN = {}


def _comm_problem(ba, dev, options, setup):
    """STEPS_COMM steps of the one-tile problem, n = 6000, SH degree 2, three views in turn, seeded trainer (jittered background, no
    mean noise); setup(ctx) -> keyword arguments of the trainer, then an optional function of the trainer.  -> final tensors, exchange_rows per step."""
    n, sh_degree = 6000, 2
    sc, cams = _scene(n, sh_degree), _views(W, H, 3)
    ctx = ba.Context(dev, options=options)
    try:
        assert ctx.uses_torch_stream
        kwargs, prepare = setup(ctx)
        gt = torch.from_numpy(synth.synthetic_gt_packed(W, H).view(np.int32)).to(dev)
        spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
        tr = ba.SplatTrainer(ba.TrainConfig(mean_noise_weight=0.0), median_scene_scale=MEDIAN, ctx=ctx, seed=77, **kwargs)
        if prepare is not None:
            prepare(tr)
        rows = []
        for s in range(STEPS_COMM):
            tr.step(ba.SceneBatch(gt, util.hip_camera(ba, cams[s % len(cams)])), spl)
            ctx.sync()
            rows.append(int(tr.stats(ctx).exchange_rows))
        return _download(spl, tr), rows
    finally:
        ctx.close()


def _plain(ba, dev):
    """The single-GPU step, once: zero-filled gradients (option zero_grads), so that no -0.0 row mark stands in m2_sh."""
    if "z" not in _PLAIN:
        _PLAIN["z"], rows = _comm_problem(ba, dev, {"zero_grads": 1}, lambda ctx: ({}, None))
        assert rows == [0] * STEPS_COMM
        assert float(np.abs(_PLAIN["z"]["m2_t"]).sum(1).astype(bool).mean()) > 0.02   # the steps trained some splats
    return _PLAIN["z"]


@gpu
def test_one_rank_communicator_walks_the_keyed_path_and_leaves_the_plain_steps_bits(dev):
    """force_exchange = 1 on a one-rank communicator: the flag sum, the union listing and the count's readback run on the
    communicator's side stream, the compact block is gathered, 'summed' and scattered on the ctx stream behind the readback event.
    Any missing hand-over between the two streams would let the update read rows the scatter has not written."""
    import brush_amd as ba

    def setup(ctx):
        ctx.comm_init(0, 1, ba.Context.comm_unique_id())
        return dict(native_comm=True, sparse_exchange=True), None
    got, rows = _comm_problem(ba, dev, {"force_exchange": 1}, setup)
    print("exchange_rows per step:", rows)
    assert all(0 < r <= 3000 for r in rows), rows
    _assert_bits(got, _plain(ba, dev), "one-rank communicator against the plain trainer")


@gpu
def test_identity_hook_in_keyed_mode_leaves_the_plain_steps_bits(dev):
    import brush_amd as ba
    from brush_amd import _ffi
    seen = []

    def hook(_user, _ptr, count):
        seen.append(int(count))
        return 0
    c_hook = _ffi.GRAD_HOOK(hook)

    def prepare(tr):
        tr.pg, tr._world, tr._hook, tr.sparse_exchange = object(), 1, c_hook, True
    got, rows = _comm_problem(ba, dev, None, lambda ctx: ({}, prepare))
    print("exchange_rows per step:", rows)
    assert all(0 < r <= 3000 for r in rows), rows
    assert seen == [c for r in rows for c in (_pad4(6000), r * _k(27, False))], seen
    _assert_bits(got, _plain(ba, dev), "identity hook, keyed, against the plain trainer")
