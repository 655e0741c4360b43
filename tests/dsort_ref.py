"""The fused depth sort (brush_amd/csrc/depth_sort.hip) restated in numpy and Python integers: what one call of depth_sort_scan
leaves behind — the order, the scan, the digit totals of the split and the splitter table — and which path every bucket takes.
Nothing here is taken from the kernels' output; test_dsort_ref.py ties it to the oracle's radix_argsort + prefix_sum.

A frame:   keys [n] uint32 (culled = 0xFFFFFFFF), counts [n] uint32, the frame's key range as K1 leaves it (minmax_of).
A table:   uint32 [SPL_STRIDE]: [0..253] splitters, ascending | [254] 0xFFFFFFFF | [255] != 0: valid | [256] kmin, [257] kmax of the
           frame that wrote it | [258..259] never touched.  None: no table at all (option dsort_splitters = 0).
run(...)   one depth_sort_scan: the sample run where the rules ask for one, then the frame itself."""
import numpy as np

CULLED = 0xFFFFFFFF
DS_TILE = 2048              # constexpr int DS_TILE = DS_WG * DS_KPT
FAST_CAP = 7168             # constexpr int FAST_CAP (BK_WG = 1024)
COUNTER_SLOTS = 128         # context.h
SPL_WORDS = 258
SPL_STRIDE = 260            # context.h DSORT_SPL_STRIDE
SPL_MIN_KEYS = 16384
SPL_SAMPLE_STRIDE = 64
SPL_SAMPLE_MIN_N = 1 << 17
SPL_SAMPLE_MIN_KEYS = 1024
SORT_GROUP_BLOCKS = 32      # context.h
SORT_DIRECT_GROUPS = 32     # context.h: more groups than this take the scanned group table
M32 = 0xFFFFFFFF


def minmax_of(keys):
    """K1's [COUNTER_SLOTS][2] (max key, max ~key over the visible keys of a slot; zeros: neutral): key i reports to slot i % 128."""
    keys = np.asarray(keys, np.uint32)
    out = np.zeros(2 * COUNTER_SLOTS, np.uint32)
    for s in range(COUNTER_SLOTS):
        k = keys[s::COUNTER_SLOTS]
        k = k[k != CULLED]
        if k.size:
            out[2 * s] = k.max()
            out[2 * s + 1] = (~k).max()
    return out


def key_range(minmax):
    """-> (any_visible, kmin, kmax) as make_split reads them."""
    mm = np.asarray(minmax, np.uint32)
    kmax, nmin = int(mm[0::2].max()), int(mm[1::2].max())
    return nmin != 0, (~nmin) & M32, kmax


def make_scale(any_visible, kmin, kmax):
    """The largest scale with (range * scale) >> 32 <= 254 — make_split, with its - 1 correction."""
    rng = kmax - kmin if any_visible else 0
    scale = min(M32, (255 << 32) // (rng + 1))
    if (rng * scale) >> 32 > 254:
        scale -= 1
    return scale


def linear_digits(keys, kmin, scale):
    keys = np.asarray(keys, np.uint32)
    d = np.full(keys.size, 255, np.int64)
    v = keys != CULLED
    # (key - kmin) < 2^32 and scale < 2^32: the product fits 64 bits
    prod = (keys[v].astype(np.uint64) - np.uint64(kmin)) * np.uint64(scale)
    d[v] = np.minimum(254, (prod >> np.uint64(32)).astype(np.int64))
    return d


def table_digits(keys, table):
    """Number of splitters <= key."""
    keys = np.asarray(keys, np.uint32)
    d = np.full(keys.size, 255, np.int64)
    v = keys != CULLED
    spl = np.asarray(table[:254], np.uint32)
    assert np.all(np.diff(spl.astype(np.int64)) >= 0) and int(table[254]) == M32, "not a table a frame could have written"
    d[v] = np.searchsorted(spl, keys[v], side="right")   # (ascending: the count of splitters <= key)
    return d


def table_is_used(table, any_visible, kmin, kmax):
    """depth_split's rule: a valid table whose frame's key range lies within a sixteenth of its own span of this frame's, at either end."""
    if table is None or not any_visible or int(table[255]) == 0:
        return False
    tmin, tmax = int(table[256]), int(table[257])
    tol = ((tmax - tmin) & M32) >> 4
    return abs(kmin - tmin) <= tol and abs(kmax - tmax) <= tol


def bucket_plan(size, bits):
    """-> (path, counting passes) of a bucket of `size` keys spanning `bits` bits."""
    if size <= FAST_CAP:
        return "resident", (bits + 8) // 9
    return "chunked", 1 if bits <= 8 else (3 if bits <= 24 else 5)


def pass_widths(bits, passes):
    return [bits // passes + (1 if p < bits % passes else 0) for p in range(passes)]


class Launches:
    """One histogram -> split -> bucket launch set over `keys`."""
    def __init__(self, keys, counts, rng, table_in, table_out, min_keys):
        keys, counts = np.asarray(keys, np.uint32), np.asarray(counts, np.uint32)
        any_visible, kmin, kmax = rng
        self.used_table = table_is_used(table_in, any_visible, kmin, kmax)
        self.scale = make_scale(any_visible, kmin, kmax)
        self.digits = table_digits(keys, table_in) if self.used_table else linear_digits(keys, kmin, self.scale)
        vis = np.flatnonzero(keys != CULLED)
        self.nv = nv = int(vis.size)
        self.totals = np.zeros(512, np.uint32)
        self.totals[:256] = np.bincount(self.digits[vis], minlength=256)
        self.order = vis[np.argsort(keys[vis], kind="stable")].astype(np.uint32)
        self.out_keys = keys[self.order]
        exact = np.cumsum(counts[self.order].astype(np.uint64))
        self.cum = (exact & np.uint64(M32)).astype(np.uint32)
        # the split's buckets are runs of the sorted order: digits are monotone in the key
        assert np.all(np.diff(self.digits[self.order]) >= 0), "the split digit is not monotone in the key"
        self.buckets = {}
        start = 0
        for b in np.flatnonzero(self.totals[:255]):
            size = int(self.totals[b])
            lo, hi = int(self.out_keys[start]), int(self.out_keys[start + size - 1])
            bits = (hi - lo).bit_length()
            path, passes = bucket_plan(size, bits)
            self.buckets[int(b)] = dict(start=start, size=size, bits=bits, path=path, passes=passes)
            self.totals[256 + b] = (int(exact[start + size - 1]) - (int(exact[start - 1]) if start else 0)) & M32
            start += size
        self.table = None
        if table_out is not None:
            t = np.array(table_out, np.uint32)
            if nv >= min_keys:
                j = np.arange(254, dtype=np.int64)
                t[:254] = self.out_keys[(j + 1) * nv // 255]
            t[254] = M32
            t[255] = 1 if nv >= min_keys else 0
            t[256], t[257] = kmin, kmax
            self.table = t


class Run:
    """What one depth_sort_scan leaves: .frame (Launches of the frame itself), .sample (Launches of the sample run or None),
    .table / .written (the table and the host's note afterwards)."""
    pass


def run(keys, counts, table=None, written=False, minmax=None):
    keys = np.asarray(keys, np.uint32)
    n = keys.size
    assert 0 < n <= (16 << 20)
    rng = key_range(minmax_of(keys) if minmax is None else minmax)
    r = Run()
    r.sample = None
    if table is not None and not written and n >= SPL_SAMPLE_MIN_N:
        m = n // SPL_SAMPLE_STRIDE
        smp = keys[::SPL_SAMPLE_STRIDE][:m]
        r.sample = Launches(smp, smp, rng, None, table, SPL_SAMPLE_MIN_KEYS)
        table = r.sample.table
    r.frame = Launches(keys, counts, rng, table, table, SPL_MIN_KEYS)
    r.table = r.frame.table
    r.written = table is not None
    nblocks = (n + DS_TILE - 1) // DS_TILE
    r.nblocks = nblocks
    r.ngroups = (nblocks + SORT_GROUP_BLOCKS - 1) // SORT_GROUP_BLOCKS
    r.scanned = r.ngroups > SORT_DIRECT_GROUPS
    return r
