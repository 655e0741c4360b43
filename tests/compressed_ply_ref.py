"""numpy restatement of the compressed.ply writer (include/brush_hip_compressed_ply.h) that
tests/test_compressed_ply_abi.py and tests/test_gpu_compressed_ply.py hold bh_splat_to_compressed_ply to, byte for byte.

Every operation is an f32 operation in the order the contract writes it (numpy rounds each one; no contraction).  The opacity byte
takes alpha = 1 / (1 + e) with e = bo_expf(-raw) of the oracle library, the restatement of the device's bh_expf."""
import numpy as np

from oracle import ply as oply

F = np.float32
CHUNK = 256
SH_C0 = F(0.2820948)


def expf(x):
    """bo_expf (oracle/brush_oracle.cpp, = the device's bh_expf) of every element, one call per distinct value."""
    from oracle import bo
    x = np.ascontiguousarray(x, F)
    u, inv = np.unique(x.view(np.uint32), return_inverse=True)
    f = bo.lib().bo_expf
    vals = np.array([f(float(v)) for v in u.view(F)], F)
    return vals[inv].reshape(x.shape)


def unorm(v, bits):
    """min(t, floor(v t + 0.5)), t = 2^bits - 1; 0 for v < 0 or NaN -> uint32"""
    v = np.asarray(v, F)
    t = F((1 << bits) - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((v * t).astype(F) + F(0.5)).astype(F)
        ok = v >= F(0)
        f = np.where(ok, np.minimum(f, t), F(0))
    return f.astype(np.uint32)


def norm01(x, lo, hi):
    """0 for hi - lo < 1e-5, else (x - lo) / (hi - lo)"""
    x, lo, hi = np.asarray(x, F), np.asarray(lo, F), np.asarray(hi, F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r = (hi - lo).astype(F)
        return np.where(r < F(1e-5), F(0), ((x - lo).astype(F) / r).astype(F)).astype(F)


def part1by2(x):
    x = np.asarray(x, np.uint32) & np.uint32(0x3FF)
    x = (x | (x << np.uint32(16))) & np.uint32(0x030000FF)
    x = (x | (x << np.uint32(8))) & np.uint32(0x0300F00F)
    x = (x | (x << np.uint32(4))) & np.uint32(0x030C30C3)
    x = (x | (x << np.uint32(2))) & np.uint32(0x09249249)
    return x


def _finite_range(v, axis):
    """(min, max) of the finite values of v + 0 along axis; (0, 0) where there is none"""
    v = np.asarray(v, F)
    fin = np.isfinite(v)
    with np.errstate(invalid="ignore"):
        z = (v + F(0)).astype(F)
    lo = np.where(fin, z, F(np.inf)).min(axis=axis)
    hi = np.where(fin, z, F(-np.inf)).max(axis=axis)
    empty = lo == F(np.inf)
    return np.where(empty, F(0), lo).astype(F), np.where(empty, F(0), hi).astype(F)


def box(pos):
    lo, hi = _finite_range(np.asarray(pos, F).reshape(-1, 3), axis=0)
    return lo, hi


def morton_keys(pos):
    """30-bit key per row: part1by2(q_z) << 2 | part1by2(q_y) << 1 | part1by2(q_x) over the finite position box"""
    pos = np.asarray(pos, F).reshape(-1, 3)
    if pos.shape[0] == 0:
        return np.zeros(0, np.uint32)
    lo, hi = box(pos)
    q = []
    for a in range(3):
        with np.errstate(invalid="ignore"):
            f = np.floor((F(1024) * norm01(pos[:, a], lo[a], hi[a])).astype(F))
            q.append(np.where(~(f >= F(0)), 0, np.where(f > F(1023), 1023, np.nan_to_num(f))).astype(np.uint32))
    return (part1by2(q[2]) << np.uint32(2)) | (part1by2(q[1]) << np.uint32(1)) | part1by2(q[0])


def rotation_words(q):
    """smallest-three word of each (w, x, y, z) row: L << 30 | the other three, 10 bits each, ascending index"""
    q = np.asarray(q, F).reshape(-1, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        s = ((((q[:, 0] * q[:, 0]).astype(F) + (q[:, 1] * q[:, 1]).astype(F)).astype(F) + (q[:, 2] * q[:, 2]).astype(F)).astype(F)
             + (q[:, 3] * q[:, 3]).astype(F)).astype(F)
        bad = (s == F(0)) | ~np.isfinite(s)
        r = np.sqrt(np.where(bad, F(1), s)).astype(F)
        a = (q / r[:, None]).astype(F)
    a[bad] = np.array([1, 0, 0, 0], F)
    L = np.argmax(np.abs(a), axis=1)   # the first of equal maxima: strict `>`
    neg = a[np.arange(a.shape[0]), L] < F(0)
    a = np.where(neg[:, None], -a, a).astype(F)
    others = np.array([[k for k in range(4) if k != l] for l in range(4)])[L]
    word = L.astype(np.uint32)
    for j in range(3):
        v = a[np.arange(a.shape[0]), others[:, j]]
        word = (word << np.uint32(10)) | unorm(((v * F(0.70710677)).astype(F) + F(0.5)).astype(F), 10)
    return word


def sh_bytes(v):
    """clamp(trunc((v * 0.125 + 0.5) * 256), 0, 255), NaN -> 0"""
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore", over="ignore"):
        f = ((((v * F(0.125)).astype(F) + F(0.5)).astype(F)) * F(256)).astype(F)
        return np.where(~(f > F(0)), 0, np.where(f >= F(255), 255, np.trunc(np.nan_to_num(f)))).astype(np.uint8)


def header(n, sh_degree, render_mip=False, up_axis=None):
    lines = ["ply", "format binary_little_endian 1.0", "comment Exported from Brush"]
    if up_axis is not None:
        lines.append("comment Vertical axis: %s %s %s" % tuple(oply._f32_display(x) for x in up_axis))
    else:
        lines.append("comment Vertical axis: y")
    lines.append("comment SH degree: %d" % sh_degree)
    lines.append("comment SplatRenderMode: %s" % ("mip" if render_mip else "default"))
    lines.append("element chunk %d" % ((n + CHUNK - 1) // CHUNK))
    lines += ["property float " + p for p in oply.CHUNK_PROPS]
    lines.append("element vertex %d" % n)
    lines += ["property uint " + p for p in oply.VERTEX_PROPS]
    k = 3 * ((sh_degree + 1) ** 2 - 1)
    if k:
        lines.append("element sh %d" % n)
        lines += ["property uchar f_rest_%d" % i for i in range(k)]
    lines.append("end_header")
    return ("\n".join(lines) + "\n").encode("ascii")


def body_size(n, sh_degree):
    return 72 * ((n + CHUNK - 1) // CHUNK) + 16 * n + 3 * ((sh_degree + 1) ** 2 - 1) * n


def compressed_ply(transforms, sh, raw_opac, render_mip=False, up_axis=None, min_scale=None, return_order=False):
    """-> the file's bytes (and the file row -> input row order)."""
    t = np.ascontiguousarray(transforms, F).reshape(-1, 10)
    n = t.shape[0]
    o = np.ascontiguousarray(raw_opac, F).reshape(n)
    s = np.ascontiguousarray(sh, F)
    coeffs = s.shape[1] if s.ndim == 3 else (s.size // (3 * n) if n else 1)   # sh [n, C, 3] (or flat when n > 0)
    s = s.reshape(n, coeffs, 3)
    deg = int(round(coeffs ** 0.5)) - 1
    assert (deg + 1) ** 2 == coeffs and deg <= 4
    if min_scale is not None and n:
        from oracle import bo
        t, o = bo.fold_min_scale(t, o, min_scale)
    head = header(n, deg, render_mip, up_axis)
    if n == 0:
        return (head, np.zeros(0, np.uint32)) if return_order else head
    keys = morton_keys(t[:, 0:3])
    order = np.argsort(keys, kind="stable").astype(np.uint32)
    T, O, S = t[order], o[order], s[order]
    nch = (n + CHUNK - 1) // CHUNK
    pad = nch * CHUNK - n
    with np.errstate(invalid="ignore", over="ignore"):
        rgb = ((S[:, 0, :] * SH_C0).astype(F) + F(0.5)).astype(F)
    cols = np.concatenate([T[:, 0:3], T[:, 7:10], rgb], axis=1)          # [n, 9]: position, log-scale, colour
    padded = np.concatenate([cols, np.full((pad, 9), np.nan, F)], axis=0).reshape(nch, CHUNK, 9)
    lo, hi = _finite_range(padded, axis=1)                                # [nch, 9]
    chunk_rows = np.concatenate([lo[:, 0:3], hi[:, 0:3], lo[:, 3:6], hi[:, 3:6], lo[:, 6:9], hi[:, 6:9]], axis=1).astype(F)
    ch = np.arange(n) // CHUNK
    nq = [norm01(cols[:, k], lo[ch, k], hi[ch, k]) for k in range(9)]
    ppos = (unorm(nq[0], 11) << np.uint32(21)) | (unorm(nq[1], 10) << np.uint32(11)) | unorm(nq[2], 11)
    pscl = (unorm(nq[3], 11) << np.uint32(21)) | (unorm(nq[4], 10) << np.uint32(11)) | unorm(nq[5], 11)
    with np.errstate(invalid="ignore", over="ignore"):
        alpha = (F(1) / (F(1) + expf(-O)).astype(F)).astype(F)
    pcol = (unorm(nq[6], 8) << np.uint32(24)) | (unorm(nq[7], 8) << np.uint32(16)) | (unorm(nq[8], 8) << np.uint32(8)) | unorm(alpha, 8)
    prot = rotation_words(T[:, 3:7])
    vert = np.stack([ppos, prot, pscl, pcol], axis=1).astype("<u4")
    body = chunk_rows.astype("<f4").tobytes() + vert.tobytes()
    if deg > 0:
        rest = S[:, 1:, :].transpose(0, 2, 1).reshape(n, -1)              # [channel][coeff 1..]: f_rest_{c K + k - 1}
        body += sh_bytes(rest).tobytes()
    assert len(body) == body_size(n, deg)
    data = head + body
    return (data, order) if return_order else data


def alpha(raw_opac):
    """the opacity the writer quantises: 1 / (1 + bo_expf(-raw)), f32"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (F(1) / (F(1) + expf(-np.asarray(raw_opac, F))).astype(F)).astype(F)


def chunk_rows(data):
    """the file's chunk element as [C, 18] f32 (CHUNK_PROPS order)"""
    body = data.index(b"end_header\n") + len(b"end_header\n")
    n = int(data[data.index(b"element vertex ") + 15:].split(b"\n", 1)[0])
    nch = (n + CHUNK - 1) // CHUNK
    return np.frombuffer(data, "<f4", count=nch * 18, offset=body).reshape(nch, 18)


def round_trip_violations(data, order, transforms, sh, raw_opac):
    """Decoded rows (oracle/ply.load_compressed_ply of `data`) against the input rows order[r] they came from, within the bounds
    of the quantisation steps.  -> {name: number of finite values outside their bound}; all zero when the file is right."""
    dec = oply.load_compressed_ply(data)
    n = len(order)
    t = np.asarray(transforms, F).reshape(-1, 10)[order]
    s = np.asarray(sh, F).reshape(n, -1, 3)[order]
    o = np.asarray(raw_opac, F).reshape(-1)[order]
    cr = chunk_rows(data).astype(np.float64)
    ch = np.arange(n) // CHUNK
    bad = {}
    for name, cols, lo_c, bits in (("position", (0, 1, 2), 0, (11, 10, 11)), ("log_scale", (7, 8, 9), 6, (11, 10, 11))):
        for a in range(3):
            lo, hi = cr[ch, lo_c + a], cr[ch, lo_c + 3 + a]
            x = t[:, cols[a]].astype(np.float64)
            fin = np.isfinite(x)
            ulp = np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(F)).astype(np.float64)
            bound = np.where(hi - lo < 1e-5, 1e-5, (hi - lo) / (2 * ((1 << bits[a]) - 1)) + 4 * ulp)
            err = np.abs(dec["transforms"][:, cols[a]].astype(np.float64) - x)
            bad["%s_%d" % (name, a)] = int(np.count_nonzero(fin & ~(err <= bound)))
    with np.errstate(over="ignore", invalid="ignore"):
        a_dec = 1.0 / (1.0 + np.exp(-dec["raw_opac"].astype(np.float64)))
    a_ref = alpha(o).astype(np.float64)
    fin = np.isfinite(a_ref)
    bad["alpha"] = int(np.count_nonzero(fin & ~(np.abs(a_dec - a_ref) <= 1.0 / 510 + 1e-7)))
    q = t[:, 3:7].astype(np.float64)
    nrm = np.sqrt((q * q).sum(axis=1))
    with np.errstate(over="ignore", invalid="ignore"):
        okq = np.isfinite(nrm) & (nrm > 0) & np.isfinite(((((t[:, 3] * t[:, 3]).astype(F) + (t[:, 4] * t[:, 4]).astype(F)).astype(F)
                                                           + (t[:, 5] * t[:, 5]).astype(F)).astype(F) + (t[:, 6] * t[:, 6]).astype(F)))
    qn = q / np.where(okq, nrm, 1.0)[:, None]
    qd = dec["transforms"][:, 3:7].astype(np.float64)
    qn = np.where(((qn * qd).sum(axis=1) < 0)[:, None], -qn, qn)
    words = np.frombuffer(data, "<u4", count=4 * n, offset=data.index(b"end_header\n") + 11 + 72 * ((n + CHUNK - 1) // CHUNK)).reshape(n, 4)
    L = (words[:, 1] >> 30).astype(np.int64)
    err = np.abs(qd - qn)
    big = np.zeros((n, 4), bool)
    big[np.arange(n), L] = True
    bad["rotation_stored"] = int(np.count_nonzero(okq[:, None] & ~big & ~(err <= 7e-4)))
    bad["rotation_rebuilt"] = int(np.count_nonzero(okq[:, None] & big & ~(err <= 3e-3)))
    if s.shape[1] > 1:
        v = s[:, 1:, :].astype(np.float64)
        inside = (v >= -4.0) & (v < 3.96875)
        err = np.abs(dec["sh"][:, 1:, :].astype(np.float64) - v)
        bad["sh"] = int(np.count_nonzero(inside & ~(err <= 0.0315 + 0.0079 * np.abs(v))))
    return bad


def random_scene(n, sh_degree, seed):
    """seeded splats: positions in a box, unnormalised quaternions, SH rest in [-4, 3.96875)"""
    rng = np.random.default_rng(seed)
    c = (sh_degree + 1) ** 2
    t = np.empty((n, 10), F)
    t[:, 0:3] = rng.uniform(-5, 5, (n, 3))
    t[:, 3:7] = rng.normal(0, 1, (n, 4))
    t[:, 7:10] = rng.uniform(-7, -1, (n, 3))
    sh = rng.uniform(-4, 3.96875, (n, c, 3)).astype(F)
    sh[:, 0, :] = rng.uniform(-2, 2, (n, 3))
    o = rng.uniform(-6, 6, n).astype(F)
    return t, sh, o


def edge_scene(sh_degree, seed=0):
    """1100 rows with every edge the contract names: NaN / +-inf in positions, scales, colours and opacity; zero and non-finite
    quaternions; a negative largest component; ties in |a_k|; a chunk (file rows 512..767 after sorting: all rows at one point, so
    one Morton cell) whose positions, scales and colours share one value; -0 next to +0; SH outside +-4.  Input rows 0..255 sit at
    the corner of the box, the only rows in cell 0: the stable sort keeps them as file rows 0..255, the first chunk."""
    t, sh, o = random_scene(1100, sh_degree, seed)
    nan, inf = F(np.nan), F(np.inf)
    rng = np.random.default_rng(seed + 1)
    t[0:256, 0:3] = F(-6.0)
    t[0:256, 7:10] = F(-3.0)
    sh[0:256, 0, :] = F(0.25)
    k = iter(256 + rng.permutation(844))
    for col in (0, 1, 2, 7, 8, 9):
        for v in (nan, inf, -inf):
            t[next(k), col] = v
    for v in (nan, inf, -inf):
        o[next(k)] = v
        sh[next(k), 0, rng.integers(0, 3)] = v
    o[next(k)] = F(200.0)
    o[next(k)] = F(-200.0)
    o[next(k)] = F(0.0)
    t[next(k), 3:7] = 0
    t[next(k), 3:7] = (nan, 1, 0, 0)
    t[next(k), 3:7] = (inf, 0, 0, 0)
    t[next(k), 3:7] = (1e30, 1e30, 0, 0)       # s overflows: the identity
    t[next(k), 3:7] = (1e-30, 0, 0, 0)         # s underflows to 0: the identity
    t[next(k), 3:7] = (0.1, -0.9, 0.2, 0.3)    # negative largest component
    t[next(k), 3:7] = (0.5, -0.5, 0.5, -0.5)   # four-way tie
    t[next(k), 3:7] = (0, -0.6, 0.6, 0)        # two-way tie, first negative
    t[next(k), 3:7] = (-1, 0, 0, 0)
    for _ in range(6):                          # -0 and +0 side by side
        r = next(k)
        t[r, 0:3] = (-0.0, 0.0, -0.0) if r % 2 else (0.0, -0.0, 0.0)
        t[r, 7] = F(-0.0)
        sh[r, 0, :] = F(-0.5 / 0.2820948) if r % 3 else F(0)
    if sh_degree > 0:
        for v in (nan, inf, -inf, F(-4.0), F(-4.01), F(3.96875), F(4.5), F(-100), F(100), F(-0.0)):
            sh[next(k), 1 + rng.integers(0, sh.shape[1] - 1), rng.integers(0, 3)] = v
    return t, sh, o
