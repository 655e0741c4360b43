"""Float32 numpy restatement of include/brush_hip_sparse_mesh.h: the marking rule, the dilation, rank / keys / pool slots, the block
layout and the scatter to a dense volume.  Written from the header's text, not from the kernels.  The per-sample fusion rule and the
extraction are tests/tsdf_ref.py's, imported unchanged: a sparse volume is held to them through the dense volume it scatters to."""
import numpy as np

import tsdf_ref as tr

F = np.float32
BLOCK = 8
MAX_STEPS = 64


def block_dims(dims):
    return tuple((int(d) + BLOCK - 1) // BLOCK for d in dims)


def n_words(dims):
    nbx, nby, nbz = block_dims(dims)
    return (nbx * nby * nbz + 31) // 32


def mark_steps(voxel_size, trunc):
    """The smallest integer M with (float)M * (4.0f * voxel_size) >= 2.0f * trunc, in f32 (MAX_STEPS + 1: refused)."""
    step, band = F(4) * F(voxel_size), F(2) * F(trunc)
    m = 0
    while m <= MAX_STEPS and not F(m) * step >= band:
        m += 1
    return m


def mark(marked, origin, voxel_size, dims, trunc, cams, depths, images=None, depth_max=np.inf, alpha_min=0.5):
    """In place: marked [NBZ,NBY,NBX] bool.  cams: dicts with vm (12 f32, column-major 3x4), cam_pos, fx, fy, cx, cy, w, h."""
    M = mark_steps(voxel_size, trunc)
    assert M <= MAX_STEPS
    vs, trunc = F(voxel_size), F(trunc)
    step = F(4) * vs
    for n, cam in enumerate(cams):
        vm, pos = np.asarray(cam["vm"], F), np.asarray(cam["cam_pos"], F)
        w, h = int(cam["w"]), int(cam["h"])
        d = np.asarray(depths[n], F).reshape(h, w)
        with np.errstate(all="ignore"):
            ok = np.isfinite(d) & (d > F(0)) & (d <= F(depth_max))
            if images is not None:
                ok &= ~(np.asarray(images[n], F).reshape(h, w, 4)[..., 3] < F(alpha_min))
            rx = ((np.arange(w, dtype=F)[None, :] + F(0.5)) - F(cam["cx"])) / F(cam["fx"])
            ry = ((np.arange(h, dtype=F)[:, None] + F(0.5)) - F(cam["cy"])) / F(cam["fy"])
            for m in range(M + 1):
                z = (d - trunc) + F(m) * step
                hit = ok & (z > F(0))
                X, Y = rx * z, ry * z
                blk = []
                for a in range(3):
                    pw = ((vm[3 * a] * X + vm[3 * a + 1] * Y) + vm[3 * a + 2] * z) + pos[a]
                    g = (pw - F(origin[a])) / vs
                    hit = hit & (g >= F(0)) & (g < F(dims[a]))
                    blk.append(g * F(0.125))
                bx, by, bz = (b[hit].astype(np.uint32) for b in blk)
                marked[bz, by, bx] = True
    return marked


def dilate(marked, r):
    """A block is set iff a set block lies within Chebyshev distance r of it inside the grid: three one-axis passes of a box."""
    out = marked.copy()
    for axis in range(3):
        src = out.copy()
        n = src.shape[axis]
        for d in range(1, r + 1):
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, n - d), slice(d, n)
            out[tuple(lo)] |= src[tuple(hi)]
            out[tuple(hi)] |= src[tuple(lo)]
    return out


def index_of(marked):
    """(bits [n_words] u32, rank [n_words] u32, keys [n_blocks] u32) of a block set [NBZ,NBY,NBX]: key = (bz NBY + by) NBX + bx."""
    flat = marked.reshape(-1)
    keys = np.flatnonzero(flat).astype(np.uint32)
    words = (len(flat) + 31) // 32
    padded = np.zeros(words * 32, np.uint64)
    padded[:len(flat)] = flat
    bits = (padded.reshape(words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    counts = padded.reshape(words, 32).sum(axis=1).astype(np.uint64)
    rank = (np.cumsum(counts) - counts).astype(np.uint32)
    return bits, rank, keys


def slot_of(bits, rank, key):
    """rank[key / 32] + popcount(bits[key / 32] & ((1 << key % 32) - 1)), or None where the block's bit is clear."""
    word, b = int(bits[key >> 5]), key & 31
    if not (word >> b) & 1:
        return None
    return int(rank[key >> 5]) + bin(word & ((1 << b) - 1)).count("1")


def block_coords(keys, dims):
    nbx, nby, _ = block_dims(dims)
    keys = np.asarray(keys, np.int64)
    return keys % nbx, (keys // nbx) % nby, keys // (nbx * nby)


def pool_indices(keys, dims):
    """For every sample of the virtual grid the index of its pool entry, slot * 512 + (lz 8 + ly) 8 + lx, or -1: [nz,ny,nx] int64."""
    nx, ny, nz = dims
    nbx, nby, nbz = block_dims(dims)
    slot = np.full(nbx * nby * nbz, -1, np.int64)
    slot[np.asarray(keys, np.int64)] = np.arange(len(keys))
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    s = slot[((k // BLOCK) * nby + j // BLOCK) * nbx + i // BLOCK]
    return np.where(s >= 0, s * 512 + ((k % BLOCK) * BLOCK + j % BLOCK) * BLOCK + i % BLOCK, -1)


def to_dense(pool_tw, pool_rgb, keys, dims):
    """The whole virtual grid as a dense volume: allocated samples copied, everything else T = 1, W = 0, rgb = 0."""
    idx = pool_indices(keys, dims)
    tw, rgb = tr.new_volume(dims, pool_rgb is not None)
    have = idx >= 0
    tw[have] = np.asarray(pool_tw, F).reshape(-1, 2)[idx[have]]
    if pool_rgb is not None:
        rgb[have] = np.asarray(pool_rgb, F).reshape(-1, 3)[idx[have]]
    return tw, rgb


def to_pool(tw, rgb, keys, dims):
    """The inverse: the pool [n_blocks,8,8,8,2] (and rgb) that holds a dense volume's samples in the blocks `keys`; samples of a boundary
    block that do not exist are T = 1, W = 0, rgb = 0."""
    n = len(keys)
    ptw = np.zeros((n, BLOCK, BLOCK, BLOCK, 2), F)
    ptw[..., 0] = 1.0
    prgb = np.zeros((n, BLOCK, BLOCK, BLOCK, 3), F) if rgb is not None else None
    idx = pool_indices(keys, dims)
    have = idx >= 0
    ptw.reshape(-1, 2)[idx[have]] = tw[have]
    if rgb is not None:
        prgb.reshape(-1, 3)[idx[have]] = rgb[have]
    return ptw, prgb


def vertex_owners(tw):
    """(owner linear index, d) of every vertex of tr.extract(tw, ...), in its order."""
    active, _ = tr.classify(tw)
    return np.nonzero(active.reshape(-1, 7))


def sparse_order(tw, keys, dims):
    """The order in which the sparse extraction emits the vertices of the dense volume tw (= to_dense of the sparse one): by pool slot,
    then local index, then d.  -> perm with sparse_vertices = dense_vertices[perm]; every owner must lie in an allocated block."""
    owner, d = vertex_owners(tw)
    pool = pool_indices(keys, dims).reshape(-1)[owner]
    assert (pool >= 0).all(), "a vertex whose owner is not allocated"
    return np.lexsort((d, pool))


def reorder_mesh(verts, cols, tris, perm):
    """The dense mesh with its vertices in the order perm: (verts, cols, tris with the indices renamed)."""
    new_index = np.empty(len(perm), np.int64)
    new_index[perm] = np.arange(len(perm))
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    return verts[perm], (cols[perm] if cols is not None else None), new_index[tris].astype(np.uint32)


def band_blocks(origin, voxel_size, dims, trunc, cams, depths, images=None, **kw):
    """[NBZ,NBY,NBX] bool: the blocks that hold a sample some view gave sdf < trunc (a touched sample whose single-view T is below 1)."""
    nbx, nby, nbz = block_dims(dims)
    nx, ny, nz = dims
    out = np.zeros((nbz, nby, nbx), bool)
    for n, cam in enumerate(cams):
        tw, _ = tr.new_volume(dims, False)
        tr.integrate(tw, None, origin, voxel_size, trunc, 64.0, [cam], [depths[n]], None if images is None else [images[n]], **kw)
        k, j, i = np.nonzero((tw[..., 1] > 0) & (tw[..., 0] < 1))
        out[k // BLOCK, j // BLOCK, i // BLOCK] = True
    return out
