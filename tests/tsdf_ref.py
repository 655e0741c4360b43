"""Float32 numpy restatement of include/brush_hip_mesh.h: TSDF integration, marching tetrahedra on the Kuhn split and the mesh PLY.
Written from the header's text (the operation order of every formula, the edge order, the case table), not from the kernels: the GPU
tests hold tsdf.hip to it bit for bit, tests/test_tsdf_ref.py holds it to the properties a mesh must have."""
import numpy as np

F = np.float32
MAX_BATCH = 8
# the seven edges a sample owns, in the header's order
D = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
D_INDEX = {d: n for n, d in enumerate(D)}
# the six tetrahedra of a cube: the permutations of the axes in lexicographic order, and which of them are negatively oriented
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
NEGATIVE = [False, True, True, False, False, True]
TET_EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
CASES = {
    1: [(0, 1, 2)], 14: [(0, 2, 1)],
    2: [(0, 4, 3)], 13: [(0, 3, 4)],
    4: [(5, 1, 3)], 11: [(5, 3, 1)],
    8: [(5, 4, 2)], 7: [(5, 2, 4)],
    3: [(1, 2, 4), (1, 4, 3)], 12: [(1, 3, 4), (1, 4, 2)],
    5: [(0, 3, 5), (0, 5, 2)], 10: [(0, 2, 5), (0, 5, 3)],
    9: [(0, 1, 5), (0, 5, 4)], 6: [(0, 4, 5), (0, 5, 1)],
}


def tet_corners(t):
    """The four vertices of tetrahedron t as offsets (x, y, z) from the cube's min corner."""
    v = [0, 0, 0]
    out = [tuple(v)]
    for axis in PERMS[t]:
        v[axis] = 1
        out.append(tuple(v))
    return out


def new_volume(dims, colour=True):
    nx, ny, nz = dims
    tw = np.zeros((nz, ny, nx, 2), F)
    tw[..., 0] = 1.0
    return tw, (np.zeros((nz, ny, nx, 3), F) if colour else None)


def sample_positions(origin, voxel_size, dims):
    """p = origin + voxel_size * (float)(i, j, k), per axis, f32: three arrays broadcastable to [nz, ny, nx]."""
    nx, ny, nz = dims
    vs = F(voxel_size)
    px = F(origin[0]) + vs * np.arange(nx, dtype=F)
    py = F(origin[1]) + vs * np.arange(ny, dtype=F)
    pz = F(origin[2]) + vs * np.arange(nz, dtype=F)
    return px[None, None, :], py[None, :, None], pz[:, None, None]


def integrate(tw, rgb, origin, voxel_size, trunc, max_weight, cams, depths, images=None, depth_min=0.0, depth_max=np.inf, alpha_min=0.5):
    """In place.  cams: dicts with vm (12 f32, column-major 3x4), fx, fy, cx, cy, w, h."""
    nz, ny, nx = tw.shape[:3]
    px, py, pz = sample_positions(origin, voxel_size, (nx, ny, nz))
    trunc, max_weight = F(trunc), F(max_weight)
    for n, cam in enumerate(cams):
        vm = np.asarray(cam["vm"], F)
        w, h = int(cam["w"]), int(cam["h"])
        depth = np.asarray(depths[n], F).reshape(h, w)
        with np.errstate(all="ignore"):
            X = ((vm[0] * px + vm[3] * py) + vm[6] * pz) + vm[9]
            Y = ((vm[1] * px + vm[4] * py) + vm[7] * pz) + vm[10]
            Z = ((vm[2] * px + vm[5] * py) + vm[8] * pz) + vm[11]
            ok = Z > F(depth_min)
            u = F(cam["fx"]) * (X / Z) + F(cam["cx"])
            v = F(cam["fy"]) * (Y / Z) + F(cam["cy"])
            ok &= (u >= F(0)) & (u < F(w)) & (v >= F(0)) & (v < F(h))
            ix = np.where(ok, np.floor(u), 0).astype(np.int64)
            iy = np.where(ok, np.floor(v), 0).astype(np.int64)
            d = depth[iy, ix]
            ok &= np.isfinite(d) & (d > F(0)) & (d <= F(depth_max))
            if images is not None:
                img = np.asarray(images[n], F).reshape(h, w, 4)
                ok &= ~(img[iy, ix, 3] < F(alpha_min))
            sdf = d - Z
            ok &= ~(sdf < -trunc)
            s = np.minimum(F(1), sdf / trunc)
            T, W = tw[..., 0], tw[..., 1]
            Wn = W + F(1)
            Tn = (W * T + s) / Wn
            if images is not None and rgb is not None:
                cn = (W[..., None] * rgb + img[iy, ix, :3]) / Wn[..., None]
                rgb[ok] = cn[ok]
            tw[..., 0] = np.where(ok, Tn, T)
            tw[..., 1] = np.where(ok, np.minimum(Wn, max_weight), W)
    return tw, rgb


def classify(tw):
    """(active [nz,ny,nx,7] bool: the owned edges that carry a vertex, valid [nz,ny,nx] bool: the valid cubes by min corner)."""
    nz, ny, nx = tw.shape[:3]
    inside = tw[..., 0] < 0
    obs = tw[..., 1] > 0
    valid = np.zeros((nz, ny, nx), bool)
    v = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for bz in (0, 1):
        for by in (0, 1):
            for bx in (0, 1):
                v &= obs[bz:nz - 1 + bz, by:ny - 1 + by, bx:nx - 1 + bx]
    valid[:nz - 1, :ny - 1, :nx - 1] = v
    active = np.zeros((nz, ny, nx, 7), bool)
    for n, (dx, dy, dz) in enumerate(D):
        has = np.zeros((nz, ny, nx), bool)   # some valid cube with min corner p - a contains p and p + d
        for az in ((0,) if dz else (0, 1)):
            for ay in ((0,) if dy else (0, 1)):
                for ax in ((0,) if dx else (0, 1)):
                    has[az:, ay:, ax:] |= valid[:nz - az, :ny - ay, :nx - ax]
        differ = np.zeros((nz, ny, nx), bool)
        differ[:nz - dz, :ny - dy, :nx - dx] = inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]
        active[..., n] = has & differ
    return active, valid


def extract(tw, rgb, origin, voxel_size):
    """(vertices [V,3] f32, colours [V,3] f32 or None, triangles [M,3] u32) in the header's order."""
    nz, ny, nx = tw.shape[:3]
    active, valid = classify(tw)
    flat = active.reshape(-1, 7)
    index = np.cumsum(flat.reshape(-1)).reshape(-1, 7) - 1   # vertex number of (owner, d) where active
    owner, dn = np.nonzero(flat)
    k, j, i = owner // (nx * ny), (owner // nx) % ny, owner % nx
    dv = np.asarray(D, np.int64)[dn]
    T = tw[..., 0]
    Ta, Tb = T[k, j, i], T[k + dv[:, 2], j + dv[:, 1], i + dv[:, 0]]
    with np.errstate(all="ignore"):
        t = Ta / (Ta - Tb)
    vs = F(voxel_size)
    verts = np.empty((len(owner), 3), F)
    for axis, idx in enumerate((i, j, k)):
        pa = F(origin[axis]) + vs * idx.astype(F)
        pb = F(origin[axis]) + vs * (idx + dv[:, axis]).astype(F)
        verts[:, axis] = pa + t * (pb - pa)
    cols = None
    if rgb is not None:
        ca, cb = rgb[k, j, i], rgb[k + dv[:, 2], j + dv[:, 1], i + dv[:, 0]]
        cols = (ca + t[:, None] * (cb - ca)).astype(F)
    inside = T < 0
    tris = []
    corners = [tet_corners(t_) for t_ in range(6)]
    for s in np.flatnonzero(valid.reshape(-1)):
        ck, cj, ci = s // (nx * ny), (s // nx) % ny, s % nx
        cube = inside[ck:ck + 2, cj:cj + 2, ci:ci + 2]
        if cube.all() or not cube.any():
            continue
        for t_ in range(6):
            vs4 = corners[t_]
            m = sum(1 << n for n, (x, y, z) in enumerate(vs4) if cube[z, y, x])
            for tri in CASES.get(m, ()):
                if NEGATIVE[t_]:
                    tri = (tri[0], tri[2], tri[1])
                row = []
                for e in tri:
                    a, b = vs4[TET_EDGES[e][0]], vs4[TET_EDGES[e][1]]
                    d = D_INDEX[(b[0] - a[0], b[1] - a[1], b[2] - a[2])]
                    o = ((ck + a[2]) * ny + (cj + a[1])) * nx + (ci + a[0])
                    assert flat[o, d]
                    row.append(index[o, d])
                tris.append(row)
    return verts, cols, np.asarray(tris, np.uint32).reshape(-1, 3)


def mesh_to_ply(verts, cols, tris):
    verts = np.asarray(verts, F).reshape(-1, 3)
    tris = np.asarray(tris, np.uint32).reshape(-1, 3)
    head = "ply\nformat binary_little_endian 1.0\ncomment Exported from Brush\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(verts)
    if cols is not None:
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    head += "element face %d\nproperty list uchar uint vertex_indices\nend_header\n" % len(tris)
    if cols is not None:
        c = np.asarray(cols, F).reshape(-1, 3)
        c = np.where(np.isnan(c), F(0), c)
        q = np.rint(np.minimum(np.maximum(c, F(0)), F(1)) * F(255)).astype(np.uint8)   # rint: half to even
        rows = np.zeros(len(verts), np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
        rows["p"], rows["c"] = verts, q
        body = rows.tobytes()
    else:
        body = verts.astype("<f4").tobytes()
    faces = np.zeros(len(tris), np.dtype([("n", "u1"), ("i", "<u4", 3)]))
    faces["n"], faces["i"] = 3, tris
    return head.encode("ascii") + body + faces.tobytes()


# ---- properties of a mesh (shared by the CPU and the GPU tests) ----------------------------------------------------------------------
def canonical(tris):
    """Each triangle rotated to start at its smallest index, rows sorted."""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    r = np.argmin(t, axis=1)
    t = np.stack([t[np.arange(len(t)), (r + n) % 3] for n in range(3)], axis=1)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


def directed_edges(tris):
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def boundary_edges(tris):
    """Directed edges whose reverse does not occur exactly as often (empty for a closed, consistently oriented mesh)."""
    e = directed_edges(tris)
    big = int(e.max()) + 1 if len(e) else 1
    fwd, nf = np.unique(e[:, 0] * big + e[:, 1], return_counts=True)
    rev, nr = np.unique(e[:, 1] * big + e[:, 0], return_counts=True)
    if len(fwd) == len(rev) and np.array_equal(fwd, rev) and np.array_equal(nf, nr):
        return np.zeros((0, 2), np.int64)
    a, b = dict(zip(fwd.tolist(), nf.tolist())), dict(zip(rev.tolist(), nr.tolist()))
    bad = [key for key in a if a[key] != b.get(key, 0)]
    return np.asarray([(key // big, key % big) for key in bad], np.int64)


def signed_volume(verts, tris):
    v = np.asarray(verts, np.float64)
    t = np.asarray(tris, np.int64)
    return float(np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)


def triangle_areas(verts, tris):
    v = np.asarray(verts, np.float64)
    t = np.asarray(tris, np.int64)
    return 0.5 * np.linalg.norm(np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]), axis=1)
