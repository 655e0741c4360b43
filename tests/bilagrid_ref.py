"""Float64 restatement of per-view bilateral grids (include/brush_hip_bilagrid.h) in numpy: the trilinear slice of a
grid g[Hg,Wg,L,12] of row-major 3x4 colour matrices on an [H,W,4] image, its backward with the L1 masses the GPU tests scale their
bounds by, the total variation with its gradient, and the Adam step.  `coord_dtype` selects the arithmetic of the coordinates alone:
numpy.float32 restates the header's f32 coordinates bit for bit (the reference of the GPU tests), numpy.float64 is the smooth
operator tests/test_bilagrid_ref.py pins to torch's grid_sample.  Everything behind the coordinates is float64."""
import numpy as np

IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)
LUM = (0.299, 0.587, 0.114)


def identity_grid(grid_h, grid_w, grid_l):
    return np.tile(IDENTITY, (grid_h, grid_w, grid_l, 1))


def to_gsplat(g):
    """g[j][i][l][k] -> gsplat's grids[k, l, j, i]."""
    return np.ascontiguousarray(np.asarray(g).transpose(3, 2, 0, 1))


def from_gsplat(grids):
    return np.ascontiguousarray(np.asarray(grids).transpose(2, 3, 1, 0))


def _axis(f, n, dt):
    """cell, upper neighbour and fraction of the coordinates f on an axis of n vertices."""
    i0 = np.minimum(np.floor(f), dt(max(n - 2, 0))).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    t = (f - i0.astype(dt)).astype(dt)
    return i0, i1, t.astype(np.float64)


def coordinates(shape, x, coord_dtype=np.float32):
    """The header's coordinates of every pixel of x [H,W,4] on a grid of `shape` = (Hg, Wg, L[, 12]), each operation rounded to
    coord_dtype on its own: dict(i0, i1, tx [W]; j0, j1, ty [H]; l0, l1, tz, inside [H,W])."""
    dt = coord_dtype
    gh, gw, gl = (int(v) for v in shape[:3])
    h, w = x.shape[:2]
    sx, sy = dt(dt(gw - 1) / dt(w)), dt(dt(gh - 1) / dt(h))
    fx = ((np.arange(w).astype(dt) + dt(0.5)) * sx).astype(dt)
    fy = ((np.arange(h).astype(dt) + dt(0.5)) * sy).astype(dt)
    c = np.asarray(x)[..., :3].astype(dt)
    lum = ((c[..., 0] * dt(0.299) + c[..., 1] * dt(0.587)).astype(dt) + c[..., 2] * dt(0.114)).astype(dt)
    fz = (np.minimum(np.maximum(lum, dt(0)), dt(1)) * dt(gl - 1)).astype(dt)
    i0, i1, tx = _axis(fx, gw, dt)
    j0, j1, ty = _axis(fy, gh, dt)
    l0, l1, tz = _axis(fz, gl, dt)
    return dict(i0=i0, i1=i1, tx=tx, j0=j0, j1=j1, ty=ty, l0=l0, l1=l1, tz=tz, inside=(lum > 0) & (lum < 1))


def _corners(co):
    """The 8 corners in (cy, cx, cz) order: (j [H,1], i [1,W], l [H,W], w_y w_x [H,W], w_z [H,W], d w_z / d tz)."""
    out = []
    for j, wy in ((co["j0"], 1.0 - co["ty"]), (co["j1"], co["ty"])):
        for i, wx in ((co["i0"], 1.0 - co["tx"]), (co["i1"], co["tx"])):
            wyx = wy[:, None] * wx[None, :]
            for l, wz, dz in ((co["l0"], 1.0 - co["tz"], -1.0), (co["l1"], co["tz"], 1.0)):
                out.append((j[:, None], i[None, :], l, wyx, wz, dz))
    return out


def slice_grid(g, x, coord_dtype=np.float32):
    """dict(y [H,W,4] f64, mass_y [H,W,3] = sum over corners |w| (sum_k |g[4r+k]| |x_k| + |g[4r+3]|), A [H,W,12])."""
    g, xd = np.asarray(g, np.float64), np.asarray(x, np.float64)
    co = coordinates(g.shape, x, coord_dtype)
    h, w = xd.shape[:2]
    a, mass = np.zeros((h, w, 12)), np.zeros((h, w, 3))
    x1 = np.concatenate([xd[..., :3], np.ones((h, w, 1))], -1)
    for j, i, l, wyx, wz, _ in _corners(co):
        gc = g[j, i, l]
        wgt = (wyx * wz)[..., None]
        a += wgt * gc
        mass += np.abs(wgt) * (np.abs(gc).reshape(h, w, 3, 4) * np.abs(x1)[:, :, None, :]).sum(-1)
    y = xd.copy()
    y[..., :3] = (a.reshape(h, w, 3, 4) * x1[:, :, None, :]).sum(-1)
    return dict(y=y, mass_y=mass, A=a)


def backward(g, x, v, coord_dtype=np.float32):
    """For a cotangent v [H,W,4] on y: dict(v_img [H,W,4], mass_v [H,W,3], v_g [Hg,Wg,L,12], S [Hg,Wg,L,12] = sum_p |w o_q|,
    reached [Hg,Wg,L] bool: some pixel has the vertex among its corners)."""
    g, xd, vd = np.asarray(g, np.float64), np.asarray(x, np.float64), np.asarray(v, np.float64)
    gh, gw, gl = g.shape[:3]
    co = coordinates(g.shape, x, coord_dtype)
    h, w = xd.shape[:2]
    x1 = np.concatenate([xd[..., :3], np.ones((h, w, 1))], -1)
    o = (vd[..., :3, None] * x1[:, :, None, :]).reshape(h, w, 12)
    a, da = np.zeros((h, w, 12)), np.zeros((h, w, 12))
    mass_a, mass_d = np.zeros((h, w, 3)), np.zeros((h, w))
    v_g, s, reached = np.zeros(gh * gw * gl * 12), np.zeros(gh * gw * gl * 12), np.zeros(gh * gw * gl, bool)
    for j, i, l, wyx, wz, dz in _corners(co):
        gc = g[j, i, l]
        wgt = wyx * wz
        a += wgt[..., None] * gc
        da += (wyx * dz)[..., None] * gc
        mass_a += np.abs(wgt)[..., None] * (np.abs(gc).reshape(h, w, 3, 4)[..., :3] * np.abs(vd[..., :3])[:, :, :, None]).sum(2)
        mass_d += np.abs(wyx) * (np.abs(gc) * np.abs(o)).sum(-1)
        cell = ((j * gw + i) * gl + l).reshape(-1)
        reached[cell] = True
        for q in range(12):
            t = (wgt * o[..., q]).reshape(-1)
            v_g += np.bincount(cell * 12 + q, weights=t, minlength=v_g.size)
            s += np.bincount(cell * 12 + q, weights=np.abs(t), minlength=s.size)
    scale = float(gl - 1) * co["inside"]
    guide = scale * (da * o).sum(-1)
    lum = np.array(LUM)
    v_img = vd.copy()
    v_img[..., :3] = (a.reshape(h, w, 3, 4)[..., :3] * vd[..., :3, None]).sum(2) + guide[..., None] * lum
    mass_v = mass_a + (scale * mass_d)[..., None] * lum
    return dict(v_img=v_img, mass_v=mass_v, v_g=v_g.reshape(g.shape), S=s.reshape(g.shape), reached=reached.reshape(gh, gw, gl))


def total_variation(g):
    """(TV, dTV/dg) of one grid: sum over the axes z, y, x of sum (g[+1] - g)^2 / count, count = the differences over all twelve
    coefficients; an axis of one vertex contributes nothing."""
    g = np.asarray(g, np.float64)
    tv, grad = 0.0, np.zeros_like(g)
    for axis in (2, 0, 1):
        n = g.shape[axis]
        if n < 2:
            continue
        hi, lo = [slice(None)] * 4, [slice(None)] * 4
        hi[axis], lo[axis] = slice(1, n), slice(0, n - 1)
        d = g[tuple(hi)] - g[tuple(lo)]
        tv += float((d * d).sum()) / d.size
        grad[tuple(hi)] += 2.0 * d / d.size
        grad[tuple(lo)] -= 2.0 * d / d.size
    return tv, grad


def adam_step(param, m1, m2, t, g, lr, beta1=0.9, beta2=0.999, eps=1e-15):
    """One Adam step in f64, the library's operations in its order, from the stored (f32) moments: -> (param, m1, m2, t), the
    parameter moved by the unrounded moments, which the library then stores rounded to f32."""
    param, m1, m2, g = (np.asarray(v, np.float64) for v in (param, m1, m2, g))
    t = int(t) + 1
    m1 = beta1 * m1 + (1.0 - beta1) * g
    m2 = beta2 * m2 + (1.0 - beta2) * g * g
    ah = m1 / (1.0 - beta1 ** float(t))
    bh = m2 / (1.0 - beta2 ** float(t))
    return param - lr * ah / (np.sqrt(bh) + eps), m1, m2, t


def smooth_grid(grid_h, grid_w, grid_l, strength=0.25):
    """A known smooth grid for the recovery tests: a vignette-like gain that falls towards the corners and rises with the level,
    one cross term and an offset that drifts across the frame."""
    g = identity_grid(grid_h, grid_w, grid_l)
    jj = np.linspace(-1.0, 1.0, grid_h)[:, None, None] if grid_h > 1 else np.zeros((1, 1, 1))
    ii = np.linspace(-1.0, 1.0, grid_w)[None, :, None] if grid_w > 1 else np.zeros((1, 1, 1))
    ll = np.linspace(0.0, 1.0, grid_l)[None, None, :] if grid_l > 1 else np.zeros((1, 1, 1))
    gain = 1.0 - strength * 0.5 * (jj * jj + ii * ii) + 0.5 * strength * ll
    for k in (0, 5, 10):
        g[..., k] = gain
    g[..., 1] = 0.2 * strength * ii
    g[..., 7] = 0.1 * strength * jj
    return g


def case_inputs(w, h, shape, seed):
    """The GPU tests' inputs: x uniform in -0.2 .. 1.2 with one row of exact 0.0 and one of exact 1.0, v' uniform in +-1, the grid
    identity +- 0.3: (x, v, g) as float32."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.2, 1.2, (h, w, 4)).astype(np.float32)
    x[0, :, :3] = 0.0
    x[h - 1, :, :3] = 1.0
    v = rng.uniform(-1.0, 1.0, (h, w, 4)).astype(np.float32)
    g = (identity_grid(*shape) + rng.uniform(-0.3, 0.3, tuple(shape) + (12,))).astype(np.float32)
    return x, v, g
