"""Numpy restatement of include/brush_hip_envmap.h: the ray of a pixel, its cube face and four taps, the composite of
a frame over the map, the gradient to the frame, the exact integer gradient to the table with the terms its error bound is made of,
and the f32 Adam step.  This file IS the specification: every operation is the header's, in the header's order and precision, and the
GPU tests hold the kernels to it bit for bit.  A camera here is a dict(vm=[12] world-to-camera column-major, fx, fy, cx, cy)."""
import numpy as np

F = np.float32


def fma32(a, b, c):
    """fma(a, b, c) of f32 arrays, correctly rounded: the product is exact in f64, the f64 sum is turned into its round-to-odd value
    with the error term of TwoSum, and a round-to-odd f64 rounds to f32 as the exact value does (53 >= 2 * 24 + 2)."""
    a, b, c = np.asarray(a, F), np.asarray(b, F), np.asarray(c, F)
    p = a.astype(np.float64) * b.astype(np.float64)
    cc = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + cc
        bb = s - p
        err = (p - (s - bb)) + (cc - bb)
        bits = s.view(np.int64) if isinstance(s, np.ndarray) else np.float64(s).view(np.int64)
        even = (bits & 1) == 0
        fix = np.isfinite(s) & (err != 0.0) & even
        toward = np.where(err > 0.0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(F)


def look_at(direction, up=(0.0, 0.0, 1.0), position=(0.0, 0.0, 0.0)):
    """vm[12] of a camera at `position` whose +z looks along `direction`, x to the right, y down."""
    z = np.asarray(direction, np.float64)
    z = z / np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    r = np.stack([x, y, z])                       # world-to-camera rotation: the rows are the camera's axes
    t = -r @ np.asarray(position, np.float64)
    return np.concatenate([r.T.reshape(-1), t]).astype(F)   # column-major: column c is r[:, c]


def camera(w, h, fov_deg, direction=(1.0, 1.0, 1.0)):
    """The test camera: `fov_deg` across the width, principal point at the centre."""
    f = F(0.5 * w / np.tan(np.radians(fov_deg) * 0.5))
    return dict(vm=look_at(direction), fx=f, fy=f, cx=F(0.5 * w), cy=F(0.5 * h))


def rays(cam, h, w):
    """d [h,w,3] f32 of every pixel."""
    vm = np.asarray(cam["vm"], F)
    x = np.arange(w, dtype=F)[None, :] + F(0.5)
    y = np.arange(h, dtype=F)[:, None] + F(0.5)
    dx = np.broadcast_to((x - F(cam["cx"])) / F(cam["fx"]), (h, w))
    dy = np.broadcast_to((y - F(cam["cy"])) / F(cam["fy"]), (h, w))
    return np.stack([fma32(vm[3 * i + 1], dy, vm[3 * i] * dx) + vm[3 * i + 2] for i in range(3)], axis=-1)


def _axis(s, res):
    half = F(res) * F(0.5)
    u = fma32(s, half, half) - F(0.5)
    u = np.fmin(np.fmax(u, F(0.0)), F(res - 1))   # (fmax / fmin: a NaN becomes 0)
    fl = np.floor(u)
    i0 = fl.astype(np.int64)
    return i0, np.minimum(i0 + 1, res - 1), (u - fl).astype(F)


def taps(cam, h, w, res):
    """-> (texel [h,w,4] int64 = (face R + j) R + i of the four taps, weight [h,w,4] f32)."""
    d = rays(cam, h, w)
    ad = np.abs(d)
    axis = np.zeros((h, w), np.int64)
    am = ad[..., 0].copy()
    for k in (1, 2):
        m = ad[..., k] > am
        axis[m] = k
        am[m] = ad[..., k][m]
    major = np.take_along_axis(d, axis[..., None], -1)[..., 0]
    a = np.take_along_axis(d, ((axis + 1) % 3)[..., None], -1)[..., 0]
    b = np.take_along_axis(d, ((axis + 2) % 3)[..., None], -1)[..., 0]
    face = 2 * axis + (major < 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        i0, i1, fu = _axis(a / am, res)
        j0, j1, fv = _axis(b / am, res)
    gu, gv = F(1.0) - fu, F(1.0) - fv
    row0, row1 = (face * res + j0) * res, (face * res + j1) * res
    texel = np.stack([row0 + i0, row0 + i1, row1 + i0, row1 + i1], -1)
    weight = np.stack([gu * gv, fu * gv, gu * fv, fu * fv], -1).astype(F)
    return texel, weight


def colour(table, texel, weight):
    """E(d) [h,w,3] f32."""
    e = np.asarray(table, F).reshape(-1, 3)[texel]   # [h,w,4,3]
    wk = [weight[..., k, None] for k in range(4)]
    return fma32(wk[3], e[..., 3, :], fma32(wk[2], e[..., 2, :], fma32(wk[1], e[..., 1, :], wk[0] * e[..., 0, :])))


def composite(table, img, cam):
    img = np.asarray(img, F)
    h, w = img.shape[:2]
    res = np.asarray(table).shape[1]
    texel, weight = taps(cam, h, w, res)
    out = img.copy()
    out[..., :3] = fma32((F(1.0) - img[..., 3])[..., None], colour(table, texel, weight), img[..., :3])
    return out


def scale_of(m, pixels):
    """(e, L, S) of the quantisation for the finite maximum m > 0."""
    _, e = np.frexp(np.float64(m))
    log_pixels = (int(pixels) - 1).bit_length()   # ceil(log2(pixels))
    return int(e), log_pixels, np.ldexp(1.0, 61 - int(e) - log_pixels)


def backward(table, img, v, cam):
    """-> dict(v_img [h,w,4] f32, sky [h,w] f32 = sum_c v_c E_c (what v_img_a is v_a minus), v_E [6,R,R,3] f32, acc the int64 sums, S, touched [6,R,R] bool, contrib_abs [6,R,R,3] f64 =
    sum |g w_k|, count [6,R,R] = contributions per texel-channel, m).  Raises ValueError on a non-finite m."""
    img, v = np.asarray(img, F), np.asarray(v, F)
    h, w = img.shape[:2]
    table = np.asarray(table, F)
    res = table.shape[1]
    texel, weight = taps(cam, h, w, res)
    # the sky's term in f64 (every w e product is exact there), rounded to f32 once
    tex = table.reshape(-1, 3)[texel].astype(np.float64)   # [h,w,4,3]
    wk = [weight[..., k, None].astype(np.float64) for k in range(4)]
    e64 = wk[3] * tex[..., 3, :] + (wk[2] * tex[..., 2, :] + (wk[1] * tex[..., 1, :] + wk[0] * tex[..., 0, :]))
    v64 = v.astype(np.float64)
    s = (v64[..., 2] * e64[..., 2] + (v64[..., 1] * e64[..., 1] + v64[..., 0] * e64[..., 0])).astype(F)
    v_img = v.copy()
    v_img[..., 3] = v[..., 3] - s
    with np.errstate(invalid="ignore"):
        m = np.abs(v[..., :3]).max()
    if not np.isfinite(m):
        raise ValueError("non-finite cotangent")
    cells = 6 * res * res
    acc = np.zeros((cells, 3), np.int64)
    contrib_abs = np.zeros((cells, 3), np.float64)
    count = np.zeros(cells, np.int64)
    touched = np.zeros(cells, bool)
    S = 1.0
    if m > 0:
        _, _, S = scale_of(m, h * w)
        oma = F(1.0) - img[..., 3]
        on = oma != 0
        g = (oma[..., None] * v[..., :3]).astype(F)[on]        # [n,3]
        tx, wk = texel[on], weight[on]                           # [n,4]
        for k in range(4):
            gw = (g * wk[:, k, None]).astype(F)
            q = np.rint(gw.astype(np.float64) * S).astype(np.int64)
            np.add.at(acc, tx[:, k], q)
            np.add.at(contrib_abs, tx[:, k], np.abs(gw.astype(np.float64)))
            np.add.at(count, tx[:, k], 1)
            touched[tx[:, k]] = True
    v_e = (acc.astype(np.float64) / S).astype(F)
    shape = (6, res, res)
    return dict(v_img=v_img, sky=s, v_E=v_e.reshape(shape + (3,)), acc=acc.reshape(shape + (3,)), S=S, touched=touched.reshape(shape),
                contrib_abs=contrib_abs.reshape(shape + (3,)), count=count.reshape(shape), m=m)


def pow_by_squaring(b, t):
    p, b, t = 1.0, float(b), int(t)
    while t:
        if t & 1:
            p = p * b
        b = b * b
        t >>= 1
    return p


def adam_step(param, m1, m2, t, g, lr, beta1=0.9, beta2=0.999, eps=1e-15):
    """One f32 Adam step of every texel, the library's operations in its order: -> (param, m1, m2, t)."""
    param, m1, m2, g = (np.asarray(a, F) for a in (param, m1, m2, g))
    t = int(t) + 1
    c1, c2 = F(1.0 - pow_by_squaring(beta1, t)), F(1.0 - pow_by_squaring(beta2, t))
    b1, b2, o1, o2 = F(beta1), F(beta2), F(1.0 - beta1), F(1.0 - beta2)
    n1 = b1 * m1 + o1 * g
    n2 = b2 * m2 + (o2 * g) * g
    new = param - F(lr) * ((n1 / c1) / (np.sqrt(n2 / c2) + F(eps)))
    return new.astype(F), n1.astype(F), n2.astype(F), t


def scene(res, w=64, h=48, fov_deg=100.0, seed=0, direction=(1.0, 1.0, 1.0)):
    """The shared test case: a camera looking down (1,1,1) (three faces and a cube corner in view), a random table, frame and
    cotangent, alpha random with 30 % of the pixels exactly 1."""
    rng = np.random.default_rng(seed * 100003 + res * 1009 + w * 31 + h)
    cam = camera(w, h, fov_deg, direction)
    table = rng.uniform(0.0, 1.0, (6, res, res, 3)).astype(F)
    img = rng.uniform(0.0, 1.0, (h, w, 4)).astype(F)
    img[..., 3][rng.uniform(size=(h, w)) < 0.3] = 1.0
    v = rng.uniform(-1.0, 1.0, (h, w, 4)).astype(F)
    return dict(cam=cam, table=table, img=img, v=v, res=res, w=w, h=h)
