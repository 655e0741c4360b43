"""Restatements for scene editing (include/brush_hip_scene.h), numpy only:
  * sh_rotation_matrices: the rotation matrices of the SH bands in f64, by least squares over 200 Fibonacci directions on an f64 copy of
    the basis of brush_amd/csrc/device_sh.h (its f32 constants, its signs);
  * make_record: what bh_scene_transform_make fills; camera_apply: the camera formulas;
  * transform_f32 / select_region_f32: the float32 arithmetic of bh_splats_transform and bh_splats_select_region, operation by operation
    (numpy rounds every float32 multiply and add on its own), so the kernels are compared bit for bit;
  * the scenes and the criterion of the end-to-end invariant, shared by the CPU test (the oracle) and the GPU test."""
import math

import numpy as np

SH_ROT_OFFSET = (0, 0, 9, 34, 83)
F = np.float32


def _c(x):
    return float(np.float32(x))   # a constant of device_sh.h as the f32 the kernels hold


def sh_basis(d):
    """[n,25] f64: the basis of device_sh.h at the unit directions d [n,3]."""
    d = np.asarray(d, np.float64).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    b = np.empty((d.shape[0], 25), np.float64)
    b[:, 0] = _c(0.2820948)
    f0a = _c(0.4886025)
    b[:, 1], b[:, 2], b[:, 3] = -f0a * y, f0a * z, -f0a * x
    z2 = z * z
    f0b = _c(-1.0925485) * z
    f1a = _c(0.54627424)
    fc1, fs1 = x * x - y * y, 2.0 * x * y
    b[:, 4], b[:, 5] = f1a * fs1, f0b * y
    b[:, 6] = _c(0.9461747) * z2 - _c(0.31539157)
    b[:, 7], b[:, 8] = f0b * x, f1a * fc1
    f0c = _c(-2.285229) * z2 + _c(0.4570458)
    f1b = _c(1.4453057) * z
    f2a = _c(-0.5900436)
    fc2, fs2 = x * fc1 - y * fs1, x * fs1 + y * fc1
    p12 = z * (_c(1.8658817) * z2 - _c(1.119529))
    b[:, 9], b[:, 10], b[:, 11], b[:, 12], b[:, 13], b[:, 14], b[:, 15] = f2a * fs2, f1b * fs1, f0c * y, p12, f0c * x, f1b * fc1, f2a * fc2
    f0d = z * (_c(-4.683326) * z2 + _c(2.0071396))
    f1c = _c(3.3116114) * z2 - _c(0.47308735)
    f2b = _c(-1.7701308) * z
    f3a = _c(0.62583575)
    fc3, fs3 = x * fc2 - y * fs2, x * fs2 + y * fc2
    b[:, 16], b[:, 17], b[:, 18], b[:, 19] = f3a * fs3, f2b * fs2, f1c * fs1, f0d * y
    b[:, 20] = _c(1.9843135) * z * p12 - _c(1.0062306) * b[:, 6]
    b[:, 21], b[:, 22], b[:, 23], b[:, 24] = f0d * x, f1c * fc1, f2b * fc2, f3a * fc3
    return b


def fibonacci_directions(n=200):
    i = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / n
    r = np.sqrt(1.0 - z * z)
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def sh_rotation_matrices(R, degree=4):
    """[D_1 .. D_degree] f64: with a' = D_l a, sum_k a'_k Y_k(d) = sum_k a_k Y_k(R^T d) for every unit d."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    dirs = fibonacci_directions(200)
    A, B = sh_basis(dirs), sh_basis(dirs @ R)   # rows of dirs @ R are R^T d
    out = []
    for l in range(1, degree + 1):
        sl = slice(l * l, (l + 1) * (l + 1))
        out.append(np.linalg.lstsq(A[:, sl], B[:, sl], rcond=None)[0])
    return out


def quat_to_matrix(q):
    w, x, y, z = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], np.float64)


def make_record(q_wxyz, t, s):
    """The fields of BhSceneTransform for x' = s R(q) x + t."""
    q = np.asarray(q_wxyz, np.float64)
    q = q / np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    R = quat_to_matrix(q)
    sh_rot = np.concatenate([d.reshape(-1) for d in sh_rotation_matrices(R)])
    t = np.asarray(t, np.float64)
    return dict(q=q, t=t, s=float(s), R=R, rot=R.reshape(-1).astype(F), quat=q.astype(F), trans=t.astype(F), scale=F(s), log_scale=F(math.log(s)),
                sh_rot=sh_rot.astype(F))


def record_from_struct(rec):
    """The same dictionary from a library record (ctypes BhSceneTransform): the kernels read its f32 fields."""
    q = np.array(list(rec.q), np.float64)
    return dict(q=q, t=np.array(list(rec.t), np.float64), s=float(rec.s), R=quat_to_matrix(q), rot=np.array(list(rec.rot), F), quat=np.array(list(rec.quat), F),
                trans=np.array(list(rec.trans), F), scale=F(rec.scale), log_scale=F(rec.log_scale), sh_rot=np.array(list(rec.sh_rot), F))


def transform_f32(rec, transforms, sh=None, min_scale=None):
    """bh_splats_transform in float32, every multiply and add rounded on its own -> (transforms', sh' or None, min_scale' or None)."""
    with np.errstate(all="ignore"):
        tr = np.array(transforms, F).reshape(-1, 10)
        r, qu, tv, sc, ls = rec["rot"].astype(F), rec["quat"].astype(F), rec["trans"].astype(F), F(rec["scale"]), F(rec["log_scale"])
        out = np.empty_like(tr)
        x, y, z = tr[:, 0], tr[:, 1], tr[:, 2]
        for i in range(3):
            out[:, i] = ((r[3 * i] * x + r[3 * i + 1] * y) + r[3 * i + 2] * z) * sc + tv[i]
        W, X, Y, Z = qu
        w, qx, qy, qz = tr[:, 3], tr[:, 4], tr[:, 5], tr[:, 6]
        out[:, 3] = ((W * w - X * qx) - Y * qy) - Z * qz
        out[:, 4] = ((W * qx + X * w) + Y * qz) - Z * qy
        out[:, 5] = ((W * qy - X * qz) + Y * w) + Z * qx
        out[:, 6] = ((W * qz + X * qy) - Y * qx) + Z * w
        out[:, 7:10] = tr[:, 7:10] + ls
        osh = None
        if sh is not None:
            shc = np.array(sh, F).reshape(tr.shape[0], -1, 3)
            osh = shc.copy()
            deg = int(round(math.sqrt(shc.shape[1]))) - 1
            for l in range(1, deg + 1):
                m = 2 * l + 1
                D = rec["sh_rot"][SH_ROT_OFFSET[l]:SH_ROT_OFFSET[l] + m * m].astype(F).reshape(m, m)
                band = shc[:, l * l:(l + 1) * (l + 1), :]
                for k in range(m):
                    acc = D[k, 0] * band[:, 0, :]
                    for j in range(1, m):
                        acc = acc + D[k, j] * band[:, j, :]
                    osh[:, l * l + k, :] = acc
        oms = None if min_scale is None else np.array(min_scale, F).reshape(-1) * sc
    return out, osh, oms


def select_region_f32(region, transforms, raw_opac=None):
    """bh_splats_select_region in float32 -> keep [N] (1.0 / 0.0).  region: dict(kind 0 box / 1 ellipsoid, invert, center, half_extent,
    rot [9] row-major, min_raw_opacity)."""
    with np.errstate(all="ignore"):
        tr = np.array(transforms, F).reshape(-1, 10)
        c, h, r = np.array(region["center"], F), np.array(region["half_extent"], F), np.array(region["rot"], F).reshape(-1)
        x, y, z = tr[:, 0], tr[:, 1], tr[:, 2]
        dx, dy, dz = x - c[0], y - c[1], z - c[2]
        p = [(r[i] * dx + r[3 + i] * dy) + r[6 + i] * dz for i in range(3)]
        if region["kind"] == 0:
            inside = (np.abs(p[0]) <= h[0]) & (np.abs(p[1]) <= h[1]) & (np.abs(p[2]) <= h[2])
        else:
            q = [p[i] / h[i] for i in range(3)]
            inside = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) <= F(1.0)
        if region.get("invert"):
            inside = ~inside
        keep = inside & np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        if raw_opac is not None:
            keep = keep & (np.array(raw_opac, F).reshape(-1) >= F(region.get("min_raw_opacity", -np.inf)))
    return keep.astype(F)


def camera_apply(vm, cam_pos, rec):
    """W' = W R^T, tv' = s tv - W R^T t, cam_pos' = s R p + t in f64 -> (vm' [12] column-major f32, cam_pos' [3] f32)."""
    vm = np.asarray(vm, np.float64).reshape(4, 3)   # rows are the columns of the 3x4 matrix
    W, tv = vm[:3].T, vm[3]
    R, t, s = rec["R"], rec["t"], rec["s"]
    W2 = W @ R.T
    tv2 = s * tv - W2 @ t
    p2 = s * (R @ np.asarray(cam_pos, np.float64)) + t
    return np.concatenate([W2.T.reshape(-1), tv2]).astype(F), p2.astype(F)


# ---- the end-to-end invariant: the transformed scene from the transformed camera is the same image ------------------------------
IMG_W, IMG_H, N_SPLATS = 96, 80, 300
CAM = dict(pos=(0.0, 0.0, 0.0), rot_xyzw=(0.0, 0.0, 0.0, 1.0), fov_x=0.9, fov_y=0.9 * IMG_H / IMG_W, center_uv=(0.5, 0.5))
# (degree, mip, seed): fixed seeds, one case per degree and Mip setting
INVARIANT_CASES = [(deg, mip, 100 + 10 * deg + mip) for deg in range(5) for mip in (0, 1)]


def invariant_case(degree, seed):
    """A scene of 300 splats at depth 3..5 with scales 0.03..0.25 in front of CAM (far from the near plane at every s), and a transform:
    s = e^u with u in [-1, 1], a random rotation and translation."""
    rng = np.random.default_rng(seed)
    n, c = N_SPLATS, (degree + 1) ** 2
    z = rng.uniform(3.0, 5.0, n)
    tx, ty = math.tan(CAM["fov_x"] / 2.0), math.tan(CAM["fov_y"] / 2.0)
    means = np.stack([z * tx * rng.uniform(-0.9, 0.9, n), z * ty * rng.uniform(-0.9, 0.9, n), z], axis=1)
    quats = rng.normal(size=(n, 4))
    log_scales = np.log(rng.uniform(0.03, 0.25, (n, 3)))
    sh = rng.uniform(-0.5, 0.5, (n, c, 3))
    sh[:, 0, :] = rng.uniform(0.2, 1.6, (n, 3))
    raw_opac = rng.uniform(-1.0, 3.0, n)
    q = rng.normal(size=4)
    t = rng.uniform(-2.0, 2.0, 3)
    s = math.exp(rng.uniform(-1.0, 1.0))
    return dict(transforms=np.concatenate([means, quats, log_scales], axis=1).astype(F), sh=sh.astype(F), raw_opac=raw_opac.astype(F)), (q, t, s)


def assert_same_image(a, b):
    """The criterion: per-pixel max-abs difference <= 1e-4 (twice the largest ordinary difference measured on the oracle, 4.5e-5) except
    at no more than 4 of the 7680 pixels, where a splat crosses the 1/255 alpha cut or the 3 sigma edge; none above 1e-2 = (1/255) x the
    largest colour magnitude of about 1.6."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).reshape(IMG_H * IMG_W, -1).max(axis=1)
    over = int((d > 1e-4).sum())
    print("invariant: max %.3e, %d pixels over 1e-4, %d over 5e-5" % (d.max(), over, int((d > 5e-5).sum())))
    assert over <= 4, (over, float(d.max()))
    assert float(d.max()) <= 1e-2, float(d.max())
    return float(d.max())
