"""Float64 torch restatement of oracle/autograd_ref.py::render with the camera intrinsics as a leaf — TEST INFRASTRUCTURE ONLY.

The renderer is tests/pose_ref.py's (and so autograd_ref.render's, statement for statement: tests/test_intrinsics_ref.py pins the
images against each other), its helpers imported unchanged, with these differences that leave the image as it is
(include/brush_hip_intrinsics.h):

  * k = (fx, fy, cx, cy) is a tensor, by default the camera's values; the clamp limits and the cull angle stay the camera's
    (constants of the gradient);
  * the lens laws are restated as the normalised distorted coordinate d(p) = (xd, yd), the pixel being k[0:2] * d + k[2:4]
    (autograd_ref._project takes the intrinsics as floats of its formulas; the laws themselves are the same);
  * every splat gets its OWN copy k_i of the four, so that one backward returns the per-splat contributions: their sum is
    v_intrinsics, the sum of their absolute values the L1 mass S_k the tolerances are stated in;
  * the pixel means, the raw covariance and the conic are kept as graph nodes with their gradients (v_xy, v_conic): what the header's
    per-splat formula is evaluated on;
  * the accumulated and the expected depth (tests/depth_ref.py's definitions) are returned beside the image.
"""
import numpy as np
import torch

from oracle.autograd_ref import _quat_to_mat, _sh_color, camera_matrices
from pose_ref import intrinsics, tie_mask  # noqa: F401  (re-exported: the callers' camera set-up and tie band)


def lens(model, dist, p):
    """p [N,3] camera-space points -> (xd, yd) [N]: the distorted normalised coordinate of the lens law, free of the intrinsics."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    if model == "pinhole":
        return x / z, y / z
    if model == "rt8":
        k1, k2, k3, k4, k5, k6, p1, p2 = [float(v) for v in dist]
        xn, yn = x / z, y / z
        r2 = xn * xn + yn * yn
        r4, r6 = r2 * r2, r2 * r2 * r2
        d = (1.0 + k1 * r2 + k2 * r4 + k3 * r6) / (1.0 + k4 * r2 + k5 * r4 + k6 * r6)
        return (xn * d + 2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn), yn * d + 2.0 * p2 * xn * yn + p1 * (r2 + 2.0 * yn * yn))
    k1, k2, k3, k4 = [float(v) for v in dist[:4]]
    r = torch.sqrt(x * x + y * y)
    th = torch.atan2(r, z)
    t2 = th * th
    d = th * (1.0 + k1 * t2 + k2 * t2 * t2 + k3 * t2 * t2 * t2 + k4 * t2 * t2 * t2 * t2)
    u, v = d * x / r, d * y / r
    if model == "kb4":
        return u, v
    assert model == "tpf"
    p1, p2, sx1, sy1 = [float(v) for v in dist[4:8]]
    r2 = x * x + y * y
    nu = 2.0 * p1 * x * y + p2 * (3.0 * x * x + y * y) + sx1 * r2
    nv = 2.0 * p2 * x * y + p1 * (x * x + 3.0 * y * y) + sy1 * r2
    return u + nu / (z * z), v + nv / (z * z)


def intrinsics_of(cam, w, h, intr=None):
    """(fx, fy, cx, cy) float64 numpy of a camera dict: camera_matrices' for a pinhole, the camera set-up's (`intr`) for a lens."""
    if cam.get("model", "pinhole") != "pinhole":
        return np.array([intr["fx"], intr["fy"], intr["cx"], intr["cy"]], np.float64)
    return np.array(camera_matrices(cam["pos"], cam["rot_xyzw"], cam["fov_x"], cam["fov_y"], cam["center_uv"], w, h)[2], np.float64)


def render(transforms, sh, raw_opac, cam, w, h, bg=(0.0, 0.0, 0.0), intrinsics=None, mip=False, smooth=False, comp_is_constant=True, k=None):
    """Arguments as autograd_ref.render; k = (fx, fy, cx, cy) a float64 tensor [4] or None (the camera's own).  Returns dict(img
    [h,w,4], acc, expected [h,w], k_n [N,4]: the per-splat copies (leaves of their own when k requires a gradient), xy [N,2], cov_raw
    [N,2,2], conic [N,3] = (c00, c01, c11), d [N,2] = (xd, yd): graph nodes that keep their gradient, tie_alpha, tie_t [h,w])."""
    dt = torch.float64
    r_np, t_np, _, lim = camera_matrices(cam["pos"], cam["rot_xyzw"], cam["fov_x"], cam["fov_y"], cam["center_uv"], w, h)
    model = cam.get("model", "pinhole")
    if model != "pinhole":
        lim = intrinsics["lim"]
    if k is None:
        k = torch.tensor(intrinsics_of(cam, w, h, intrinsics), dtype=dt)
    rc, tc = torch.tensor(r_np, dtype=dt), torch.tensor(t_np, dtype=dt)
    mean, quat, log_s = transforms[:, 0:3], transforms[:, 3:7], transforms[:, 7:10]
    n = transforms.shape[0]
    k_n = k.unsqueeze(0).repeat(n, 1)
    if k_n.requires_grad:
        k_n.retain_grad()
    fx, fy, cx, cy = k_n[:, 0], k_n[:, 1], k_n[:, 2], k_n[:, 3]
    mean_c = mean @ rc.T + tc
    zc = mean_c[:, 2]
    if model == "pinhole":
        keep = (zc >= 0.01) & (zc <= 1e10)
    else:
        theta = torch.atan2(torch.sqrt(mean_c[:, 0] ** 2 + mean_c[:, 1] ** 2), zc)
        keep = (theta <= intrinsics["half_max_render_fov"]) & (zc <= 1e10)
    q = quat / quat.norm(dim=1, keepdim=True)
    m = _quat_to_mat(q) * torch.exp(log_s)[:, None, :]
    cov_c = rc @ (m @ m.transpose(1, 2)) @ rc.T
    xz = torch.clamp(mean_c[:, 0] / zc, lim[2], lim[0])
    yz = torch.clamp(mean_c[:, 1] / zc, lim[3], lim[1])
    zero = torch.zeros_like(zc)
    if model == "pinhole":
        jac = torch.stack([torch.stack([fx / zc, zero, -fx / zc * xz], -1), torch.stack([zero, fy / zc, -fy / zc * yz], -1)], -2)
    else:
        q = torch.stack([xz * zc, yz * zc, zc], -1) if model == "rt8" else mean_c
        if not q.requires_grad:
            q = q.detach().requires_grad_(True)
        ju, jv = lens(model, cam["dist"], q)
        ru = torch.autograd.grad((fx * ju + cx).sum(), q, create_graph=True)[0]
        rv = torch.autograd.grad((fy * jv + cy).sum(), q, create_graph=True)[0]
        jac = torch.stack([ru, rv], -2)
    cov2 = jac @ cov_c @ jac.transpose(1, 2)
    blur = 0.1 if mip else 0.3
    det_raw = torch.clamp(cov2[:, 0, 0] * cov2[:, 1, 1] - cov2[:, 0, 1] * cov2[:, 0, 1], min=0.0)
    a, b, c = cov2[:, 0, 0] + blur, cov2[:, 0, 1], cov2[:, 1, 1] + blur
    det = a * c - b * b
    conic = torch.stack([c / det, -b / det, a / det], -1)
    xd, yd = lens(model, cam.get("dist", ()), mean_c)
    xy = torch.stack([fx * xd + cx, fy * yd + cy], -1)
    for node in (conic, xy):
        if node.requires_grad:
            node.retain_grad()
    c00, c01, c11 = conic[:, 0], conic[:, 1], conic[:, 2]
    mx, my = xy[:, 0], xy[:, 1]
    alpha0 = torch.sigmoid(raw_opac)
    if mip:
        comp = torch.sqrt(det_raw / det)
        alpha0 = alpha0 * (comp.detach() if comp_is_constant else comp)
    cam_pos = torch.tensor(np.asarray(cam["pos"], np.float64), dtype=dt)
    vd = mean - cam_pos
    vd = vd / vd.norm(dim=1, keepdim=True)
    color = torch.clamp(_sh_color(sh, vd) + 0.5, -100.0, 100.0)
    color = torch.clamp(color, min=0.0)
    keep = keep & (alpha0 >= 1.0 / 255.0)

    py, px = torch.meshgrid(torch.arange(h, dtype=dt) + 0.5, torch.arange(w, dtype=dt) + 0.5, indexing="ij")
    T = torch.ones((h, w), dtype=dt)
    rgb = torch.zeros((h, w, 3), dtype=dt)
    acc = torch.zeros((h, w), dtype=dt)
    done = torch.zeros((h, w), dtype=torch.bool)
    inf = torch.full((h, w), float("inf"), dtype=dt)
    tie_alpha, tie_t = inf.clone(), inf.clone()
    order = torch.argsort(zc.detach(), stable=True)
    for i in order.tolist():
        if not bool(keep[i]):
            continue
        dx, dy = px - mx[i], py - my[i]
        sigma = 0.5 * (c00[i] * dx * dx + c11[i] * dy * dy) + c01[i] * dx * dy
        alpha = torch.clamp(alpha0[i] * torch.exp(-sigma), max=0.999)
        live = (sigma >= 0) & ~done
        with torch.no_grad():
            tie_alpha = torch.where(live, torch.minimum(tie_alpha, (alpha - 1.0 / 255.0).abs()), tie_alpha)
        if smooth:
            tt = torch.clamp((alpha - (1.0 / 255.0 - 0.5e-3)) / 1.0e-3, 0.0, 1.0)
            w_cut = tt * tt * (3.0 - 2.0 * tt)
            ok = (sigma >= 0) & (w_cut > 0) & ~done
            alpha = alpha * w_cut
        else:
            ok = (sigma >= 0) & (alpha >= 1.0 / 255.0) & ~done
        next_t = T * (1.0 - alpha)
        sat = ok & (next_t <= 1e-4)
        contrib = ok & ~sat
        with torch.no_grad():
            tie_t = torch.where(ok, torch.minimum(tie_t, (next_t - 1e-4).abs()), tie_t)
        vis = torch.where(contrib, alpha * T, torch.zeros_like(T))
        rgb = rgb + vis[..., None] * color[i]
        acc = acc + vis * zc[i]
        T = torch.where(contrib, next_t, T)
        done = done | sat
    bgt = torch.tensor(bg, dtype=dt)
    img = torch.cat([rgb + T[..., None] * bgt, (1.0 - T)[..., None]], dim=-1)
    A = 1.0 - T
    expected = torch.where(A > 0, acc / torch.where(A > 0, A, torch.ones_like(A)), torch.zeros_like(A))
    return dict(img=img, acc=acc, expected=expected, k_n=k_n, xy=xy, cov_raw=cov2, conic=conic, d=torch.stack([xd, yd], -1), tie_alpha=tie_alpha,
                tie_t=tie_t)


def intrinsics_gradients(scene, cam, w, h, v_output, bg=(0.0, 0.0, 0.0), intrinsics=None, mip=False, smooth=False, k=None, skip_ties=False,
                         v_depth=None):
    """Gradients of <v_output, image> [+ <v_depth, expected depth>] with respect to (fx, fy, cx, cy) and the splats; numpy float64 in
    and out.  skip_ties: both cotangents are zeroed on tie_mask's pixels first (the returned `v_output`, `v_depth` are what was
    used, `ties` the mask).
    Returns dict(img, expected, v_intrinsics [4], S [4], per_splat [N,4], v_intrinsics_leaf [4], v_transforms, v_sh, v_raw_opac, k [4],
    v_xy [N,2], v_conic [N,3], cov_raw [N,2,2], conic [N,3], d [N,2], ties, v_output, v_depth)."""
    tr = torch.tensor(np.asarray(scene["transforms"], np.float64), requires_grad=True)
    sh = torch.tensor(np.asarray(scene["sh"], np.float64), requires_grad=True)
    op = torch.tensor(np.asarray(scene["raw_opac"], np.float64), requires_grad=True)
    k_np = intrinsics_of(cam, w, h, intrinsics) if k is None else np.asarray(k, np.float64)
    kt = torch.tensor(k_np, requires_grad=True)
    out = render(tr, sh, op, cam, w, h, bg, intrinsics, mip, smooth, k=kt)
    ties = tie_mask(out, smooth).numpy()
    v = np.array(v_output, np.float64)
    vd = None if v_depth is None else np.array(v_depth, np.float64)
    if skip_ties:
        v[ties] = 0.0
        if vd is not None:
            vd[ties] = 0.0
    loss = (out["img"] * torch.tensor(v)).sum()
    if vd is not None:
        loss = loss + (out["expected"] * torch.tensor(vd)).sum()
    loss.backward()
    n = tr.shape[0]
    z = lambda g, x: np.zeros(tuple(x.shape)) if g is None else g.numpy()
    per = z(out["k_n"].grad, out["k_n"])
    return dict(img=out["img"].detach().numpy(), expected=out["expected"].detach().numpy(), v_intrinsics=per.sum(0), S=np.abs(per).sum(0),
                per_splat=per, v_intrinsics_leaf=z(kt.grad, kt), v_transforms=z(tr.grad, tr), v_sh=z(sh.grad, sh), v_raw_opac=z(op.grad, op),
                k=k_np, v_xy=z(out["xy"].grad, out["xy"]), v_conic=z(out["conic"].grad, out["conic"]), cov_raw=out["cov_raw"].detach().numpy(),
                conic=out["conic"].detach().numpy(), d=out["d"].detach().numpy(), ties=ties, v_output=v, v_depth=vd, n=n)


# ---- the header's per-splat formula, in f64 -------------------------------------------------------------------------------------
def inverse2x2_vjp(minv, v):
    """device_math.h's inverse2x2_vjp on rows (c00, c01, c11): -minv v minv as full symmetric matrices."""
    m00, m01, m11 = minv[:, 0], minv[:, 1], minv[:, 2]
    v00, v01, v11 = v[:, 0], v[:, 1], v[:, 2]
    t00 = -m00 * v00 - m01 * v01
    t01 = -m01 * v00 - m11 * v01
    t10 = -m00 * v01 - m01 * v11
    t11 = -m01 * v01 - m11 * v11
    return np.stack([t00 * m00 + t10 * m01, t01 * m00 + t11 * m01, t01 * m01 + t11 * m11], -1)


def header_formula(k, v_xy, v_conic, conic, cov_raw, d):
    """brush_hip_intrinsics.h, per splat [N,4]: g = (v_xy, v_conic), G = inverse2x2_vjp(conic, {g2, g3 / 2, g4}), A = cov_raw."""
    fx, fy = k[0], k[1]
    g0, g1 = v_xy[:, 0], v_xy[:, 1]
    G = inverse2x2_vjp(conic, np.stack([v_conic[:, 0], 0.5 * v_conic[:, 1], v_conic[:, 2]], -1))
    a00, a01, a11 = cov_raw[:, 0, 0], cov_raw[:, 0, 1], cov_raw[:, 1, 1]
    return np.stack([g0 * d[:, 0] + 2.0 * (G[:, 0] * a00 + G[:, 1] * a01) / fx, g1 * d[:, 1] + 2.0 * (G[:, 2] * a11 + G[:, 1] * a01) / fy, g0, g1], -1)
