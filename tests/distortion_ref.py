"""Float64 torch restatement of oracle/autograd_ref.py::render's loop that also folds the distortion map — TEST INFRASTRUCTURE ONLY
(include/brush_hip_distortion.h).

Built like tests/depth_ref.py and tests/normal_ref.py: the set-up in front of the loop and the loop's alpha / cut-off / saturation
rule are autograd_ref.render's, statement for statement (tests/test_distortion_ref.py pins the RGBA against depth_ref.render's,
exactly); the helpers of those files are imported unchanged.  Beside the colour, the depth and the normals the loop folds, per pixel
and with the blend's own weight w_i = T_i alpha_i and the per-splat depth m_i (splat_depth below):

  A = sum of w_i = 1 - T_final,   M1 = sum of w_i m_i,   M2 = sum of w_i m_i^2
  dist = A M2 - M1^2 = sum over i, sum over j < i of w_i w_j (m_i - m_j)^2        (the background contributes nothing)

in float64, unshifted (the cancellation a float32 kernel has to avoid is 1e-16 of M2 A here), and it records the tie margins
depth_ref.tie_mask reads.
"""
import numpy as np
import torch

from oracle.autograd_ref import _project, _quat_to_mat, _sh_color, camera_matrices
from depth_ref import intrinsics, tie_mask  # noqa: F401  (re-exported for the tests)
from normal_ref import splat_normals


def splat_depth(z, kind="z", near=0.2, far=1000.0):
    """The per-splat depth m of brush_hip_distortion.h: z itself ("z") or 2DGS's far (z - near) / ((far - near) z) ("ndc")."""
    if kind == "z":
        return z
    assert kind == "ndc" and 0.0 < near < far
    return far * (z - near) / ((far - near) * z)


def pair_sum(weights, m):
    """The literal definition: sum over i, sum over j < i of w_i w_j (m_i - m_j)^2 per pixel, from render(keep_terms=True)'s terms."""
    k = weights.shape[0]
    out = torch.zeros(weights.shape[1:], dtype=weights.dtype)
    for i in range(k):
        for j in range(i):
            out = out + weights[i] * weights[j] * (m[i] - m[j]) ** 2
    return out


def render(transforms, sh, raw_opac, cam, w, h, bg=(0.0, 0.0, 0.0), intrinsics=None, mip=False, smooth=False, comp_is_constant=True, kind="z", near=0.2,
           far=1000.0, keep_terms=False, window=None):
    """Arguments as autograd_ref.render, then the distortion kind.  Returns dict(img [h,w,4], dist [h,w], A, M1, M2 [h,w], normal
    [h,w,3] (accumulated), acc [h,w] (depth), expected [h,w], alpha [h,w], tie_alpha, tie_t, tie_median [h,w], n_terms [h,w], m [N],
    z [N], keep [N]) and, keep_terms=True, terms = (weights [K,h,w], m [K]) of the K splats the loop visited, in the blend's order
    (detached).  window = (x0, y0, x1, y1): every map covers the pixels x0 <= x < x1, y0 <= y < y1 of the frame only (a large frame's
    gradient test pays for the pixels its cotangents touch)."""
    dt = torch.float64
    r_np, t_np, (fx, fy, cx, cy), lim = camera_matrices(cam["pos"], cam["rot_xyzw"], cam["fov_x"], cam["fov_y"], cam["center_uv"], w, h)
    model = cam.get("model", "pinhole")
    if model != "pinhole":
        fx, fy, cx, cy = intrinsics["fx"], intrinsics["fy"], intrinsics["cx"], intrinsics["cy"]
        lim = intrinsics["lim"]
    rc, tc = torch.tensor(r_np, dtype=dt), torch.tensor(t_np, dtype=dt)
    mean, quat, log_s = transforms[:, 0:3], transforms[:, 3:7], transforms[:, 7:10]
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
        ju, jv = _project(model, cam["dist"], q, fx, fy, cx, cy)
        ru = torch.autograd.grad(ju.sum(), q, create_graph=True)[0]
        rv = torch.autograd.grad(jv.sum(), q, create_graph=True)[0]
        jac = torch.stack([ru, rv], -2)
    cov2 = jac @ cov_c @ jac.transpose(1, 2)
    blur = 0.1 if mip else 0.3
    det_raw = torch.clamp(cov2[:, 0, 0] * cov2[:, 1, 1] - cov2[:, 0, 1] * cov2[:, 0, 1], min=0.0)
    a, b, c = cov2[:, 0, 0] + blur, cov2[:, 0, 1], cov2[:, 1, 1] + blur
    det = a * c - b * b
    c00, c01, c11 = c / det, -b / det, a / det
    mx, my = _project(model, cam.get("dist", ()), mean_c, fx, fy, cx, cy)
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
    nrm, axis, facing = splat_normals(transforms, rc, tc)
    mz = splat_depth(zc, kind, near, far)

    x0, y0, x1, y1 = (0, 0, w, h) if window is None else window
    py, px = torch.meshgrid(torch.arange(y0, y1, dtype=dt) + 0.5, torch.arange(x0, x1, dtype=dt) + 0.5, indexing="ij")
    h, w = y1 - y0, x1 - x0   # (from here on the shape of the maps: the window's)
    T = torch.ones((h, w), dtype=dt)
    rgb = torch.zeros((h, w, 3), dtype=dt)
    acc = torch.zeros((h, w), dtype=dt)
    nacc = torch.zeros((h, w, 3), dtype=dt)
    m1 = torch.zeros((h, w), dtype=dt)
    m2 = torch.zeros((h, w), dtype=dt)
    n_terms = torch.zeros((h, w), dtype=torch.int64)
    term_w, term_m = [], []
    done = torch.zeros((h, w), dtype=torch.bool)
    inf = torch.full((h, w), float("inf"), dtype=dt)
    tie_alpha, tie_t, tie_median = inf.clone(), inf.clone(), inf.clone()
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
            tie_median = torch.where(contrib, torch.minimum(tie_median, (next_t - 0.5).abs()), tie_median)
            n_terms = n_terms + contrib.to(torch.int64)
        vis = torch.where(contrib, alpha * T, torch.zeros_like(T))
        rgb = rgb + vis[..., None] * color[i]
        acc = acc + vis * zc[i]
        nacc = nacc + vis[..., None] * nrm[i]
        m1 = m1 + vis * mz[i]
        m2 = m2 + vis * mz[i] * mz[i]
        if keep_terms:
            term_w.append(vis.detach())
            term_m.append(mz[i].detach())
        T = torch.where(contrib, next_t, T)
        done = done | sat
    bgt = torch.tensor(bg, dtype=dt)
    img = torch.cat([rgb + T[..., None] * bgt, (1.0 - T)[..., None]], dim=-1)
    A = 1.0 - T
    expected = torch.where(A > 0, acc / torch.where(A > 0, A, torch.ones_like(A)), torch.zeros_like(A))
    out = dict(img=img, dist=A * m2 - m1 * m1, A=A, M1=m1, M2=m2, normal=nacc, acc=acc, expected=expected, alpha=A, tie_alpha=tie_alpha,
               tie_t=tie_t, tie_median=tie_median, n_terms=n_terms, m=mz, keep=keep, z=zc)
    if keep_terms:
        out["terms"] = (torch.stack(term_w) if term_w else torch.zeros((0, h, w), dtype=dt), torch.stack(term_m) if term_m else torch.zeros((0,), dtype=dt))
    return out


def gradients(scene, cam, w, h, v_distortion, kind="z", near=0.2, far=1000.0, v_output=None, v_depth=None, depth_mode="expected", v_normal=None,
              bg=(0.0, 0.0, 0.0), intrinsics=None, mip=False, smooth=False, window=None):
    """d( <v_distortion, dist> [+ <v_output, img>] [+ <v_depth, depth(depth_mode)>] [+ <v_normal, accumulated normals>] ) /
    d(transforms, sh, raw_opac) by autograd; numpy float64 in and out.  With a window the cotangents have the window's shape."""
    tr = torch.tensor(np.asarray(scene["transforms"], np.float64), requires_grad=True)
    sh = torch.tensor(np.asarray(scene["sh"], np.float64), requires_grad=True)
    op = torch.tensor(np.asarray(scene["raw_opac"], np.float64), requires_grad=True)
    out = render(tr, sh, op, cam, w, h, bg, intrinsics, mip, smooth, kind=kind, near=near, far=far, window=window)
    loss = (out["dist"] * torch.tensor(np.asarray(v_distortion, np.float64))).sum()
    if v_output is not None:
        loss = loss + (out["img"] * torch.tensor(np.asarray(v_output, np.float64))).sum()
    if v_depth is not None:
        loss = loss + (out["acc" if depth_mode == "accumulated" else "expected"] * torch.tensor(np.asarray(v_depth, np.float64))).sum()
    if v_normal is not None:
        loss = loss + (out["normal"] * torch.tensor(np.asarray(v_normal, np.float64))).sum()
    loss.backward()
    z = lambda g, x: np.zeros(tuple(x.shape)) if g is None else g.numpy()
    out = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}
    return out, z(tr.grad, tr), z(sh.grad, sh), z(op.grad, op)
