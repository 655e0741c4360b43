"""Float64 torch restatement of oracle/autograd_ref.py::render's loop that also accumulates normals, and of the normals of a depth
map — TEST INFRASTRUCTURE ONLY (include/brush_hip_normal.h).

Built like tests/depth_ref.py: the set-up in front of the loop and the loop's alpha / cut-off / saturation rule are
autograd_ref.render's, statement for statement (tests/test_normal_ref.py pins the RGBA of the two against each other, exactly); its
helpers are imported unchanged.  Beside the colour the loop folds, per pixel and with the blend's own weight w_i = T_i alpha_i:

  N     = sum of w_i n_i      (n_i = the splat's camera-space normal; the background contributes 0)
  D     = sum of w_i z_i      (as depth_ref)
  A     = 1 - T_final
  unit  = N / |N|, 0 where |N| == 0

and it records the tie margins depth_ref.tie_mask reads.
"""
import numpy as np
import torch

from oracle.autograd_ref import _project, _quat_to_mat, _sh_color, camera_matrices
from depth_ref import intrinsics, tie_mask  # noqa: F401  (re-exported for the tests)


def splat_normals(transforms, rc, tc):
    """The splat normal of brush_hip_normal.h.  transforms [N,10] f64 (mean, quaternion wxyz, log-scale), rc [3,3] / tc [3] the view
    rotation and translation.  -> (n [N,3] oriented camera-space normals, k [N] the axis, facing [N] = n_c . mean_c / |mean_c| before
    the flip).  k and the sign are piecewise constant: the gradient reaches the quaternion only."""
    mean, quat, log_s = transforms[:, 0:3], transforms[:, 3:7], transforms[:, 7:10]
    ls = log_s.detach()
    first = (ls[:, 0] <= ls[:, 1]) & (ls[:, 0] <= ls[:, 2])
    k = torch.where(first, 0, torch.where(ls[:, 1] <= ls[:, 2], 1, 2)).to(torch.int64)   # the smallest; the lowest index on a tie
    q = quat / quat.norm(dim=1, keepdim=True)
    r = _quat_to_mat(q)
    n_w = torch.gather(r, 2, k[:, None, None].expand(-1, 3, 1))[:, :, 0]
    n_c = n_w @ rc.T
    mean_c = (mean @ rc.T + tc).detach()
    d = (n_c.detach() * mean_c).sum(1)
    sign = torch.where(d > 0, -torch.ones_like(d), torch.ones_like(d))
    n = n_c * sign[:, None]
    return n, k, d / mean_c.norm(dim=1)


def camera_rt(cam, w, h):
    r_np, t_np, _, _ = camera_matrices(cam["pos"], cam["rot_xyzw"], cam["fov_x"], cam["fov_y"], cam["center_uv"], w, h)
    return torch.tensor(r_np, dtype=torch.float64), torch.tensor(t_np, dtype=torch.float64)


def render(transforms, sh, raw_opac, cam, w, h, bg=(0.0, 0.0, 0.0), intrinsics=None, mip=False, smooth=False, comp_is_constant=True):
    """Arguments as autograd_ref.render.  Returns dict(img [h,w,4], normal [h,w,3] (accumulated), unit [h,w,3], acc [h,w] (depth),
    expected [h,w], alpha [h,w], tie_alpha, tie_t, tie_median [h,w], splat_normals [N,3], axis [N], facing [N], keep [N])."""
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

    py, px = torch.meshgrid(torch.arange(h, dtype=dt) + 0.5, torch.arange(w, dtype=dt) + 0.5, indexing="ij")
    T = torch.ones((h, w), dtype=dt)
    rgb = torch.zeros((h, w, 3), dtype=dt)
    acc = torch.zeros((h, w), dtype=dt)
    nacc = torch.zeros((h, w, 3), dtype=dt)
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
        vis = torch.where(contrib, alpha * T, torch.zeros_like(T))
        rgb = rgb + vis[..., None] * color[i]
        acc = acc + vis * zc[i]
        nacc = nacc + vis[..., None] * nrm[i]
        T = torch.where(contrib, next_t, T)
        done = done | sat
    bgt = torch.tensor(bg, dtype=dt)
    img = torch.cat([rgb + T[..., None] * bgt, (1.0 - T)[..., None]], dim=-1)
    A = 1.0 - T
    expected = torch.where(A > 0, acc / torch.where(A > 0, A, torch.ones_like(A)), torch.zeros_like(A))
    return dict(img=img, normal=nacc, unit=unit(nacc), acc=acc, expected=expected, alpha=A, tie_alpha=tie_alpha, tie_t=tie_t,
                tie_median=tie_median, splat_normals=nrm, axis=axis, facing=facing, keep=keep, z=zc)


def unit(n):
    """n / |n| along the last axis, 0 where |n| == 0 (with a zero gradient there)."""
    sq = (n * n).sum(-1, keepdim=True)
    has = sq > 0
    length = torch.sqrt(torch.where(has, sq, torch.ones_like(sq)))
    return torch.where(has, n / length, torch.zeros_like(n))


def depth_to_normal(depth, fx, fy, cx, cy):
    """brush_hip_normal.h's normals of a z-depth map [h,w] (f64 tensor) of a pinhole camera -> (normals [h,w,3], valid [h,w])."""
    h, w = depth.shape
    dt = depth.dtype
    d0 = depth.detach()
    good = torch.isfinite(d0) & (d0 > 0)
    valid = torch.zeros((h, w), dtype=torch.bool)
    out = torch.zeros((h, w, 3), dtype=dt)
    if h < 3 or w < 3:
        return out, valid
    valid[1:-1, 1:-1] = good[1:-1, 1:-1] & good[1:-1, :-2] & good[1:-1, 2:] & good[:-2, 1:-1] & good[2:, 1:-1]
    d = torch.where(good, depth, torch.ones_like(depth))   # (no NaN or inf reaches the arithmetic, nor its gradient)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dt), torch.arange(w, dtype=dt), indexing="ij")
    p = torch.stack([(xs + 0.5 - cx) / fx * d, (ys + 0.5 - cy) / fy * d, d], -1)
    gx = p[1:-1, 2:] - p[1:-1, :-2]
    gy = p[2:, 1:-1] - p[:-2, 1:-1]
    c = torch.linalg.cross(gy, gx, dim=-1)
    inner = torch.where(valid[1:-1, 1:-1][..., None], unit(c), torch.zeros_like(c))
    out = torch.nn.functional.pad(inner.permute(2, 0, 1), (1, 1, 1, 1)).permute(1, 2, 0)
    return out, valid


def gradients(scene, cam, w, h, v_normal, mode, v_output=None, v_depth=None, depth_mode="expected", bg=(0.0, 0.0, 0.0), intrinsics=None,
              mip=False, smooth=False, loss_fn=None):
    """d( <v_normal, normal(mode)> [+ <v_output, img>] [+ <v_depth, depth(depth_mode)>] ) / d(transforms, sh, raw_opac) by autograd —
    or of loss_fn(out), a scalar of render()'s outputs; numpy float64 in and out.  out["v_tr_normal_path"] [N,10] is the part of the
    transforms gradient that arrives through the splat normals themselves (the gradient with Vn forced to 0 is the total minus it)."""
    tr = torch.tensor(np.asarray(scene["transforms"], np.float64), requires_grad=True)
    sh = torch.tensor(np.asarray(scene["sh"], np.float64), requires_grad=True)
    op = torch.tensor(np.asarray(scene["raw_opac"], np.float64), requires_grad=True)
    out = render(tr, sh, op, cam, w, h, bg, intrinsics, mip, smooth)
    out["splat_normals"].retain_grad()
    if loss_fn is not None:
        loss = loss_fn(out)
    else:
        loss = (out["normal" if mode == "accumulated" else "unit"] * torch.tensor(np.asarray(v_normal, np.float64))).sum()
        if v_output is not None:
            loss = loss + (out["img"] * torch.tensor(np.asarray(v_output, np.float64))).sum()
        if v_depth is not None:
            loss = loss + (out["acc" if depth_mode == "accumulated" else "expected"] * torch.tensor(np.asarray(v_depth, np.float64))).sum()
    loss.backward()
    vn = out["splat_normals"].grad
    tr2 = tr.detach().clone().requires_grad_(True)
    rc, tc = camera_rt(cam, w, h)
    (splat_normals(tr2, rc, tc)[0] * (torch.zeros_like(tr2[:, :3]) if vn is None else vn)).sum().backward()
    z = lambda g, x: np.zeros(tuple(x.shape)) if g is None else g.numpy()
    out = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}
    out["v_tr_normal_path"] = z(tr2.grad, tr2)
    return out, z(tr.grad, tr), z(sh.grad, sh), z(op.grad, op)
