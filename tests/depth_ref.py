"""Float64 torch restatement of oracle/autograd_ref.py::render's loop that also accumulates depth — TEST INFRASTRUCTURE ONLY.

The set-up in front of the loop (projection, conic, opacity, colour, the keep mask, the depth order) and the loop's alpha / cut-off /
saturation rule are autograd_ref.render's, statement for statement (tests/test_depth_ref.py pins the RGBA of the two against each
other, exactly); its helpers are imported unchanged.  Beside the colour the loop folds, per pixel and with the blend's own weight
w_i = T_i alpha_i:

  D      = sum of w_i z_i              (z_i = camera-space z of the splat's mean; the background contributes 0)
  A      = 1 - T_final                 (the image's alpha)
  median = z of the contributing splat at which T first becomes <= 0.5 (0 where that never happens)

and it records, per pixel, how close the float64 run came to each threshold decision (include/brush_hip_depth.h): a
float32 renderer may decide a pixel the other way only where one of these margins is tiny.
"""
import numpy as np
import torch

from oracle.autograd_ref import _project, _quat_to_mat, _sh_color, camera_matrices


def render(transforms, sh, raw_opac, cam, w, h, bg=(0.0, 0.0, 0.0), intrinsics=None, mip=False, smooth=False, comp_is_constant=True):
    """Arguments as autograd_ref.render.  Returns dict(img [h,w,4], acc [h,w], alpha [h,w], expected [h,w], median [h,w],
    tie_alpha, tie_t, tie_median [h,w]: the smallest |alpha - 1/255|, |next_T - 1e-4| and |T - 0.5| the pixel met while live,
    n_terms [h,w]: contributing splats)."""
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

    py, px = torch.meshgrid(torch.arange(h, dtype=dt) + 0.5, torch.arange(w, dtype=dt) + 0.5, indexing="ij")
    T = torch.ones((h, w), dtype=dt)
    rgb = torch.zeros((h, w, 3), dtype=dt)
    acc = torch.zeros((h, w), dtype=dt)
    median = torch.zeros((h, w), dtype=dt)
    done = torch.zeros((h, w), dtype=torch.bool)
    inf = torch.full((h, w), float("inf"), dtype=dt)
    tie_alpha, tie_t, tie_median = inf.clone(), inf.clone(), inf.clone()
    n_terms = torch.zeros((h, w), dtype=torch.int64)
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
            hit = contrib & (T > 0.5) & (next_t <= 0.5)
            median = torch.where(hit, zc[i].detach(), median)
            n_terms = n_terms + contrib.to(torch.int64)
        vis = torch.where(contrib, alpha * T, torch.zeros_like(T))
        rgb = rgb + vis[..., None] * color[i]
        acc = acc + vis * zc[i]
        T = torch.where(contrib, next_t, T)
        done = done | sat
    bgt = torch.tensor(bg, dtype=dt)
    img = torch.cat([rgb + T[..., None] * bgt, (1.0 - T)[..., None]], dim=-1)
    A = 1.0 - T
    expected = torch.where(A > 0, acc / torch.where(A > 0, A, torch.ones_like(A)), torch.zeros_like(A))
    return dict(img=img, acc=acc, alpha=A, expected=expected, median=median, tie_alpha=tie_alpha, tie_t=tie_t, tie_median=tie_median,
                n_terms=n_terms, z=zc, keep=keep)


def tie_mask(out, mode):
    """Pixels a float32 renderer may decide differently (brush_hip_depth.h tests): some alpha within 1e-6 of 1/255, some next_T
    within 1e-6 of 1e-4 or, for the median, some T within 1e-5 of 0.5."""
    m = (out["tie_alpha"] <= 1e-6) | (out["tie_t"] <= 1e-6)
    if mode == "median":
        m = m | (out["tie_median"] <= 1e-5)
    return m


def gradients(scene, cam, w, h, v_depth, mode, v_output=None, bg=(0.0, 0.0, 0.0), intrinsics=None, mip=False, smooth=False):
    """d( <v_depth, depth(mode)> [+ <v_output, img>] ) / d(transforms, sh, raw_opac) by autograd; numpy float64 in and out."""
    tr = torch.tensor(np.asarray(scene["transforms"], np.float64), requires_grad=True)
    sh = torch.tensor(np.asarray(scene["sh"], np.float64), requires_grad=True)
    op = torch.tensor(np.asarray(scene["raw_opac"], np.float64), requires_grad=True)
    out = render(tr, sh, op, cam, w, h, bg, intrinsics, mip, smooth)
    loss = (out["acc" if mode == "accumulated" else "expected"] * torch.tensor(np.asarray(v_depth, np.float64))).sum()
    if v_output is not None:
        loss = loss + (out["img"] * torch.tensor(np.asarray(v_output, np.float64))).sum()
    loss.backward()
    z = lambda g, x: np.zeros(tuple(x.shape)) if g is None else g.numpy()
    return out, z(tr.grad, tr), z(sh.grad, sh), z(op.grad, op)


def intrinsics(camp, w, h):
    """What render() wants as `intrinsics`, from the oracle's camera set-up (as tests/test_oracle_autograd_pin.py takes it)."""
    from oracle import bo
    cam = bo.camera(img_w=w, img_h=h, **camp)
    return dict(fx=float(cam.fx), fy=float(cam.fy), cx=float(cam.cx), cy=float(cam.cy), half_max_render_fov=float(cam.half_max_render_fov),
                lim=(float(cam.lim_pos_x), float(cam.lim_pos_y), float(cam.lim_neg_x), float(cam.lim_neg_y)))
