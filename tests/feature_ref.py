"""Float64 restatements for the feature maps (include/brush_hip_features.h) — TEST INFRASTRUCTURE ONLY.

render(): oracle/autograd_ref.py::render's loop, built as tests/depth_ref.py is (the set-up in front of the loop and the loop's
alpha / cut-off / saturation rule are autograd_ref.render's, statement for statement; tests/test_feature_ref.py pins the RGBA of
the two against each other, exactly), which beside the colour folds, per pixel and with the blend's own weight w_i = T_i alpha_i,

  F = sum of w_i f_i            (f_i = the caller's feature row of splat i, any channel count; the background contributes 0)

and records the same tie margins as depth_ref.render, so depth_ref.tie_mask(out, "accumulated") applies to its result.

l1_loss() / cross_entropy_loss(): float64 numpy restatements of the two fused losses, value and gradient.
"""
import numpy as np
import torch

from oracle.autograd_ref import _project, _quat_to_mat, _sh_color, camera_matrices


def render(transforms, sh, raw_opac, features, cam, w, h, bg=(0.0, 0.0, 0.0), intrinsics=None, mip=False, smooth=False, comp_is_constant=True,
           map_grad=True):
    """Arguments as autograd_ref.render, plus features [N,C].  Returns dict(img [h,w,4], feat [h,w,C], alpha [h,w], tie_alpha, tie_t
    [h,w]: the smallest |alpha - 1/255| and |next_T - 1e-4| the pixel met while live, n_terms [h,w]: contributing splats, vis
    [N,h,w]: the weight w_i of every splat at every pixel (0 where it does not contribute), carrying the graph).
    map_grad=False: feat is folded from detached values (no graph: a wide map of a long list would hold C floats per pixel and
    splat); gradients then go through vis, <v, F> = sum of vis_i (v . f_i) (gradients() below)."""
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
    feat = torch.zeros((h, w, features.shape[1]), dtype=dt)
    done = torch.zeros((h, w), dtype=torch.bool)
    inf = torch.full((h, w), float("inf"), dtype=dt)
    tie_alpha, tie_t = inf.clone(), inf.clone()
    n_terms = torch.zeros((h, w), dtype=torch.int64)
    vis_of = [torch.zeros((h, w), dtype=dt)] * transforms.shape[0]
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
            n_terms = n_terms + contrib.to(torch.int64)
        vis = torch.where(contrib, alpha * T, torch.zeros_like(T))
        rgb = rgb + vis[..., None] * color[i]
        if map_grad:
            feat = feat + vis[..., None] * features[i]
        else:
            with torch.no_grad():
                feat = feat + vis.detach()[..., None] * features[i].detach()
        vis_of[i] = vis
        T = torch.where(contrib, next_t, T)
        done = done | sat
    bgt = torch.tensor(bg, dtype=dt)
    img = torch.cat([rgb + T[..., None] * bgt, (1.0 - T)[..., None]], dim=-1)
    return dict(img=img, feat=feat, alpha=1.0 - T, tie_alpha=tie_alpha, tie_t=tie_t, n_terms=n_terms, z=zc, keep=keep,
                vis=torch.stack(vis_of))


def gradients(scene, features, cam, w, h, v_map, v_output=None, bg=(0.0, 0.0, 0.0), intrinsics=None, mip=False, smooth=False):
    """d( <v_map, F> [+ <v_output, img>] ) / d(transforms, sh, raw_opac, features) by autograd; numpy float64 in and out."""
    tr = torch.tensor(np.asarray(scene["transforms"], np.float64), requires_grad=True)
    sh = torch.tensor(np.asarray(scene["sh"], np.float64), requires_grad=True)
    op = torch.tensor(np.asarray(scene["raw_opac"], np.float64), requires_grad=True)
    ft = torch.tensor(np.asarray(features, np.float64), requires_grad=True)
    out = render(tr, sh, op, ft, cam, w, h, bg, intrinsics, mip, smooth, map_grad=False)
    loss = (out["vis"] * torch.einsum("hwc,nc->nhw", torch.tensor(np.asarray(v_map, np.float64)), ft)).sum()
    if v_output is not None:
        loss = loss + (out["img"] * torch.tensor(np.asarray(v_output, np.float64))).sum()
    loss.backward()
    z = lambda g, x: np.zeros(tuple(x.shape)) if g is None else g.numpy()
    return out, z(tr.grad, tr), z(sh.grad, sh), z(op.grad, op), z(ft.grad, ft)


def l1_loss(fmap, target, weight=1.0):
    """-> (loss, valid pixels, v_map): l = sum_c |F_c - t_c| over the pixels whose C target values are all finite, times
    weight / (H W C); sign(0) = 0.  d = F - t is formed in float32, as the kernel forms it (its sign decides the gradient);
    everything behind it is float64."""
    f32, t32 = np.asarray(fmap, np.float32), np.asarray(target, np.float32)
    h, w, c = f32.shape
    valid = np.isfinite(t32).all(axis=-1)
    with np.errstate(invalid="ignore"):
        d = np.where(valid[..., None], (f32 - t32).astype(np.float64), 0.0)
    cw = float(weight) / (h * w * c)
    return cw * np.abs(d).sum(), int(valid.sum()), cw * np.sign(d)


def cross_entropy_loss(fmap, labels, weight=1.0):
    """-> (loss, valid pixels, v_map): l = logsumexp_c(F) - F_label over the pixels with label < C, times weight / (H W);
    v_map = (softmax(F) - onehot) weight / (H W).  Float64 on the float32 logits, the maximum subtracted."""
    f = np.asarray(fmap, np.float32).astype(np.float64)
    lab = np.asarray(labels).astype(np.int64)
    h, w, c = f.shape
    valid = lab < c
    safe = np.where(valid, lab, 0)
    m = f.max(axis=-1, keepdims=True)
    e = np.exp(f - m)
    s = e.sum(axis=-1, keepdims=True)
    picked = np.take_along_axis(f, safe[..., None], axis=-1)[..., 0]
    l = np.log(s[..., 0]) + (m[..., 0] - picked)
    onehot = np.zeros_like(f)
    np.put_along_axis(onehot, safe[..., None], 1.0, axis=-1)
    cw = float(weight) / (h * w)
    v = np.where(valid[..., None], cw * (e / s - onehot), 0.0)
    return cw * np.where(valid, l, 0.0).sum(), int(valid.sum()), v
