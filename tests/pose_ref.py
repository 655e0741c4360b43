"""Float64 torch restatement of oracle/autograd_ref.py::render with the camera pose as a leaf — TEST INFRASTRUCTURE ONLY.

The renderer is autograd_ref.render's, statement for statement (tests/test_pose_ref.py pins the two images against each other), its
helpers imported unchanged, with three differences that leave the image as it is (include/brush_hip_pose.h):

  * W [3,3] and t [3] (world-to-camera) are tensors, by default camera_matrices' values;
  * the SH view direction is taken from p = -W^T t instead of the camera's `pos` (the same point);
  * every splat gets its OWN copy W_i, t_i of the pose, so that one backward returns the per-splat contributions to the twelve
    entries: their sum is v_viewmat, the sum of their absolute values the L1 mass S_k the tolerances are stated in.

The layout of the twelve is BhCamera.vm's: column-major 3x4, entry (row i, column j) of W at [3 j + i], t at [9..11].
"""
import numpy as np
import torch

from oracle.autograd_ref import _project, _quat_to_mat, _sh_color, camera_matrices


def pose_of(cam, w, h):
    """(W [3,3], t [3]) float64 numpy of a camera dict (camera_matrices)."""
    r, t, _, _ = camera_matrices(cam["pos"], cam["rot_xyzw"], cam["fov_x"], cam["fov_y"], cam["center_uv"], w, h)
    return r, t


def pack(w_mat, t):
    """W, t -> the twelve in BhCamera.vm's layout."""
    return np.concatenate([np.asarray(w_mat, np.float64).T.reshape(-1), np.asarray(t, np.float64).reshape(-1)])


def unpack(vm):
    vm = np.asarray(vm, np.float64)
    return vm[:9].reshape(3, 3).T.copy(), vm[9:12].copy()


def render(transforms, sh, raw_opac, cam, w, h, bg=(0.0, 0.0, 0.0), intrinsics=None, mip=False, smooth=False, comp_is_constant=True,
           pose=None):
    """Arguments as autograd_ref.render; pose = (W [3,3], t [3]) float64 tensors or None (the camera's own).  Returns dict(img
    [h,w,4], W_n [N,3,3], t_n [N,3]: the per-splat copies of the pose (leaves of their own when W / t require a gradient),
    tie_alpha, tie_t [h,w]: how close the pixel came to the 1/255 and the 1e-4 decisions while live)."""
    dt = torch.float64
    r_np, t_np, (fx, fy, cx, cy), lim = camera_matrices(cam["pos"], cam["rot_xyzw"], cam["fov_x"], cam["fov_y"], cam["center_uv"], w, h)
    model = cam.get("model", "pinhole")
    if model != "pinhole":
        fx, fy, cx, cy = intrinsics["fx"], intrinsics["fy"], intrinsics["cx"], intrinsics["cy"]
        lim = intrinsics["lim"]
    rc, tc = (torch.tensor(r_np, dtype=dt), torch.tensor(t_np, dtype=dt)) if pose is None else pose
    mean, quat, log_s = transforms[:, 0:3], transforms[:, 3:7], transforms[:, 7:10]
    n = transforms.shape[0]
    w_n = rc.unsqueeze(0).repeat(n, 1, 1)
    t_n = tc.unsqueeze(0).repeat(n, 1)
    if w_n.requires_grad:
        w_n.retain_grad()
    if t_n.requires_grad:
        t_n.retain_grad()
    mean_c = torch.einsum("nij,nj->ni", w_n, mean) + t_n
    zc = mean_c[:, 2]
    if model == "pinhole":
        keep = (zc >= 0.01) & (zc <= 1e10)
    else:
        theta = torch.atan2(torch.sqrt(mean_c[:, 0] ** 2 + mean_c[:, 1] ** 2), zc)
        keep = (theta <= intrinsics["half_max_render_fov"]) & (zc <= 1e10)
    q = quat / quat.norm(dim=1, keepdim=True)
    m = _quat_to_mat(q) * torch.exp(log_s)[:, None, :]
    cov_c = w_n @ (m @ m.transpose(1, 2)) @ w_n.transpose(1, 2)
    xz = torch.clamp(mean_c[:, 0] / zc, lim[2], lim[0])
    yz = torch.clamp(mean_c[:, 1] / zc, lim[3], lim[1])
    zero = torch.zeros_like(zc)
    if model == "pinhole":
        jac = torch.stack([torch.stack([fx / zc, zero, -fx / zc * xz], -1), torch.stack([zero, fy / zc, -fy / zc * yz], -1)], -2)
    else:
        q = torch.stack([xz * zc, yz * zc, zc], -1) if model == "rt8" else mean_c
        if not q.requires_grad:
            q = q.detach().requires_grad_(True)
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
    cam_pos = -torch.einsum("nji,nj->ni", w_n, t_n)          # p = -W^T t
    vd = mean - cam_pos
    vd = vd / vd.norm(dim=1, keepdim=True)
    color = torch.clamp(_sh_color(sh, vd) + 0.5, -100.0, 100.0)
    color = torch.clamp(color, min=0.0)
    keep = keep & (alpha0 >= 1.0 / 255.0)

    py, px = torch.meshgrid(torch.arange(h, dtype=dt) + 0.5, torch.arange(w, dtype=dt) + 0.5, indexing="ij")
    T = torch.ones((h, w), dtype=dt)
    rgb = torch.zeros((h, w, 3), dtype=dt)
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
        T = torch.where(contrib, next_t, T)
        done = done | sat
    bgt = torch.tensor(bg, dtype=dt)
    img = torch.cat([rgb + T[..., None] * bgt, (1.0 - T)[..., None]], dim=-1)
    return dict(img=img, W_n=w_n, t_n=t_n, tie_alpha=tie_alpha, tie_t=tie_t)


def tie_mask(out, smooth):
    """Pixels a float32 renderer may decide differently from this one (as tests/depth_ref.py::tie_mask): some next_T within 1e-6 of
    1e-4 and, with the hard cut-off, some alpha within 1e-6 of 1/255 (the smooth cut-off is continuous there)."""
    m = out["tie_t"] <= 1e-6
    if not smooth:
        m = m | (out["tie_alpha"] <= 1e-6)
    return m


def pose_gradients(scene, cam, w, h, v_output, bg=(0.0, 0.0, 0.0), intrinsics=None, mip=False, smooth=False, pose=None, skip_ties=False):
    """Gradients of <v_output, image> with respect to the pose and the splats; numpy float64 in and out.  skip_ties: v_output is
    zeroed on tie_mask's pixels first (the returned `v_output` is what was used, `ties` the mask).
    Returns dict(img, v_viewmat [12], S [12], per_splat [N,12], v_transforms [N,10], v_sh, v_raw_opac, vm [12], ties, v_output)."""
    tr = torch.tensor(np.asarray(scene["transforms"], np.float64), requires_grad=True)
    sh = torch.tensor(np.asarray(scene["sh"], np.float64), requires_grad=True)
    op = torch.tensor(np.asarray(scene["raw_opac"], np.float64), requires_grad=True)
    w_np, t_np = pose_of(cam, w, h) if pose is None else pose
    wm = torch.tensor(np.asarray(w_np, np.float64), requires_grad=True)
    tv = torch.tensor(np.asarray(t_np, np.float64), requires_grad=True)
    out = render(tr, sh, op, cam, w, h, bg, intrinsics, mip, smooth, pose=(wm, tv))
    ties = tie_mask(out, smooth).numpy()
    v = np.array(v_output, np.float64)
    if skip_ties:
        v[ties] = 0.0
    (out["img"] * torch.tensor(v)).sum().backward()
    n = tr.shape[0]
    gw = out["W_n"].grad if out["W_n"].grad is not None else torch.zeros((n, 3, 3), dtype=torch.float64)
    gt = out["t_n"].grad if out["t_n"].grad is not None else torch.zeros((n, 3), dtype=torch.float64)
    per = torch.cat([gw.transpose(1, 2).reshape(n, 9), gt], dim=1).numpy()
    z = lambda g, x: np.zeros(tuple(x.shape)) if g is None else g.numpy()
    return dict(img=out["img"].detach().numpy(), v_viewmat=per.sum(0), S=np.abs(per).sum(0), per_splat=per, v_transforms=z(tr.grad, tr),
                v_sh=z(sh.grad, sh), v_raw_opac=z(op.grad, op), vm=pack(w_np, t_np), ties=ties, v_output=v,
                v_viewmat_leaf=pack(z(wm.grad, wm), z(tv.grad, tv)))


# ---- the tangent space ----------------------------------------------------------------------------------------------------------
def _hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]], np.float64)


def twist(vm, v_viewmat):
    """(v_omega, v_tau): the derivative along W <- exp([omega]x) W, t <- exp([omega]x) t + tau at zero, in f64."""
    w_mat, t = unpack(vm)
    v_w, v_t = unpack(v_viewmat)
    a = v_w @ w_mat.T
    axial = np.array([a[2, 1] - a[1, 2], a[0, 2] - a[2, 0], a[1, 0] - a[0, 1]])
    return np.concatenate([axial + np.cross(t, v_t), v_t])


def twist_mass(vm, S):
    """An upper bound of the L1 mass of the six twist entries, from the L1 masses S of the twelve (|.| through the linear map)."""
    w_mat, t = unpack(vm)
    s_w, s_t = unpack(S)
    a = s_w @ np.abs(w_mat).T
    axial = np.array([a[2, 1] + a[1, 2], a[0, 2] + a[2, 0], a[1, 0] + a[0, 1]])
    at = np.abs(t)
    cross = np.array([at[1] * s_t[2] + at[2] * s_t[1], at[2] * s_t[0] + at[0] * s_t[2], at[0] * s_t[1] + at[1] * s_t[0]])
    return np.concatenate([axial + cross, s_t])


def apply_twist(w_mat, t, tw):
    """exp([omega]x) W, re-orthonormalised (Gram-Schmidt on the columns), and exp([omega]x) t + tau; f64."""
    tw = np.asarray(tw, np.float64)
    r = torch.linalg.matrix_exp(torch.tensor(_hat(tw[:3]))).numpy()
    m = r @ np.asarray(w_mat, np.float64)
    c0 = m[:, 0] / np.linalg.norm(m[:, 0])
    c1 = m[:, 1] - (c0 @ m[:, 1]) * c0
    c1 = c1 / np.linalg.norm(c1)
    return np.stack([c0, c1, np.cross(c0, c1)], axis=1), r @ np.asarray(t, np.float64) + tw[3:]


def omega_from_splat_grads(vm, transforms, v_transforms):
    """Identity (c) at SH degree 0: v_omega = W sum_i c_i + t x (W sum_i v_mean_i), with
    c_i = mean_i x v_mean_i + (w v_qv - v_qw qv + qv x v_qv) / 2 for the un-normalised quaternion (w, qv) and its gradient."""
    w_mat, t = unpack(vm)
    tr, g = np.asarray(transforms, np.float64), np.asarray(v_transforms, np.float64)
    mean, v_mean = tr[:, 0:3], g[:, 0:3]
    qw, qv, gw, gv = tr[:, 3:4], tr[:, 4:7], g[:, 3:4], g[:, 4:7]
    c = np.cross(mean, v_mean) + 0.5 * (qw * gv - gw * qv + np.cross(qv, gv))
    return w_mat @ c.sum(0) + np.cross(t, w_mat @ v_mean.sum(0))


def omega_mass_from_splat_grads(vm, transforms, v_transforms):
    """L1 mass of the summands of omega_from_splat_grads, per entry."""
    w_mat, t = unpack(vm)
    tr, g = np.asarray(transforms, np.float64), np.asarray(v_transforms, np.float64)
    mean, v_mean = tr[:, 0:3], g[:, 0:3]
    qw, qv, gw, gv = tr[:, 3:4], tr[:, 4:7], g[:, 3:4], g[:, 4:7]
    c = np.cross(mean, v_mean) + 0.5 * (qw * gv - gw * qv + np.cross(qv, gv))
    per = c @ w_mat.T + np.cross(t[None, :], v_mean @ w_mat.T)
    return np.abs(per).sum(0)


def rigid_map(scene, cam_pose, g_rot, b):
    """The world map mean -> G mean + b, R_i -> G R_i, W -> W G^T, t -> t - W G^T b: (scene', (W', t'))."""
    w_mat, t = cam_pose
    tr = np.asarray(scene["transforms"], np.float64).copy()
    tr[:, 0:3] = tr[:, 0:3] @ g_rot.T + b
    # q_G (x) q_i, q_G from the rotation matrix by the trace formulas
    qg = _quat_of(g_rot)
    tr[:, 3:7] = _qmul(qg[None, :], tr[:, 3:7])
    sc = dict(transforms=tr, sh=np.asarray(scene["sh"], np.float64), raw_opac=np.asarray(scene["raw_opac"], np.float64))
    w2 = w_mat @ g_rot.T
    return sc, (w2, t - w2 @ b)


def _quat_of(r):
    w = 0.5 * np.sqrt(max(1.0 + r[0, 0] + r[1, 1] + r[2, 2], 0.0))
    return np.array([w, (r[2, 1] - r[1, 2]) / (4 * w), (r[0, 2] - r[2, 0]) / (4 * w), (r[1, 0] - r[0, 1]) / (4 * w)])


def _qmul(a, b):
    aw, av, bw, bv = a[:, 0:1], a[:, 1:4], b[:, 0:1], b[:, 1:4]
    return np.concatenate([aw * bw - (av * bv).sum(1, keepdims=True), aw * bv + bw * av + np.cross(av, bv)], axis=1)


def intrinsics(camp, w, h):
    """What render() wants as `intrinsics`, from the oracle's camera set-up (as tests/depth_ref.py takes it)."""
    from oracle import bo
    cam = bo.camera(img_w=w, img_h=h, **camp)
    return dict(fx=float(cam.fx), fy=float(cam.fy), cx=float(cam.cx), cy=float(cam.cy), half_max_render_fov=float(cam.half_max_render_fov),
                lim=(float(cam.lim_pos_x), float(cam.lim_pos_y), float(cam.lim_neg_x), float(cam.lim_neg_y)))
