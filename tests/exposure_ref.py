"""Float64 restatement of per-view exposure compensation (include/brush_hip_exposure.h) in numpy: the affine colour
transform of a view on an [H,W,4] image, its backward with the per-entry L1 masses the GPU tests scale their bounds by, plain Adam
on the twelve parameters, and the recovery loop (a least-squares fit of a known transform) whose settings the GPU test takes.
tests/test_exposure_ref.py pins the backward to torch autograd."""
import numpy as np

IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)
# the transform the recovery tests fit: gains 0.7 / 1.0 / 1.25, one cross term, offsets +-0.05
M_STAR = np.array([0.7, 0.0, 0.0, 0.05, 0.0, 1.0, 0.1, 0.0, 0.0, 0.0, 1.25, -0.05], np.float64)
# ... with Adam at this rate for this many updates (chosen on the CPU: recovery() on the oracle's render)
RECOVERY_LR, RECOVERY_ITERS = 0.02, 400


def _split(m):
    m = np.asarray(m, np.float64).reshape(3, 4)
    return m[:, :3], m[:, 3]


def apply(m, x):
    """y [H,W,4] f64: y_r = sum_c m[4r+c] x_c + m[4r+3], alpha passes through."""
    a, b = _split(m)
    x = np.asarray(x, np.float64)
    y = x.copy()
    y[..., :3] = x[..., :3] @ a.T + b
    return y


def apply_mass(m, x):
    """[H,W,3]: sum_c |m_rc| |x_c| + |m_r3|, the magnitude the apply kernel's roundings scale with."""
    a, b = _split(m)
    return np.abs(np.asarray(x, np.float64)[..., :3]) @ np.abs(a).T + np.abs(b)


def backward(m, x, v):
    """For a cotangent v [H,W,4] on y: dict(v_img [H,W,4], v_m [12], S [12] the L1 mass sum_p |term| of every entry of v_m,
    v_mass [H,W,3] = sum_r |m_rc| |v_r|)."""
    a, _ = _split(m)
    x, v = np.asarray(x, np.float64), np.asarray(v, np.float64)
    v_img = v.copy()
    v_img[..., :3] = v[..., :3] @ a
    xr, vr = x[..., :3].reshape(-1, 3), v[..., :3].reshape(-1, 3)
    v_m, s = np.zeros((3, 4)), np.zeros((3, 4))
    v_m[:, :3] = vr.T @ xr
    v_m[:, 3] = vr.sum(0)
    s[:, :3] = np.abs(vr).T @ np.abs(xr)
    s[:, 3] = np.abs(vr).sum(0)
    return dict(v_img=v_img, v_m=v_m.reshape(12), S=s.reshape(12), v_mass=np.abs(v[..., :3]) @ np.abs(a))


def adam_step(param, m1, m2, t, g, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """One plain Adam step in f64, the library's operations in its order: -> (param, m1, m2, t)."""
    param, m1, m2, g = (np.asarray(v, np.float64) for v in (param, m1, m2, g))
    t = int(t) + 1
    m1 = beta1 * m1 + (1.0 - beta1) * g
    m2 = beta2 * m2 + (1.0 - beta2) * g * g
    ah = m1 / (1.0 - beta1 ** float(t))
    bh = m2 / (1.0 - beta2 ** float(t))
    return param - lr * ah / (np.sqrt(bh) + eps), m1, m2, t


def mse_cotangent(y, target):
    """d/dy of mean((y - target)^2 over rgb): [H,W,4], alpha 0."""
    y, target = np.asarray(y, np.float64), np.asarray(target, np.float64)
    v = np.zeros_like(y)
    v[..., :3] = 2.0 * (y[..., :3] - target[..., :3]) / y[..., :3].size
    return v


def recovery(x, m_star=M_STAR, lr=RECOVERY_LR, iters=RECOVERY_ITERS, f32_params=False):
    """Fits y* = M* x from the identity by Adam on the mean squared error: -> (max |m - M*| at the start, at the end).
    f32_params: the parameters are rounded to f32 after every step, as the device table holds them."""
    target = apply(m_star, x)
    m, m1, m2, t = IDENTITY.copy(), np.zeros(12), np.zeros(12), 0
    start = float(np.abs(m - m_star).max())
    for _ in range(iters):
        g = backward(m, x, mse_cotangent(apply(m, x), target))["v_m"]
        m, m1, m2, t = adam_step(m, m1, m2, t, g, lr)
        if f32_params:
            m = m.astype(np.float32).astype(np.float64)
    return start, float(np.abs(m - m_star).max())


def darker_view_loop(bo, trainer_cls, cfg, scene, cams, gts, background, steps, lr, median_scene_scale=3.0):
    """The CPU run of tests/test_gpu_exposure_train.py's two-view loop: the oracle's train step (oracle/trainer.py) with the
    exposure term of this file around its loss — step s trains view s % 2 with row s % 2 — -> the [2,12] table after `steps`
    steps.  `scene` is updated in place, as the oracle's trainer does."""
    rows = [dict(m=IDENTITY.copy(), m1=np.zeros(12), m2=np.zeros(12), t=0) for _ in cams]
    tr = trainer_cls(bo, cfg, median_scene_scale)
    real_fwd, real_bwd = bo.image_loss_forward, bo.image_loss_backward
    for s in range(steps):
        row = rows[s % 2]
        m32 = row["m"].astype(np.float32).astype(np.float64)   # the device table holds f32

        def fwd(pred, gt, *a, **k):
            x = pred.transpose(1, 2, 0).astype(np.float64)
            y = x @ m32.reshape(3, 4)[:, :3].T + m32.reshape(3, 4)[:, 3]
            fwd.x, fwd.y = x, np.ascontiguousarray(y.transpose(2, 0, 1).astype(np.float32))
            return real_fwd(fwd.y, gt, *a, **k)

        def bwd(pred, gt, dl, *a, **k):
            g = real_bwd(fwd.y, gt, dl, *a, **k)   # v' on the exposed image, [3,h,w]
            h, w = g.shape[1:]
            x4, v4 = np.zeros((h, w, 4)), np.zeros((h, w, 4))
            x4[..., :3], v4[..., :3] = fwd.x, g.transpose(1, 2, 0)
            r = backward(m32, x4, v4)
            row["m"], row["m1"], row["m2"], row["t"] = adam_step(m32, row["m1"], row["m2"], row["t"], r["v_m"], lr)
            return np.ascontiguousarray(r["v_img"][..., :3].transpose(2, 0, 1).astype(np.float32))
        bo.image_loss_forward, bo.image_loss_backward = fwd, bwd
        try:
            tr.step(scene, cams[s % 2], gts[s % 2], background)
        finally:
            bo.image_loss_forward, bo.image_loss_backward = real_fwd, real_bwd
    return np.stack([r["m"] for r in rows])
