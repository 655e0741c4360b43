"""Restatement of include/brush_hip_depth_loss.h in numpy: the fused depth loss with its gradient, and the held-out depth metrics.

    t = fma(scale, gt, offset) as ONE f32 fma: evaluated exactly in float64 (a product of two f32 is exact there; the sum is rounded
        to float64 first, which changes the f32 result only for sums within 2^-29 of an f32 rounding boundary: none in the tests,
        which check that with `t_is_safe`), then rounded once to f32
    valid: gt finite, t > 0, E > 0
    L1:        l = |E - t|,    v_depth = sign(E - t) c
    disparity: l = |1/E - t|,  v_depth = -(sign(1/E - t) c) / (E E)
    c = f32(weight / (H W)); every difference, quotient and product above is an f32 operation, the sign is the f32 difference's
    loss = f32(c * sum of l in float64), count = valid pixels
    metrics: z_t = t (L1) or f32(1 / t) (disparity); abs-rel, RMSE and the 1.25 inlier share over the valid pixels, per-pixel terms
    and sums in float64.
"""
import numpy as np

L1, DISPARITY = 0, 1
KINDS = {"l1": L1, "disparity": DISPARITY}
f32 = np.float32


def target(gt, scale=1.0, offset=0.0):
    gt = np.asarray(gt, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.float64(f32(scale)) * gt.astype(np.float64) + np.float64(f32(offset))).astype(np.float32)


def t_is_safe(gt, scale=1.0, offset=0.0):
    """The float64 evaluation of the fma rounds to the same f32 as the exact one: the float64 sum is not a tie of two f32."""
    gt = np.asarray(gt, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.float64(f32(scale)) * gt.astype(np.float64) + np.float64(f32(offset))
    x = x[np.isfinite(x)]
    lo = x.astype(np.float32).astype(np.float64)
    up = np.nextafter(lo.astype(np.float32), np.where(x >= lo, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)).astype(np.float64)
    return not np.any(x == 0.5 * (lo + up))


def valid_mask(depth, gt, scale=1.0, offset=0.0):
    depth, gt = np.asarray(depth, np.float32), np.asarray(gt, np.float32)
    t = target(gt, scale, offset)
    with np.errstate(invalid="ignore"):
        return np.isfinite(gt) & (t > 0) & (depth > 0), t


def constant(weight, pixels):
    return f32(np.float64(f32(weight)) / np.float64(pixels))


def loss_and_grad(depth, gt, kind=L1, weight=1.0, scale=1.0, offset=0.0):
    """-> dict(loss f32, count int, v_depth f32 [H,W], sum float64, diff f32 [H,W] (the signed f32 difference, 0 where invalid),
    valid bool [H,W], t f32 [H,W])."""
    kind = KINDS.get(kind, kind)
    depth = np.asarray(depth, np.float32)
    v = np.zeros(depth.shape, np.float32)
    if not f32(weight) > 0:
        return dict(loss=f32(0), count=0, v_depth=v, sum=0.0, diff=v.copy(), valid=np.zeros(depth.shape, bool), t=target(gt, scale, offset))
    valid, t = valid_mask(depth, gt, scale, offset)
    c = constant(weight, depth.size)
    e, tt = depth[valid], t[valid]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        x = e if kind == L1 else (f32(1.0) / e).astype(np.float32)
        d = (x - tt).astype(np.float32)
        s = np.where(d > 0, c, np.where(d < 0, -c, f32(0))).astype(np.float32)
        if kind == L1:
            g = s
        else:
            g = np.where(d != 0, (-s / (e * e).astype(np.float32)).astype(np.float32), f32(0)).astype(np.float32)
    v[valid] = g
    diff = np.zeros(depth.shape, np.float32)
    diff[valid] = d
    total = float(np.sum(np.abs(d.astype(np.float64)), dtype=np.float64))
    return dict(loss=f32(np.float64(c) * total), count=int(valid.sum()), v_depth=v, sum=total, diff=diff, valid=valid, t=t)


def metrics(depth, gt, kind=L1, scale=1.0, offset=0.0):
    """-> float64 [4]: abs-rel, RMSE, inlier share (ratio < 1.25), valid count; the first three 0 without a valid pixel."""
    kind = KINDS.get(kind, kind)
    depth = np.asarray(depth, np.float32)
    valid, t = valid_mask(depth, gt, scale, offset)
    n = int(valid.sum())
    if n == 0:
        return np.zeros(4)
    e = depth[valid].astype(np.float64)
    with np.errstate(over="ignore", divide="ignore"):
        zt = (t[valid] if kind == L1 else (f32(1.0) / t[valid]).astype(np.float32)).astype(np.float64)
        d = e - zt
        ratio = np.maximum(e / zt, zt / e)
        return np.array([np.sum(np.abs(d) / zt) / n, np.sqrt(np.sum(d * d) / n), np.sum(ratio < 1.25) / n, n], np.float64)


def tie_mask(depth, gt, scale=1.0, offset=0.0):
    """Disparity kind: the valid pixels with |1/E - t| <= 2^-20 t, whose sign a last-place difference in 1/E could flip."""
    valid, t = valid_mask(depth, gt, scale, offset)
    depth = np.asarray(depth, np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = np.abs(1.0 / depth.astype(np.float64) - t.astype(np.float64))
        return valid & (d <= 2.0 ** -20 * t.astype(np.float64))
