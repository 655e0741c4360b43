"""Float64 restatement of include/brush_hip_normal_loss.h — TEST INFRASTRUCTURE ONLY: the normal-consistency loss
between an accumulated normal map N [H,W,3] and the normals u of a depth map [H,W] (tests/normal_ref.py::depth_to_normal: the same
stencil, the same validity rule), weighted by a constant alpha A [H,W]:

    l(p)     = A (1 - N . u)          at a valid pixel (its stencil is valid), 0 elsewhere
    loss     = c * sum of l,  c = f32(weight / (H W));  count = the valid pixels
    v_normal = -c A u                 at a valid pixel, 0 elsewhere
    v_depth  = d loss / d depth: the chain of v_u = -c A N through depth_to_normal, written out as the gather the header describes
               (every pixel collects from the at most four valid stencils that read it) — tests/test_normal_loss_ref.py pins it
               against torch.autograd.
"""
import numpy as np
import torch

import normal_ref


def constant(weight, pixels):
    return float(np.float32(np.float64(np.float32(weight)) / np.float64(pixels)))


def loss_terms(normal, depth, alpha, fx, fy, cx, cy, weight=1.0):
    """Differentiable float64 torch tensors in, -> (loss scalar tensor, valid [H,W] bool tensor, u [H,W,3])."""
    h, w = depth.shape
    u, valid = normal_ref.depth_to_normal(depth, fx, fy, cx, cy)
    l = alpha.detach() * (1.0 - (normal * u).sum(-1))
    l = torch.where(valid, l, torch.zeros_like(l))
    return constant(weight, h * w) * l.sum(), valid, u


def _stencil_grad(d, v, fx, fy, cx, cy, x, y, which):
    """d <v, c / |c|> / d (the depth of neighbour `which` of the stencil at (x, y)), float64 numpy: 0 left, 1 right, 2 up, 3 down."""
    kx, kxl, kxr = (x + 0.5 - cx) / fx, (x - 0.5 - cx) / fx, (x + 1.5 - cx) / fx
    ky, kyu, kyd = (y + 0.5 - cy) / fy, (y - 0.5 - cy) / fy, (y + 1.5 - cy) / fy
    dl, dr, du, dd = d[y, x - 1], d[y, x + 1], d[y - 1, x], d[y + 1, x]
    gx = np.array([kxr * dr - kxl * dl, ky * (dr - dl), dr - dl])
    gy = np.array([kx * (dd - du), kyd * dd - kyu * du, dd - du])
    c = np.cross(gy, gx)
    ln = np.linalg.norm(c)
    if ln == 0.0:
        return 0.0
    u = c / ln
    vc = (v - u * v.dot(u)) / ln
    if which < 2:
        vg = np.cross(vc, gy)   # c = gy x gx: v_gx = vc x gy
        return -vg.dot([kxl, ky, 1.0]) if which == 0 else vg.dot([kxr, ky, 1.0])
    vg = np.cross(gx, vc)       # v_gy = gx x vc
    return -vg.dot([kx, kyu, 1.0]) if which == 2 else vg.dot([kx, kyd, 1.0])


def value_and_grad(normal, depth, alpha, fx, fy, cx, cy, weight=1.0):
    """numpy in (any float type; evaluated in float64) -> dict(loss float, count int, valid bool [H,W], u [H,W,3], v_normal [H,W,3],
    v_depth [H,W]).  weight <= 0 or NaN: everything 0."""
    n = np.asarray(normal, np.float64)
    d = np.asarray(depth, np.float64)
    a = np.asarray(alpha, np.float64)
    h, w = d.shape
    out = dict(loss=0.0, count=0, valid=np.zeros((h, w), bool), u=np.zeros((h, w, 3)), v_normal=np.zeros((h, w, 3)), v_depth=np.zeros((h, w)))
    if not np.float32(weight) > 0:
        return out
    c = constant(weight, h * w)
    u_t, valid_t = normal_ref.depth_to_normal(torch.tensor(d), fx, fy, cx, cy)
    u, valid = u_t.numpy(), valid_t.numpy()
    l = np.where(valid, a * (1.0 - (n * u).sum(-1)), 0.0)
    out.update(loss=c * float(l.sum()), count=int(valid.sum()), valid=valid, u=u, v_normal=np.where(valid[..., None], -c * a[..., None] * u, 0.0))
    v_u = -c * a[..., None] * n
    g = out["v_depth"]
    for y in range(h):
        for x in range(w):
            # pixel (x, y) is the right neighbour of the stencil at x-1, the left one of x+1, the lower one of y-1, the upper one of y+1
            for (qx, qy, which) in ((x - 1, y, 1), (x + 1, y, 0), (x, y - 1, 3), (x, y + 1, 2)):
                if 0 <= qx < w and 0 <= qy < h and valid[qy, qx]:
                    g[y, x] += _stencil_grad(d, v_u[qy, qx], fx, fy, cx, cy, qx, qy, which)
    return out
