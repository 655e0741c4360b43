"""The reference's LpipsModel::lpips (crates/lpips/src/lib.rs) restated in torch on the CPU, in f64 or f32, with autograd: the
oracle tests/test_gpu_lpips.py holds bh_lpips_forward / bh_lpips_value_and_grad to.

Inputs are what the library takes: img_hwc4 [H,W,4] f32 (alpha ignored) and gt_packed [H,W] rgba8 (uint32), decoded like
unpack_gt_rgb (brush-loss/src/lib.rs:662-696) in f32.  Parameters are the canonical flat vector of include/brush_hip_lpips.h.
The model's constants (shift, scale, 1e-10) are the f32 values the kernels use, widened when dtype is f64."""
import numpy as np
import torch
import torch.nn.functional as F

CONVS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
         (512, 512), (512, 512), (512, 512))
BLOCK_CONVS = (2, 2, 3, 3, 3)
HEADS = (64, 128, 256, 512, 512)
SHIFT = np.array([-0.030, -0.088, -0.188], np.float32)
SCALE = np.array([0.458, 0.448, 0.450], np.float32)
PARAM_COUNT = 14716160


def unpack_params(flat):
    flat = np.asarray(flat, np.float32).reshape(-1)
    assert flat.size == PARAM_COUNT
    convs, o = [], 0
    for ci, co in CONVS:
        w = flat[o:o + co * ci * 9].reshape(co, ci, 3, 3)
        o += co * ci * 9
        b = flat[o:o + co]
        o += co
        convs.append((w, b))
    heads = []
    for c in HEADS:
        heads.append(flat[o:o + c])
        o += c
    assert o == flat.size
    return convs, heads


def pack_rgba8(r, g, b, a=None):
    r, g, b = (np.asarray(v, np.uint32) for v in (r, g, b))
    a = np.full_like(r, 255) if a is None else np.asarray(a, np.uint32)
    return (r | (g << 8) | (b << 16) | (a << 24)).astype(np.uint32)


def gt_rgb(gt_packed, composite_bg=None):
    """unpack_gt_rgb in f32: byte * (1/255) [+ (1 - a * (1/255)) * bg]."""
    g = np.asarray(gt_packed, np.uint32)
    inv = np.float32(1.0 / 255.0)
    out = np.stack([((g >> (8 * c)) & 0xFF).astype(np.float32) * inv for c in range(3)], -1).astype(np.float32)
    if composite_bg is not None:
        inv_a = (np.float32(1.0) - (g >> 24).astype(np.float32) * inv).astype(np.float32)
        for c in range(3):
            out[..., c] = (out[..., c] + (inv_a * np.float32(composite_bg[c])).astype(np.float32)).astype(np.float32)
    return out


class Model:
    def __init__(self, flat, dtype=torch.float64):
        convs, heads = unpack_params(flat)
        self.dtype = dtype
        self.convs = [(torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype)) for w, b in convs]
        self.heads = [torch.from_numpy(h).to(dtype) for h in heads]
        self.shift = torch.from_numpy(SHIFT).to(dtype).reshape(1, 3, 1, 1)
        self.scale = torch.from_numpy(SCALE).to(dtype).reshape(1, 3, 1, 1)

    def lpips(self, a_hw3, b_hw3):
        """LpipsModel::lpips on two [H,W,3] tensors of self.dtype (0-1 range) -> scalar."""
        xa = (a_hw3.permute(2, 0, 1).unsqueeze(0) * 2.0 - 1.0 - self.shift) / self.scale
        xb = (b_hw3.permute(2, 0, 1).unsqueeze(0) * 2.0 - 1.0 - self.shift) / self.scale
        loss = torch.zeros((), dtype=self.dtype)
        L = 0
        for bi, n in enumerate(BLOCK_CONVS):
            if bi != 0:
                xa = F.max_pool2d(xa, 2, 2)
                xb = F.max_pool2d(xb, 2, 2)
            for _ in range(n):
                w, b = self.convs[L]
                xa = F.relu(F.conv2d(xa, w, b, padding=1))
                xb = F.relu(F.conv2d(xb, w, b, padding=1))
                L += 1
            na = xa / (xa.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            nb = xb / (xb.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            d = (na - nb).pow(2)
            cls = (d * self.heads[bi].reshape(1, -1, 1, 1)).sum(1)
            loss = loss + cls.mean()
        return loss


def value_and_grad(model: Model, img_hwc4, gt_packed, composite_bg=None, grad=True):
    """(LPIPS as float, dLPIPS/dimg rgb [H,W,3] numpy in model.dtype or None)."""
    img = torch.from_numpy(np.ascontiguousarray(np.asarray(img_hwc4, np.float32)[..., :3])).to(model.dtype)
    gt = torch.from_numpy(gt_rgb(gt_packed, composite_bg)).to(model.dtype)
    img.requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        v = model.lpips(img, gt)
        if not grad:
            return float(v), None
        v.backward()
    return float(v.detach()), img.grad.numpy().copy()
