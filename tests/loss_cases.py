"""Image families for the image loss (brush_amd/csrc/loss.hip, loss_fused.hip), and the two yardsticks every test of them shares:
oracle/autograd_loss_ref.py (float64, torch autograd) and the oracle's float32 restatement.  Plain numpy, seeded.

Uniform noise is the best-conditioned input SSIM can get; on images like the ones training sees, E[x^2] - mu^2 cancels against
C2 = 9e-4 and float32 is a hundred times less accurate (tests/test_loss_cases_ref.py measures it).  Each family returns
(img [H,W,4] float32, gt_packed [H,W] uint32 rgba8)."""
import functools

import numpy as np

INV_255 = np.float32(1.0) / np.float32(255.0)

# (h, w): tests/test_gpu_loss_pair_pinned.py says what each one exercises
SHAPES = [(115, 40), (115, 18), (83, 260), (1, 1), (16, 16)]
# (l1 weight, ssim weight): the train step's pair, the SSIM term alone, the L1 term alone
WEIGHTS = [(0.8, -0.2), (0.0, 1.0), (1.0, 0.0)]
# name -> (composite bg, mask, alpha weight)
MODES = {"plain": (None, False, 0.0), "composite": ((0.3, 0.5, 0.2), False, 0.1), "mask": (None, True, 0.0)}


def pack(rgba):
    a = np.asarray(rgba).astype(np.uint32)
    return (a[..., 0] | (a[..., 1] << 8) | (a[..., 2] << 16) | (a[..., 3] << 24)).astype(np.uint32)


def quantise(v):
    return np.clip(np.rint(np.asarray(v, np.float64) * 255.0), 0, 255).astype(np.uint32)


def decode_f32(gt_packed):
    """[H,W] packed -> [H,W,4] float32, as the kernels decode a byte: float32(byte) * float32(1 / 255)."""
    g = np.asarray(gt_packed, np.uint32)
    return np.stack([((g >> (8 * k)) & 0xFF).astype(np.float32) * INV_255 for k in range(4)], -1)


def _grid(h, w):
    return np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")


def _smooth(h, w):
    """[H,W,4] in [0.1, 0.9]: 0.5 + 0.4 sin(x / 7) cos(y / 5) with a phase per channel; the alpha plane in [0.6, 1]."""
    y, x = _grid(h, w)
    v = np.stack([0.5 + 0.4 * np.sin(x / 7.0 + 1.3 * c) * np.cos(y / 5.0 + 0.7 * c) for c in range(3)], -1)
    a = 0.8 + 0.2 * np.cos(x / 11.0) * np.sin(y / 9.0 + 0.4)
    return np.concatenate([v, a[..., None]], -1)


def noise(h, w, seed):
    rng = np.random.default_rng(seed)
    gt = pack(rng.integers(0, 256, (h, w, 4), dtype=np.uint32))
    return rng.uniform(-0.1, 1.1, (h, w, 4)).astype(np.float32), gt


def flat_bright(h, w, seed):
    rng = np.random.default_rng(seed)
    gt = pack(np.broadcast_to(np.array([230, 230, 230, 255], np.uint32), (h, w, 4)))   # 0.9, alpha 1
    img = 0.9 + rng.normal(0.0, 0.003, (h, w, 4))
    img[..., 3] += 0.1
    return img.astype(np.float32), gt


def converged(h, w, seed):
    rng = np.random.default_rng(seed)
    gt = pack(quantise(_smooth(h, w)))
    return (decode_f32(gt).astype(np.float64) + rng.normal(0.0, 0.002, (h, w, 4))).astype(np.float32), gt


def ramp(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = _grid(h, w)
    t = x / max(w - 1, 1) if w > 1 else np.full((h, w), 0.5)
    s = y / max(h - 1, 1) if h > 1 else np.full((h, w), 0.5)
    v = np.stack([t, 1.0 - t, 0.25 + 0.5 * t, 0.5 + 0.5 * s], -1)
    return (v + rng.normal(0.0, 0.01, (h, w, 4))).astype(np.float32), pack(quantise(v))


def disc(h, w):
    """The object of black_bg: [H,W] bool, a disc round the image's centre (never empty)."""
    y, x = _grid(h, w)
    r = max(0.35 * min(h, w), 0.75)
    return (y + 0.5 - h / 2.0) ** 2 + (x + 0.5 - w / 2.0) ** 2 <= r * r


def black_bg(h, w, seed):
    """NeRF-synthetic: GT alpha 0 and colour 0 outside a disc, alpha 1 and random colour inside; the render is exactly 0 outside."""
    rng = np.random.default_rng(seed)
    inside = disc(h, w)
    rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint32)
    rgba[..., 3] = 255
    rgba[~inside] = 0
    gt = pack(rgba)
    img = decode_f32(gt).astype(np.float64) + rng.normal(0.0, 0.05, (h, w, 4))
    img[~inside] = 0.0
    return img.astype(np.float32), gt


def inverted(h, w, seed):
    rng = np.random.default_rng(seed)
    gt = pack(quantise(_smooth(h, w)))
    d = decode_f32(gt)
    img = np.float32(1.0) - d
    img[..., 3] = (d[..., 3].astype(np.float64) + rng.normal(0.0, 0.01, (h, w))).astype(np.float32)
    return img, gt


def identical_patch(h, w):
    """The rows x columns of `identical` where the render is NOT its photo (never empty)."""
    return slice(h // 4, h // 4 + max(1, h // 4)), slice(w // 4, w // 4 + max(1, w // 4))


def identical(h, w, seed, patch=True):
    """The render bit-equal to the float32 value the kernels decode from the photo, alpha included: every such pixel is an exact tie
    of the L1 sign.  The photo saturates at white and at black.  With `patch`, one rectangle (identical_patch) differs by N(0, 0.02):
    an image that is a tie everywhere has no gradient to measure an error against."""
    rng = np.random.default_rng(seed)
    v = _smooth(h, w)
    v[..., :3] = np.clip(0.5 + 1.5 * (v[..., :3] - 0.5), 0.0, 1.0)
    gt = pack(quantise(v))
    img = decode_f32(gt)
    if patch:
        ys, xs = identical_patch(h, w)
        img[ys, xs] = (img[ys, xs].astype(np.float64) + rng.normal(0.0, 0.02, img[ys, xs].shape)).astype(np.float32)
    return img, gt


FAMILIES = {"noise": noise, "flat_bright": flat_bright, "converged": converged, "ramp": ramp, "black_bg": black_bg, "inverted": inverted,
            "identical": identical}


@functools.lru_cache(maxsize=None)
def case(family, h, w, seed=1):
    img, gt = FAMILIES[family](h, w, seed)
    assert img.shape == (h, w, 4) and img.dtype == np.float32 and gt.shape == (h, w) and gt.dtype == np.uint32
    img.setflags(write=False)
    gt.setflags(write=False)
    return img, gt


# ---------------------------------------------------------------------------------------------------------------------------
# the yardsticks
# ---------------------------------------------------------------------------------------------------------------------------
def gt_eff_f32(gt, bg):
    """[H,W,4] float32: the colour the loss compares with (composited over bg when given, unfused float32), and the GT alpha."""
    d = decode_f32(gt)
    if bg is not None:
        d[..., :3] = d[..., :3] + (np.float32(1.0) - d[..., 3:4]) * np.asarray(bg, np.float32)
    return d


def ambiguous(img, gt, bg, ch):
    """[H,W] bool: pixels where float32 and float64 disagree about the sign of (render - photo) in one of the first `ch` channels —
    exact ties of the float32 values, whose photo is k / 255 in float64 and k * (1 / 255) in float32.  The L1 term's gradient there
    is a convention, not an error."""
    d32 = np.sign(img - gt_eff_f32(gt, bg))
    g64 = np.stack([((gt >> (8 * k)) & 0xFF).astype(np.float64) / 255.0 for k in range(4)], -1)
    if bg is not None:
        g64[..., :3] = g64[..., :3] + (1.0 - g64[..., 3:4]) * np.asarray(bg, np.float64)
    d64 = np.sign(img.astype(np.float64) - g64)
    return (d32 != d64)[..., :ch].any(-1)


def _dl(h, w, ch, alpha_w):
    dl = np.empty((ch, h, w), np.float32)
    dl[:3] = 1.0 / (h * w * 3)
    if ch == 4:
        dl[3] = alpha_w / (h * w)
    return dl


def _loss_of_map(m, ch, alpha_w):
    m = np.asarray(m, np.float64)
    return float(m[:3].mean() + (alpha_w * m[3].mean() if ch == 4 else 0.0))


@functools.lru_cache(maxsize=None)
def yardsticks(family, h, w, weights, mode, seed=1):
    """One case through both references -> dict: ch, dl; map64 / grad64 / loss64 (float64, autograd); map32 / grad32 / loss32 (the
    oracle's float32 restatement); excluded [H,W] (ambiguous pixels).  Maps are [ch,H,W], gradients [H,W,ch]; the loss is
    mean(colour planes) + alpha weight * mean(alpha plane), its gradient what image_loss_value_and_grad returns."""
    from oracle import autograd_loss_ref, bo
    img, gt = case(family, h, w, seed)
    (l1_w, ssim_w), (bg, mask, alpha_w) = weights, MODES[mode]
    ch = 4 if alpha_w > 0 else 3
    pc = np.ascontiguousarray(img[..., :ch].transpose(2, 0, 1))
    dl = _dl(h, w, ch, alpha_w)
    m64, g64 = autograd_loss_ref.backward(pc, gt, dl, l1_w, ssim_w, bg, mask)
    m32 = bo.image_loss_forward(pc, gt, l1_w, ssim_w, bg=bg, mask=mask)
    g32 = bo.image_loss_backward(pc, gt, dl, l1_w, ssim_w, bg=bg, mask=mask)
    out = dict(ch=ch, dl=dl, map64=m64, grad64=g64.transpose(1, 2, 0), loss64=_loss_of_map(m64, ch, alpha_w), map32=m32, grad32=g32.transpose(1, 2, 0),
               loss32=_loss_of_map(m32, ch, alpha_w), excluded=ambiguous(img, gt, bg, ch))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def grad_err(g, y, where=None):
    """max |g - float64 gradient| over the pixels of `where` (default: all) that are not excluded; 0.0 if there are none."""
    keep = ~y["excluded"] if where is None else (where & ~y["excluded"])
    if not keep.any():
        return 0.0
    return float(np.abs(np.asarray(g, np.float64)[..., :y["ch"]] - y["grad64"])[keep].max())


def regions(h, w):
    """name -> [H,W] bool, a partition: the 5-px image border (zero padding applies); pixels within 5 px of a seam between the fused
    kernels' 16-column x 32-row blocks; the interior."""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    border = (y < 5) | (y >= h - 5) | (x < 5) | (x >= w - 5)

    def near_seam(i, n, pitch):
        hit = np.zeros(i.shape, bool)
        for s in range(pitch, n, pitch):   # the seam lies between pixels s - 1 and s
            hit |= (i >= s - 5) & (i < s + 5)
        return hit
    seam = (near_seam(x, w, 16) | near_seam(y, h, 32)) & ~border
    return {"border": border, "seam": seam, "interior": ~border & ~seam}
