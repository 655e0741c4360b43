"""numpy restatement of the image half of LoadImage::load (brush-dataset/src/load_image.rs:60-131) and view_to_packed_data
(scene.rs:97-136): the contract include/brush_hip_image.h and brush_amd/csrc/image.hip are held to, bit for bit.

resize() is image::imageops::resize of the image crate 0.25 as the reference builds it.  That crate's source is not part of this
repository, so this file is the contract:
  * a vertical pass (h -> nh) into an f32 intermediate, then a horizontal pass (w -> nw) back to u8; the same size is a copy;
  * per pass, src -> dst, all f32: ratio = src / dst, sratio = max(ratio, 1), src_support = support * sratio (Lanczos3: 3,
    Triangle: 1); output o: c = (o + 0.5) * ratio, left = clamp(floor(c - src_support), 0, src - 1),
    right = clamp(ceil(c + src_support), left + 1, src); tap i in [left, right) weighs k((i - (c - 0.5)) / sratio), then every
    weight is divided by their sum (accumulated in tap order);
  * lanczos3(x) = |x| < 3 ? sinc(x) sinc(x / 3) : 0 with sinc(t) = t == 0 ? 1 : sin(a) / a, a = t * PI_f32, sin being the C
    library's sinf (what Rust's f32::sin lowers to on Linux; np.sin's float32 result may differ by an ulp);
    triangle(x) = |x| < 1 ? 1 - |x| : 0;
  * every channel t = 0, then t = t + v_i * w_i per tap in order (a multiply and an add, no FMA); the vertical pass stores t
    unrounded, the horizontal pass round_half_away(clamp(t, 0, 255)).  Alpha is a channel like any other.
"""
import ctypes

import numpy as np

F = np.float32
PI = F(np.pi)   # std::f32::consts::PI
LANCZOS3, TRIANGLE = "lanczos3", "triangle"

_libm = ctypes.CDLL("libm.so.6")
_libm.sinf.restype = ctypes.c_float
_libm.sinf.argtypes = [ctypes.c_float]


def sinf(x):
    return F(_libm.sinf(float(F(x))))


def _sinc(t):
    t = F(t)
    if t == 0:
        return F(1.0)
    a = F(t * PI)
    return F(sinf(a) / a)


def kernel(filter, x):
    x = F(x)
    if filter == TRIANGLE:
        return F(F(1.0) - abs(x)) if abs(x) < F(1.0) else F(0.0)
    return F(_sinc(x) * _sinc(F(x / F(3.0)))) if abs(x) < F(3.0) else F(0.0)


def pass_weights(src, dst, filter):
    """-> [(left, f32 weights)] of every output of one pass."""
    ratio = F(F(src) / F(dst))
    sratio = ratio if ratio >= F(1.0) else F(1.0)
    support = F(F(1.0 if filter == TRIANGLE else 3.0) * sratio)
    out = []
    for o in range(dst):
        c = F(F(F(o) + F(0.5)) * ratio)
        left = int(np.floor(F(c - support)))
        left = min(max(left, 0), src - 1)
        right = int(np.ceil(F(c + support)))
        right = min(max(right, left + 1), src)
        cc = F(c - F(0.5))
        ws, s = [], F(0.0)
        for i in range(left, right):
            k = kernel(filter, F(F(F(i) - cc) / sratio))
            ws.append(k)
            s = F(s + k)
        out.append((left, np.array([F(k / s) for k in ws], dtype=F)))
    return out


def _pass(x, dst, filter):
    """Resample axis 0 of the f32 array x to dst entries (taps beyond an output's count weigh +0: t + 0 is t)."""
    src = x.shape[0]
    tab = pass_weights(src, dst, filter)
    stride = max(len(w) for _, w in tab)
    lefts = np.array([l for l, _ in tab], dtype=np.int64)
    W = np.zeros((dst, stride), dtype=F)
    for o, (_, w) in enumerate(tab):
        W[o, :len(w)] = w
    t = np.zeros((dst,) + x.shape[1:], dtype=F)
    bshape = (dst,) + (1,) * (x.ndim - 1)
    for j in range(stride):
        idx = np.minimum(lefts + j, src - 1)
        t = t + x[idx] * W[:, j].reshape(bshape)
    return t


def round_half_away_u8(t):
    t = np.clip(t, F(0.0), F(255.0)).astype(np.float64)   # exact widening; + 0.5 is then exact too
    return np.floor(t + 0.5).astype(np.uint8)


def resize(img, nw, nh, filter=LANCZOS3):
    """image::imageops::resize(img, nw, nh, filter): img uint8 [H,W] or [H,W,C] -> uint8 [nh,nw(,C)]."""
    img = np.asarray(img, dtype=np.uint8)
    h, w = img.shape[:2]
    if (nw, nh) == (w, h):
        return img.copy()
    x = img.reshape(h, w, -1).astype(F)
    v = _pass(x, nh, filter)                                 # [nh, w, C] f32, unrounded
    hz = _pass(np.ascontiguousarray(v.transpose(1, 0, 2)), nw, filter).transpose(1, 0, 2)
    return round_half_away_u8(hz).reshape((nh, nw) + img.shape[2:])


def output_size(w, h, max_resolution=1920, scale=1.0):
    """LoadImage::output_scale and the size load() resizes to (max_resolution 0 / None: no cap)."""
    s = F(scale)
    if max_resolution:
        cap = F(F(max_resolution) / F(max(w, h, max_resolution)))
        s = F(cap * s)
    s = min(s, F(1.0))
    if s < F(1.0):
        return int(max(F(F(w) * s), F(1.0))), int(max(F(F(h) * s), F(1.0)))
    return w, h


def merge_mask(img, mask, invert=False):
    """load_image.rs:69-112: into_rgba8, the one-channel mask Triangle-resized to the image if its size differs, alpha = mask
    (or 255 - mask)."""
    img = np.asarray(img, dtype=np.uint8)
    h, w = img.shape[:2]
    mask = np.asarray(mask, dtype=np.uint8)
    if mask.shape != (h, w):
        mask = resize(mask, w, h, TRIANGLE)
    a = (255 - mask).astype(np.uint8) if invert else mask
    return np.concatenate([img[:, :, :3], a[:, :, None]], axis=2)


def pack(img, premultiply):
    """view_to_packed_data: uint8 [H,W,3|4] -> (uint32 [H,W] r | g << 8 | b << 16 | a << 24, has_alpha)."""
    img = np.asarray(img, dtype=np.uint8)
    has_alpha = img.shape[2] == 4
    rgb = img[:, :, :3].astype(np.uint32)
    a = img[:, :, 3].astype(np.uint32) if has_alpha else np.full(img.shape[:2], 255, np.uint32)
    if has_alpha and premultiply:
        rgb = (rgb * a[:, :, None] + 127) // 255
    return rgb[:, :, 0] | (rgb[:, :, 1] << 8) | (rgb[:, :, 2] << 16) | (a << 24), has_alpha


def load_view(img, mask=None, invert=False, max_resolution=1920, scale=1.0, premultiply=None):
    """LoadImage::load of a decoded view + view_to_packed_data -> (uint32 [nh, nw], has_alpha)."""
    img = np.asarray(img, dtype=np.uint8)
    if premultiply is None:
        premultiply = mask is None
    if mask is not None:
        img = merge_mask(img, mask, invert)
    h, w = img.shape[:2]
    nw, nh = output_size(w, h, max_resolution, scale)
    if (nw, nh) != (w, h):
        img = resize(img, nw, nh, LANCZOS3)
    return pack(img, premultiply)
