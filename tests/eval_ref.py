"""numpy restatement of eval_stats' metrics (brush-train/src/eval.rs:38-55), the reference tests/test_gpu_eval.py holds
bh_eval_metrics / bh_eval_view to:
    q    = round(rgb * 255) / 255          f32 multiply, round half to even (np.rint), f32 divide, no clamp
    mse  = mean_{H,W,3} image_loss_forward(q, gt, l1 1, ssim 0)^2
    psnr = ln(1 / mse) * 10 / ln 10         f32
    ssim = mean_{H,W,3} image_loss_forward(q, gt, l1 0, ssim 1)
The loss maps come from the CPU oracle (oracle.bo.image_loss_forward); the per-pixel terms are f32 and the means f64 sums rounded
to f32, as the kernel does."""
import numpy as np

LN_10 = np.float32(2.302585092994046)
F255 = np.float32(255.0)


def quantise(rgb):
    """(rgb * 255).round() / 255 in f32, half to even."""
    x = np.asarray(rgb, np.float32)
    k = np.rint((x * F255).astype(np.float32)).astype(np.float32)
    return (k / F255).astype(np.float32)


def psnr_f32(mse):
    """mse.recip().log() * 10.0 / LN_10, every step an f32 operation (+inf for mse == 0)."""
    mse = np.float32(mse)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.float32(np.float32(1.0) / mse)
        ln = np.float32(np.log(r))
        return np.float32(np.float32(ln * np.float32(10.0)) / LN_10)


def pack_rgba8(r, g, b, a=255):
    """[H,W] u32 with r in bits 0-7 ... a in 24-31."""
    r, g, b = (np.asarray(v, np.uint32) for v in (r, g, b))
    return (r | (g << 8) | (b << 16) | (np.uint32(a) << 24)).astype(np.uint32)


def terms(img, gt_packed):
    """Per-pixel f32 terms [3,H,W]: the squared L1 map and the SSIM map of the quantised render."""
    from oracle import bo
    x = np.asarray(img, np.float32)
    q = quantise(x[..., :3])
    chw = np.ascontiguousarray(q.transpose(2, 0, 1))
    l1 = bo.image_loss_forward(chw, gt_packed, 1.0, 0.0)
    ss = bo.image_loss_forward(chw, gt_packed, 0.0, 1.0)
    return (l1 * l1).astype(np.float32), ss.astype(np.float32)


def metrics_from_terms(sq, ss):
    n = sq.size
    mse = np.float32(np.asarray(sq, np.float64).sum() / n)
    ssim = np.float32(np.asarray(ss, np.float64).sum() / n)
    return mse, psnr_f32(mse), ssim


def eval_metrics(img, gt_packed):
    """-> (mse, psnr, ssim) as np.float32 for an [H,W,3|4] f32 render against [H,W] packed rgba8."""
    return metrics_from_terms(*terms(img, gt_packed))


def rgb8(img):
    """The kernel's optional output: clip(rint(x * 255), 0, 255) per channel, alpha 255, packed [H,W] u32."""
    x = np.asarray(img, np.float32)[..., :3]
    with np.errstate(invalid="ignore"):
        k = np.clip(np.rint((x * F255).astype(np.float32)), 0, 255).astype(np.uint32)
    return pack_rgba8(k[..., 0], k[..., 1], k[..., 2])


def tie_values(ks):
    """f32 values x with f32(x * 255) == k + 0.5 exactly (a tie for the rounding), one per k in ks (0 <= k < 255)."""
    out = []
    for k in ks:
        want = np.float32(k + 0.5)
        x = np.float32((k + 0.5) / 255.0)
        for _ in range(64):
            v = np.float32(x * F255)
            if v == want:
                break
            x = np.nextafter(x, np.float32(np.inf) if v < want else np.float32(-np.inf), dtype=np.float32)
        if np.float32(x * F255) != want:
            raise ValueError("no f32 tie for k = %d" % k)
        out.append(x)
    return np.array(out, np.float32)
