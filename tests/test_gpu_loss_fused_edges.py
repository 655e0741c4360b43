"""The fused loss pair (brush_amd/csrc/loss_fused.hip) at the shapes where its tile mapping and row paths change, and the
kernels' literal Gaussian taps against their definition."""
import ctypes
import ctypes.util
import os
import re

import numpy as np
import pytest
import torch

import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (h, w):
#   33 x 18   two tile columns -> row-major tile mapping; w % 4 != 0 -> pass B's narrow-row path; one row past a 32-row block
#   32 x 256  exact multiples; 16 tile columns -> banded mapping, bands 2 tile columns wide
#   70 x 260  17 tile columns -> bands 3 wide, bands 6 and 7 empty; wide rows; five tile rows -> the last block's lower half
#             lies outside the image
SHAPES = [(33, 18), (32, 256), (70, 260)]


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("bg,mask,alpha_w", [(None, False, 0.0), ((0.3, 0.5, 0.2), False, 0.1), (None, True, 0.0)])
def test_fused_loss_edge_shapes_match_oracle(dev, oracle_lib, h, w, bg, mask, alpha_w):
    """image_loss_value_and_grad against the oracle's stand-alone forward / backward, with the tolerances of
    test_gpu_loss_optim.py::test_fused_loss_matches_oracle_and_standalone: 2e-6 x max(1, |loss|) and 2e-6 x max|g|."""
    import brush_amd as ba
    rng = np.random.default_rng(h * 7 + w)
    gt = util.packed_from_rgba(rng.integers(0, 256, (h, w, 4), dtype=np.uint32))
    img = rng.uniform(-0.1, 1.1, (h, w, 4)).astype(np.float32)
    ch = 4 if alpha_w > 0 else 3
    gt_t = torch.from_numpy(gt.view(np.int32)).to(dev)
    loss, v_out = ba.image_loss_value_and_grad(torch.from_numpy(img).to(dev), gt_t, 0.8, -0.2, composite_bg=bg, mask=mask, alpha_weight=alpha_w)
    pc = np.ascontiguousarray(img[..., :ch].transpose(2, 0, 1))
    rlm = oracle_lib.image_loss_forward(pc, gt, 0.8, -0.2, bg=bg, mask=mask).astype(np.float64)
    ref_loss = rlm[:3].mean() + (alpha_w * rlm[3].mean() if ch == 4 else 0.0)
    dl = np.empty((ch, h, w), np.float32)
    dl[:3] = 1.0 / (h * w * 3)
    if ch == 4:
        dl[3] = alpha_w / (h * w)
    rg = oracle_lib.image_loss_backward(pc, gt, dl, 0.8, -0.2, bg=bg, mask=mask).transpose(1, 2, 0)
    g = v_out.cpu().numpy()
    loss_err = abs(float(loss.item()) - ref_loss)
    grad_err = np.abs(g[..., :ch] - rg).max()
    print("%dx%d loss err %.3g (bound %.3g)  grad err %.3g (bound %.3g)" % (h, w, loss_err, 2e-6 * max(1.0, abs(ref_loss)), grad_err, 2e-6 * max(np.abs(rg).max(), 1e-12)))
    assert g.shape == (h, w, 4) and np.isfinite(g).all()
    assert loss_err <= 2e-6 * max(1.0, abs(ref_loss))
    assert grad_err <= 2e-6 * max(np.abs(rg).max(), 1e-12)
    if ch == 3:
        assert not g[..., 3].any()


def test_literal_taps_are_the_hosts_gauss_taps():
    """The kernels' tap literals equal what gauss_taps() computes on the host (libm expf, float sum, float divide), bit for bit
    — the comparison the launcher makes before every first launch, here without a device."""
    src = open(os.path.join(ROOT, "brush_amd", "csrc", "loss_fused.hip")).read()
    lit = {int(i): v for i, v in re.findall(r"#define BH_TAP_(\d) (0x[0-9a-f.]+p[-+]?\d+)f", src)}
    assert sorted(lit) == [0, 1, 2, 3, 4, 5]
    table = np.array([float.fromhex(lit[min(i, 10 - i)]) for i in range(11)], np.float32)
    assert [float(t).hex() for t in table] == [float.fromhex(lit[min(i, 10 - i)]).hex() for i in range(11)]   # exactly floats
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.expf.restype = ctypes.c_float
    libm.expf.argtypes = [ctypes.c_float]
    f = np.float32
    sigma = f(1.5)
    w = np.empty(11, np.float32)
    total = f(0.0)
    for i in range(11):
        x = f(i) - f(5.0)
        w[i] = f(libm.expf(float(-x * x / (f(2.0) * sigma * sigma))))
        total = f(total + w[i])
    w = (w / total).astype(np.float32)
    assert w.tobytes() == table.tobytes(), [(float(a).hex(), float(b).hex()) for a, b in zip(w, table) if a != b]
