"""Held-out evaluation (brush-train/src/eval.rs) without a GPU: the two C-ABI entry points are declared, bound and exported, the
host mirrors exist, argument checks run before the device is touched, and tests/eval_ref.py — the numpy restatement
tests/test_gpu_eval.py holds the kernel to — is checked against what eval_stats promises."""
import math
import os
import re

import numpy as np

import eval_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL_SYMBOLS = ("bh_eval_metrics", "bh_eval_view")


def test_header_ffi_and_library_carry_the_eval_functions():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    src = open(os.path.join(ROOT, "include", "brush_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _ffi.load()
    for name in EVAL_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _ffi.SYMBOLS, name
        assert getattr(lib, name) is not None
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    for name in ("eval_metrics", "eval_stats", "run_eval"):
        assert re.search(r"\b%s\(" % name, hpp), name
    import brush_amd as ba
    for name in ("eval_metrics", "eval_stats", "run_eval", "EvalSample", "EvalResult"):
        assert hasattr(ba, name), name


def test_binding_covers_82_entry_points():
    """The header declares 82 product entry points (80 before, + bh_eval_metrics and bh_eval_view; the test-hook build's own are
    not counted) and the binding carries every one of them."""
    import __graft_entry__ as g
    g.build()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "brush_hip.h")).read(), flags=re.S)
    from brush_amd import _ffi
    declared = set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)) - set(_ffi.TEST_HOOK_SYMBOLS)
    assert len(declared) == 82 and set(_ffi.SYMBOLS) == declared, sorted(declared ^ set(_ffi.SYMBOLS))


def test_eval_entry_points_reject_bad_arguments_without_a_device():
    """A NULL context is refused outright (before the library touches the device)."""
    from brush_amd import _ffi
    lib = _ffi.load()
    assert lib.bh_eval_metrics(None, None, None, 16, 16, None, None) == -1
    assert lib.bh_eval_view(None, None, 0, 0, None, None, None, None, 0, None, None, None) == -1


def test_exact_ties_round_half_to_even():
    ks = np.arange(255)
    x = eval_ref.tie_values(ks)
    assert np.all((x * np.float32(255.0)).astype(np.float32) == (ks + 0.5).astype(np.float32))
    k = np.rint(eval_ref.quantise(x) * np.float32(255.0))
    want = np.where(ks % 2 == 0, ks, ks + 1)
    assert np.array_equal(k, want)
    assert not np.array_equal(k, np.floor(ks + 0.5 + 0.5))   # roundf (half away from zero) would differ at every even k
    # the quantised value is k / 255 by a true f32 divide, not k * (1 / 255)
    q = eval_ref.quantise(x)
    assert np.array_equal(q, (want.astype(np.float32) / np.float32(255.0)).astype(np.float32))


def test_constant_offset_gives_its_psnr():
    rng = np.random.default_rng(3)
    h, w = 37, 53
    for m in (1, 3, 17, 60):
        b = rng.integers(0, 256 - m, size=(h, w, 3)).astype(np.uint32)
        gt = eval_ref.pack_rgba8(b[..., 0], b[..., 1], b[..., 2])
        img = ((b + m).astype(np.float32) / np.float32(255.0)).astype(np.float32)
        mse, psnr, ssim = eval_ref.eval_metrics(img, gt)
        d = m / 255.0
        assert abs(float(psnr) - (-20.0 * math.log10(d))) < 1e-4, (m, float(psnr))
        assert abs(float(mse) - d * d) < 1e-4 * d * d   # (GT bytes are byte * (1/255), the render k / 255)
        assert float(ssim) < 1.0


def test_identical_images_score_ssim_one_and_a_huge_psnr():
    rng = np.random.default_rng(4)
    b = rng.integers(0, 256, size=(40, 29, 3)).astype(np.uint32)
    gt = eval_ref.pack_rgba8(b[..., 0], b[..., 1], b[..., 2])
    img = (b.astype(np.float32) / np.float32(255.0)).astype(np.float32)
    mse, psnr, ssim = eval_ref.eval_metrics(img, gt)
    assert abs(float(ssim) - 1.0) < 1e-6
    # the reference reads GT bytes as byte * (1/255) and the render as k / 255: not always the same f32, so mse is tiny, not 0
    assert float(mse) < 1e-13 and float(psnr) > 100.0
    assert eval_ref.psnr_f32(0.0) == np.float32(np.inf)


def test_values_above_one_are_not_clamped():
    h, w = 20, 24
    gt = eval_ref.pack_rgba8(np.full((h, w), 255), np.full((h, w), 255), np.full((h, w), 255))
    img = np.full((h, w, 4), 1.2, np.float32)
    mse, psnr, _ = eval_ref.eval_metrics(img, gt)
    want = (306.0 / 255.0 - 1.0) ** 2
    assert abs(float(mse) - want) < 1e-6 * want, float(mse)
    # ... whereas the 8-bit copy is clamped
    assert np.all(eval_ref.rgb8(img) == np.uint32(0xFFFFFFFF))
    neg = np.full((2, 2, 4), -0.1, np.float32)
    assert np.all(eval_ref.rgb8(neg) == np.uint32(0xFF000000))


def test_psnr_follows_the_f32_formula():
    for mse in (1e-10, 3.7e-4, 0.01, 0.5, 1.0, 2.0):
        got = eval_ref.psnr_f32(mse)
        assert got.dtype == np.float32
        assert abs(float(got) - 10.0 * math.log10(1.0 / float(np.float32(mse)))) < 1e-5 * max(1.0, abs(float(got)))
