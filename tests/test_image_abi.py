"""Mask merge and resampling of LoadImage::load (include/brush_hip_image.h) without a GPU: the header declares exactly the binding's
IMAGE_SYMBOLS and the library exports them, the Python and C++ mirrors exist, bh_view_output_size (host only) equals the
restatement of output_scale, and the numpy restatement tests/image_ref.py passes hand-worked cases."""
import os
import re
import subprocess

import numpy as np
import pytest

import image_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def test_header_declares_the_binding_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_image.h"))
    assert declared == set(_ffi.IMAGE_SYMBOLS), declared ^ set(_ffi.IMAGE_SYMBOLS)
    assert '#include "brush_hip.h"' in src
    base, _ = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    assert not (base & declared) and not (set(_ffi.SYMBOLS) & declared)
    assert not (set(_ffi.LPIPS_SYMBOLS) & declared) and not (set(_ffi.COMPRESSED_PLY_SYMBOLS) & declared)
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in _ffi.IMAGE_SYMBOLS:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
    lib = _ffi.load()
    for name in _ffi.IMAGE_SYMBOLS:
        assert getattr(lib, name) is not None
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_image.h"' in hpp
    for name in ("view_output_size(", "resize_u8(", "submit_view("):
        assert name in hpp, name
    import brush_amd as ba
    assert callable(ba.view_output_size) and callable(ba.resize_image) and callable(ba.BatchUploader.submit_view)


def test_view_load_struct_matches_the_header():
    import ctypes as C
    from brush_amd import _ffi
    src = open(os.path.join(ROOT, "include", "brush_hip_image.h")).read()
    body = re.search(r"typedef struct BhViewLoad \{(.*?)\} BhViewLoad;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        m = re.match(r"\s*(\w+)\s+(.*)", decl)
        if m:
            names += [n.strip() for n in m.group(2).split(",")]
    assert names == [f[0] for f in _ffi.BhViewLoad._fields_]
    assert C.sizeof(_ffi.BhViewLoad) == 48


def test_entry_points_reject_bad_arguments():
    import ctypes as C
    from brush_amd import _ffi
    lib = _ffi.load()
    ow, oh = C.c_uint32(), C.c_uint32()
    assert lib.bh_view_output_size(0, 10, 1920, 1.0, C.byref(ow), C.byref(oh)) == -1
    assert lib.bh_view_output_size(10, 10, 1920, 0.0, C.byref(ow), C.byref(oh)) == -1
    assert lib.bh_view_output_size(10, 10, 1920, float("nan"), C.byref(ow), C.byref(oh)) == -1
    assert lib.bh_view_output_size(10, 10, 1920, float("inf"), C.byref(ow), C.byref(oh)) == -1
    assert lib.bh_resize_u8(None, None, 1, 1, 3, None, 1, 1, 0) == -1
    assert lib.bh_uploader_commit_view(None, 0, None) == -1


def _grid():
    sizes = [(4032, 3024), (3024, 4032), (1920, 1080), (1080, 1920), (1920, 1920), (1921, 1), (1, 1921), (3840, 2160), (1, 1), (7, 5),
             (2000, 3), (3, 2000), (640, 480), (12000, 9000), (1919, 1081)]
    for w, h in sizes:
        for mx in (0, 1, 2, 100, 1080, 1919, 1920, 1921, 4096):
            for s in (1.0, 0.5, 0.25, 0.125, 0.3, 0.001, 2.0, 1.0 / 3.0):
                yield w, h, mx, s


def test_view_output_size_equals_the_restatement():
    import brush_amd as ba
    seen_clamp = seen_eq = seen_unchanged = 0
    for w, h, mx, s in _grid():
        got = ba.view_output_size(w, h, mx, s)
        want = ref.output_size(w, h, mx, s)
        assert got == want, (w, h, mx, s, got, want)
        seen_clamp += 1 in got and (w > 1 and h > 1)
        seen_eq += mx == max(w, h)
        seen_unchanged += got == (w, h)
    assert seen_clamp and seen_eq and seen_unchanged
    # hand-worked: the reference's default cap on a 12 MP phone view, portrait, and the LOD scales of a 1080p view
    assert ba.view_output_size(4032, 3024, 1920, 1.0) == (1920, 1440)
    assert ba.view_output_size(3024, 4032, 1920, 1.0) == (1440, 1920)
    assert ba.view_output_size(1920, 1080, 1920, 1.0) == (1920, 1080)
    assert ba.view_output_size(1920, 1080, 1920, 0.5) == (960, 540)
    assert ba.view_output_size(1920, 1080, 1920, 0.25) == (480, 270)
    assert ba.view_output_size(2000, 3, 1920, 0.1) == (192, 1)   # 3 * 0.096 = 0.288 -> max(., 1) = 1
    assert ba.view_output_size(640, 480, 1920, 2.0) == (640, 480)  # never enlarged
    assert ba.view_output_size(640, 480, 0, 0.5) == (320, 240)    # no cap


def test_restatement_triangle_hand_worked_cases():
    # 2 -> 1: c = 1, taps 0, 1 at (i - 0.5) / 2 = -0.25, 0.25 -> 0.75, 0.75 -> 0.5, 0.5: the pair average, rounded half away
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(2, 2, 3), dtype=np.uint8)
    v = img.astype(np.float64)
    pair = (v[0] + v[1]) / 2
    assert np.array_equal(ref.resize(img, 1, 1, ref.TRIANGLE)[0, 0], np.floor((pair[0] + pair[1]) / 2 + 0.5).astype(np.uint8))
    assert ref.resize(np.array([[10, 21]], np.uint8), 1, 1, ref.TRIANGLE).tolist() == [[16]]   # 15.5 -> 16
    # 4 -> 2: the support widens to 2 source pixels, so a third tap joins with a quarter weight: 0.75 0.75 0.25 over 1.75
    w = ref.pass_weights(4, 2, ref.TRIANGLE)
    f = np.float32
    assert [l for l, _ in w] == [0, 1]
    assert w[0][1].tolist() == [f(f(0.75) / f(1.75)), f(f(0.75) / f(1.75)), f(f(0.25) / f(1.75))]
    assert w[1][1].tolist() == w[0][1].tolist()[::-1]
    row = np.array([[10, 20, 31, 40]], np.uint8)
    assert ref.resize(row, 2, 1, ref.TRIANGLE).tolist() == [[17, 33]]   # 17.29 and 33.29
    # Lanczos3 2 -> 1: both taps at |x| = 0.25: equal weights, the pair average again
    assert ref.resize(np.array([[10, 21]], np.uint8), 1, 1, ref.LANCZOS3).tolist() == [[16]]


@pytest.mark.parametrize("filter", [ref.LANCZOS3, ref.TRIANGLE])
def test_restatement_keeps_a_constant_image_constant(filter):
    for c, val in ((1, 0), (3, 255), (4, 97)):
        img = np.full((37, 53, c), val, np.uint8)
        for nw, nh in ((17, 11), (53, 5), (1, 1), (25, 37), (60, 40)):
            out = ref.resize(img, nw, nh, filter)
            assert out.shape == (nh, nw, c) and (out == val).all(), (c, val, nw, nh, np.unique(out))


def test_restatement_same_size_is_a_copy_and_weights_sum_to_one():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, size=(9, 13, 4), dtype=np.uint8)
    assert np.array_equal(ref.resize(img, 13, 9), img)
    for src, dst in ((4032, 1920), (3024, 1440), (7, 1), (1080, 540), (100, 137)):
        for f in (ref.LANCZOS3, ref.TRIANGLE):
            for left, w in ref.pass_weights(src, dst, f):
                assert 0 <= left < src and left + len(w) <= src
                assert abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-5


def test_restatement_weights_use_the_c_library_sinf():
    # Output 0 of a 4032 -> 1920 Lanczos3 pass, tap 3: x = 1.1666667, a = x * PI_f32 = 0x406a9281.  The C library's sinf gives
    # 0xbf000007 there, numpy's float32 sin 0xbf000006: the restatement must take the former, so its weights differ.
    f = np.float32
    a = np.array([0x406A9281], np.uint32).view(f)[0]
    assert ref.sinf(a).view(np.uint32) == 0xBF000007
    assert np.sin(np.array([a], f))[0].view(np.uint32) == 0xBF000006
    (left, w), = ref.pass_weights(4032, 1920, ref.LANCZOS3)[:1]
    saved = ref.sinf
    try:
        ref.sinf = lambda v: np.sin(np.array([v], f))[0]
        (left_np, w_np), = ref.pass_weights(4032, 1920, ref.LANCZOS3)[:1]
    finally:
        ref.sinf = saved
    assert left == left_np == 0 and len(w) == len(w_np)
    assert not np.array_equal(w.view(np.uint32), w_np.view(np.uint32))
    assert ref.kernel(ref.LANCZOS3, 0.0) == 1.0 and ref.kernel(ref.LANCZOS3, 3.0) == 0.0 and ref.kernel(ref.TRIANGLE, 1.0) == 0.0


def test_restatement_mask_merge_and_pack():
    img = np.zeros((2, 4, 3), np.uint8)
    img[:] = (10, 20, 30)
    mask = np.arange(8, dtype=np.uint8).reshape(2, 4) * 30
    rgba = ref.merge_mask(img, mask)
    assert rgba[:, :, 3].tolist() == mask.tolist() and (rgba[:, :, :3] == (10, 20, 30)).all()   # load_image.rs mask_becomes_alpha
    assert ref.merge_mask(img, mask, invert=True)[:, :, 3].tolist() == (255 - mask).tolist()    # inverted_mask_flips_alpha
    packed, alpha = ref.pack(rgba, premultiply=True)
    assert alpha and packed[0, 1] == ((10 * 30 + 127) // 255) | (((20 * 30 + 127) // 255) << 8) | (((30 * 30 + 127) // 255) << 16) | (30 << 24)
    packed, alpha = ref.pack(img, premultiply=True)
    assert not alpha and (packed == (10 | 20 << 8 | 30 << 16 | 255 << 24)).all()
    small = np.array([[0, 255]], np.uint8)   # a 2 x 1 mask on a 4 x 2 view: Triangle upsampling
    assert ref.merge_mask(img, small)[:, :, 3].tolist() == [[0, 64, 191, 255]] * 2
