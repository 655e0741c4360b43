"""LPIPS (crates/lpips/src/lib.rs) without a GPU: include/brush_hip_lpips.h declares exactly the binding's LPIPS_SYMBOLS and the
library exports them, argument checks run before the device is touched, both state-dict key schemes map to the canonical flat
vector, and the torch restatement tests/lpips_ref.py has the reference's identity and symmetry properties."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import lpips_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def test_header_declares_the_binding_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_lpips.h"))
    assert declared == set(_ffi.LPIPS_SYMBOLS), declared ^ set(_ffi.LPIPS_SYMBOLS)
    assert '#include "brush_hip.h"' in src
    m = re.search(r"#define\s+BH_LPIPS_PARAM_COUNT\s+(\d+)u", src)
    assert m and int(m.group(1)) == _ffi.LPIPS_PARAM_COUNT == lpips_ref.PARAM_COUNT
    assert lpips_ref.PARAM_COUNT == sum(co * ci * 9 + co for ci, co in lpips_ref.CONVS) + sum(lpips_ref.HEADS)
    assert sum(co * ci * 9 + co for ci, co in lpips_ref.CONVS) == 14714688
    # brush_hip.h gains nothing: its set stays the binding's SYMBOLS, disjoint from the LPIPS table
    base, _ = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    assert not (base & declared)
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in _ffi.LPIPS_SYMBOLS:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
    lib = _ffi.load()
    for name in _ffi.LPIPS_SYMBOLS:
        assert getattr(lib, name) is not None
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_lpips.h"' in hpp
    for name in ("class Lpips", "lpips(", "lpips_value_and_grad(", "train_set_lpips("):
        assert name in hpp, name
    import brush_amd as ba
    for name in ("Lpips", "lpips", "lpips_value_and_grad"):
        assert hasattr(ba, name), name
    assert ba.TrainConfig().lpips_loss_weight == 0.0


def test_entry_points_reject_bad_arguments_without_a_device():
    import ctypes as C
    from brush_amd import _ffi
    lib = _ffi.load()
    flat = np.zeros(8, np.float32)
    assert lib.bh_lpips_create(None, flat.ctypes.data_as(C.POINTER(C.c_float)), 8) is None
    assert lib.bh_lpips_create(None, None, _ffi.LPIPS_PARAM_COUNT) is None
    lib.bh_lpips_destroy(None)   # (a no-op)
    assert lib.bh_lpips_forward(None, None, None, None, 16, 16, None, None) == -1
    assert lib.bh_lpips_value_and_grad(None, None, None, None, 16, 16, None, 1.0, None, None) == -1
    assert lib.bh_train_set_lpips(None, None, 0.0) == -1


def _random_burn_state_dict(seed):
    rng = np.random.default_rng(seed)
    sd, L = {}, 0
    for b, n in enumerate(lpips_ref.BLOCK_CONVS):
        for j in range(n):
            ci, co = lpips_ref.CONVS[L]
            sd["blocks.%d.convs.%d.weight" % (b, j)] = torch.from_numpy(rng.standard_normal((co, ci, 3, 3)).astype(np.float32))
            sd["blocks.%d.convs.%d.bias" % (b, j)] = torch.from_numpy(rng.standard_normal(co).astype(np.float32))
            L += 1
    for b, c in enumerate(lpips_ref.HEADS):
        sd["heads.%d.weight" % b] = torch.from_numpy(rng.random((1, c, 1, 1)).astype(np.float32))
    return sd


def test_state_dict_key_schemes_map_to_the_same_flat_vector():
    import brush_amd as ba
    burn = _random_burn_state_dict(1)
    # the torch `lpips` package's names for the same tensors
    idx = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
    tv = {"scaling_layer.shift": torch.tensor([-0.030, -0.088, -0.188]).reshape(1, 3, 1, 1),
          "scaling_layer.scale": torch.tensor([0.458, 0.448, 0.450]).reshape(1, 3, 1, 1)}
    for b, n in enumerate(lpips_ref.BLOCK_CONVS):
        for j in range(n):
            for p in ("weight", "bias"):
                tv["net.slice%d.%d.%s" % (b + 1, idx[b][j], p)] = burn["blocks.%d.convs.%d.%s" % (b, j, p)]
        tv["lin%d.model.1.weight" % b] = burn["heads.%d.weight" % b]
    a = ba.Lpips.flat_from_state_dict(burn)
    t = ba.Lpips.flat_from_state_dict(tv)
    assert a.dtype == np.float32 and a.size == lpips_ref.PARAM_COUNT
    assert np.array_equal(a, t)
    # canonical order: conv 0's weight first, then its bias; the heads last
    assert np.array_equal(a[:64 * 27], burn["blocks.0.convs.0.weight"].numpy().reshape(-1))
    assert np.array_equal(a[64 * 27:64 * 28], burn["blocks.0.convs.0.bias"].numpy())
    assert np.array_equal(a[-512:], burn["heads.4.weight"].numpy().reshape(-1))
    convs, heads = lpips_ref.unpack_params(a)
    assert np.array_equal(convs[7][0], burn["blocks.3.convs.0.weight"].numpy())
    bad = dict(tv)
    bad["scaling_layer.scale"] = torch.ones(1, 3, 1, 1)
    with pytest.raises(ValueError, match="scale"):
        ba.Lpips.flat_from_state_dict(bad)
    bad = dict(burn)
    bad["blocks.1.convs.0.weight"] = torch.zeros(128, 63, 3, 3)
    with pytest.raises(ValueError, match="shape"):
        ba.Lpips.flat_from_state_dict(bad)


def test_random_params_have_the_canonical_layout():
    import brush_amd as ba
    a = ba.Lpips.random_params(3)
    assert a.dtype == np.float32 and a.size == lpips_ref.PARAM_COUNT
    assert np.array_equal(a, ba.Lpips.random_params(3))
    _, heads = lpips_ref.unpack_params(a)
    assert all(np.all(h >= 0) for h in heads)


def test_reference_restatement_has_the_reference_properties():
    """The reference's test_structural_properties (crates/lpips/src/lib.rs): LPIPS(x, x) < 1e-5 and LPIPS(a, b) == LPIPS(b, a),
    for any weights; plus a distance that grows with the perturbation."""
    import brush_amd as ba
    m = lpips_ref.Model(ba.Lpips.random_params(2), torch.float32)
    rng = np.random.default_rng(0)
    h, w = 40, 52
    a = torch.from_numpy(rng.random((h, w, 3)).astype(np.float32))
    b = torch.from_numpy(rng.random((h, w, 3)).astype(np.float32))
    with torch.no_grad():
        assert abs(float(m.lpips(a, a))) < 1e-5
        ab, ba_ = float(m.lpips(a, b)), float(m.lpips(b, a))
        assert ab > 0 and abs(ab - ba_) < 1e-5, (ab, ba_)
        small = float(m.lpips(a, (a + 0.01 * (b - a))))
        assert 0 < small < ab
    # f64 and f32 agree closely on the same inputs
    m64 = lpips_ref.Model(ba.Lpips.random_params(2), torch.float64)
    with torch.no_grad():
        v64 = float(m64.lpips(a.double(), b.double()))
    assert abs(v64 - ab) < 1e-5 * abs(v64)


def test_gt_decode_composites_like_unpack_gt_rgb():
    g = lpips_ref.pack_rgba8(np.array([255, 0]), np.array([128, 10]), np.array([0, 20]), np.array([255, 0]))
    plain = lpips_ref.gt_rgb(g)
    assert plain[0, 0] == np.float32(1.0) and plain[1, 2] == np.float32(20) * np.float32(1 / 255)
    comp = lpips_ref.gt_rgb(g, (0.5, 0.25, 1.0))
    assert np.array_equal(comp[0], plain[0])   # opaque: unchanged
    assert comp[1, 0] == np.float32(0.5) and comp[1, 2] == np.float32(np.float32(20) * np.float32(1 / 255) + np.float32(1.0))
