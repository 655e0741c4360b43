"""Per-view bilateral grids (include/brush_hip_bilagrid.h) without a GPU: the header declares exactly the binding's BILAGRID_SYMBOLS,
both libraries export them, brush_hip.h keeps its 82, brush_hip.hpp and host.py mirror the surface, a null context is refused
before the device is touched, and the trainer refuses the tile partition and an exposure table beside the grids."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bh_bilagrid_create", "bh_bilagrid_destroy", "bh_bilagrid_dims", "bh_bilagrid_set_params", "bh_bilagrid_get_params",
         "bh_bilagrid_get_grad", "bh_bilagrid_get_state", "bh_bilagrid_set_state", "bh_bilagrid_set_adam", "bh_bilagrid_slice",
         "bh_bilagrid_backward", "bh_bilagrid_tv", "bh_train_set_bilagrid"}


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def test_header_declares_the_binding_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_bilagrid.h"))
    assert declared == set(_ffi.BILAGRID_SYMBOLS) == NAMES, declared ^ set(_ffi.BILAGRID_SYMBOLS)
    assert '#include "brush_hip.h"' in src
    base, _ = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    assert set(_ffi.SYMBOLS) <= base and not (base & declared)
    assert len(_ffi.SYMBOLS) == 82
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported_th = subprocess.run(["nm", "-D", "--defined-only", _ffi.TEST_HOOKS_LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = _ffi.load()
    for name in _ffi.BILAGRID_SYMBOLS:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
        assert re.search(r"\bT %s$" % name, exported_th, flags=re.M), name
        assert getattr(lib, name) is not None
    assert len(_ffi.BILAGRID_SYMBOLS["bh_bilagrid_backward"][1]) == 10 and len(_ffi.BILAGRID_SYMBOLS["bh_bilagrid_slice"][1]) == 7
    assert len(_ffi.BILAGRID_SYMBOLS["bh_bilagrid_create"][1]) == 6 and len(_ffi.BILAGRID_SYMBOLS["bh_train_set_bilagrid"][1]) == 3
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_bilagrid.h"' in hpp
    for name in NAMES:
        assert name + "(" in hpp, name


def test_python_mirror_has_the_surface():
    import brush_amd as ba
    for name in ("params", "grads", "state", "set_state", "set_lr", "set_view", "slice", "backward", "tv", "to_gsplat", "from_gsplat", "close"):
        assert hasattr(ba.BilateralGridTable, name), name
    assert isinstance(ba.BilateralGridTable.params, property) and ba.BilateralGridTable.params.fset is not None
    sig = inspect.signature(ba.BilateralGridTable.backward).parameters
    assert sig["update"].default is False and sig["tv_weight"].default == 0.0
    init = inspect.signature(ba.BilateralGridTable.__init__).parameters
    assert init["grid"].default == (16, 16, 8) and init["lr"].default == 2e-3 and init["eps"].default == 1e-15
    sig = inspect.signature(ba.SplatTrainer.__init__).parameters
    assert "bilagrid" in sig and "bilagrid_lr" in sig and sig["bilagrid_tv_weight"].default == 10.0


def test_layout_mapping_round_trips():
    import bilagrid_ref as br
    g = np.arange(3 * 4 * 2 * 12, dtype=np.float64).reshape(3, 4, 2, 12)
    s = br.to_gsplat(g)
    assert s.shape == (12, 2, 3, 4) and s[7, 1, 2, 3] == g[2, 3, 1, 7] and np.array_equal(br.from_gsplat(s), g)


def test_entry_points_reject_a_null_context_without_a_device():
    from brush_amd import _ffi
    lib = _ffi.load()
    h = C.c_void_p()
    assert lib.bh_bilagrid_create(None, 3, 16, 16, 8, C.byref(h)) == -1 and not h.value
    assert lib.bh_bilagrid_destroy(None, None) == -1
    assert lib.bh_bilagrid_dims(None, None, None, None, None, None) == -1
    assert lib.bh_bilagrid_set_params(None, None, 1, 1, None) == -1 and lib.bh_bilagrid_get_params(None, None, 1, 1, None) == -1
    assert lib.bh_bilagrid_get_grad(None, None, 1, 1, None) == -1
    assert lib.bh_bilagrid_get_state(None, None, 1, None, None, None) == -1 and lib.bh_bilagrid_set_state(None, None, 1, None, None, 0) == -1
    assert lib.bh_bilagrid_set_adam(None, None, 2e-3, 0.9, 0.999, 1e-15) == -1
    assert lib.bh_bilagrid_slice(None, None, 1, None, 1, 1, None) == -1
    assert lib.bh_bilagrid_backward(None, None, 1, None, None, 1, 1, None, 0.0, 0) == -1
    assert lib.bh_bilagrid_tv(None, None, 1, None) == -1
    assert lib.bh_train_set_bilagrid(None, None, 0.0) == -1


def test_trainer_refuses_the_tile_partition_and_an_exposure_table():
    import brush_amd as ba
    import pytest
    with pytest.raises(ValueError, match="bilagrid is not available"):
        ba.SplatTrainer(ba.TrainConfig(), partition="tiles", bilagrid=object())
    with pytest.raises(ValueError, match="alternatives"):
        ba.SplatTrainer(ba.TrainConfig(), bilagrid=object(), exposure=object())
