"""Per-view exposure compensation (include/brush_hip_exposure.h) without a GPU: the header declares exactly the binding's
EXPOSURE_SYMBOLS, the library exports them, brush_hip.h keeps its 82, brush_hip.hpp and host.py mirror the surface, and a null
context is refused before the device is touched."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bh_exposure_create", "bh_exposure_destroy", "bh_exposure_set_params", "bh_exposure_get_params", "bh_exposure_get_grad",
         "bh_exposure_get_state", "bh_exposure_set_state", "bh_exposure_set_adam", "bh_exposure_apply", "bh_exposure_backward",
         "bh_train_set_exposure"}


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def test_header_declares_the_binding_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_exposure.h"))
    assert declared == set(_ffi.EXPOSURE_SYMBOLS) == NAMES, declared ^ set(_ffi.EXPOSURE_SYMBOLS)
    assert '#include "brush_hip.h"' in src
    base, _ = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    assert set(_ffi.SYMBOLS) <= base and not (base & declared)
    assert len(_ffi.SYMBOLS) == 82
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported_th = subprocess.run(["nm", "-D", "--defined-only", _ffi.TEST_HOOKS_LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = _ffi.load()
    for name in _ffi.EXPOSURE_SYMBOLS:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
        assert re.search(r"\bT %s$" % name, exported_th, flags=re.M), name
        assert getattr(lib, name) is not None
    assert len(_ffi.EXPOSURE_SYMBOLS["bh_exposure_backward"][1]) == 9 and len(_ffi.EXPOSURE_SYMBOLS["bh_exposure_apply"][1]) == 7
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_exposure.h"' in hpp
    for name in NAMES:
        assert name + "(" in hpp, name


def test_python_mirror_has_the_surface():
    import brush_amd as ba
    for name in ("params", "grads", "state", "set_state", "set_lr", "apply", "backward", "close"):
        assert hasattr(ba.ExposureTable, name), name
    assert isinstance(ba.ExposureTable.params, property) and ba.ExposureTable.params.fset is not None
    assert "update" in inspect.signature(ba.ExposureTable.backward).parameters
    sig = inspect.signature(ba.SplatTrainer.__init__).parameters
    assert "exposure" in sig and "exposure_lr" in sig


def test_entry_points_reject_a_null_context_without_a_device():
    from brush_amd import _ffi
    lib = _ffi.load()
    h = C.c_void_p()
    assert lib.bh_exposure_create(None, 3, C.byref(h)) == -1 and not h.value
    assert lib.bh_exposure_destroy(None, None) == -1
    assert lib.bh_exposure_set_params(None, None, 1, 1, None) == -1 and lib.bh_exposure_get_params(None, None, 1, 1, None) == -1
    assert lib.bh_exposure_get_grad(None, None, 1, 1, None) == -1
    assert lib.bh_exposure_get_state(None, None, 1, None, None, None) == -1 and lib.bh_exposure_set_state(None, None, 1, None, None, 0) == -1
    assert lib.bh_exposure_set_adam(None, None, 1e-3, 0.9, 0.999, 1e-8) == -1
    assert lib.bh_exposure_apply(None, None, 1, None, 1, 1, None) == -1
    assert lib.bh_exposure_backward(None, None, 1, None, None, 1, 1, None, 0) == -1
    assert lib.bh_train_set_exposure(None, None) == -1


def test_trainer_refuses_a_table_with_the_tile_partition():
    import brush_amd as ba
    import pytest
    with pytest.raises(ValueError, match="exposure is not available"):
        ba.SplatTrainer(ba.TrainConfig(), partition="tiles", exposure=object())
