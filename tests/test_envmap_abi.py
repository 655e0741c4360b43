"""Environment maps (include/brush_hip_envmap.h) without a GPU: the header declares exactly the binding's ENVMAP_SYMBOLS, both
libraries export them, brush_hip.h keeps its 82, brush_hip.hpp and host.py mirror the surface, a null context is refused before the
device is touched, and SplatTrainer refuses what the term cannot do."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bh_envmap_create", "bh_envmap_destroy", "bh_envmap_set_params", "bh_envmap_get_params", "bh_envmap_get_grad", "bh_envmap_get_state",
         "bh_envmap_set_state", "bh_envmap_set_adam", "bh_envmap_composite", "bh_envmap_backward", "bh_train_set_envmap"}


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def test_header_declares_the_binding_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_envmap.h"))
    assert declared == set(_ffi.ENVMAP_SYMBOLS) == NAMES, declared ^ set(_ffi.ENVMAP_SYMBOLS)
    assert '#include "brush_hip.h"' in src
    base, _ = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    assert set(_ffi.SYMBOLS) <= base and not (base & declared)
    assert len(_ffi.SYMBOLS) == 82
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported_th = subprocess.run(["nm", "-D", "--defined-only", _ffi.TEST_HOOKS_LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = _ffi.load()
    for name in _ffi.ENVMAP_SYMBOLS:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
        assert re.search(r"\bT %s$" % name, exported_th, flags=re.M), name
        assert getattr(lib, name) is not None
    assert len(_ffi.ENVMAP_SYMBOLS["bh_envmap_backward"][1]) == 9 and len(_ffi.ENVMAP_SYMBOLS["bh_envmap_composite"][1]) == 7
    assert re.search(r"#define\s+BH_ENVMAP_MAX_RESOLUTION\s+%du" % _ffi.ENVMAP_MAX_RESOLUTION, src)
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_envmap.h"' in hpp and "class EnvironmentMap" in hpp and "train_set_envmap(" in hpp
    for name in NAMES:
        assert name + "(" in hpp, name


def test_python_mirror_has_the_surface():
    import brush_amd as ba
    for name in ("params", "grads", "state", "set_state", "set_lr", "composite", "backward", "close"):
        assert hasattr(ba.EnvironmentMap, name), name
    assert isinstance(ba.EnvironmentMap.params, property) and ba.EnvironmentMap.params.fset is not None
    assert "update" in inspect.signature(ba.EnvironmentMap.backward).parameters
    init = inspect.signature(ba.EnvironmentMap.__init__).parameters
    assert init["resolution"].default == 64
    assert init["lr"].default == inspect.signature(ba.ExposureTable.__init__).parameters["lr"].default
    sig = inspect.signature(ba.SplatTrainer.__init__).parameters
    assert "envmap" in sig and "envmap_lr" in sig
    assert "envmap" in inspect.signature(ba.run_eval).parameters and inspect.signature(ba.run_eval).parameters["envmap"].default is None
    assert "envmap" not in inspect.signature(ba.fuse_views).parameters


def test_entry_points_reject_a_null_context_without_a_device():
    from brush_amd import _ffi
    lib = _ffi.load()
    h = C.c_void_p()
    assert lib.bh_envmap_create(None, 64, C.byref(h)) == -1 and not h.value
    assert lib.bh_envmap_destroy(None, None) == -1
    assert lib.bh_envmap_set_params(None, None, None) == -1 and lib.bh_envmap_get_params(None, None, None) == -1
    assert lib.bh_envmap_get_grad(None, None, None) == -1
    assert lib.bh_envmap_get_state(None, None, None, None, None) == -1 and lib.bh_envmap_set_state(None, None, None, None, 0) == -1
    assert lib.bh_envmap_set_adam(None, None, 1e-3, 0.9, 0.999, 1e-15) == -1
    assert lib.bh_envmap_composite(None, None, None, None, 1, 1, None) == -1
    assert lib.bh_envmap_backward(None, None, None, None, None, 1, 1, None, 0) == -1
    assert lib.bh_train_set_envmap(None, None) == -1


def test_trainer_refuses_what_the_map_cannot_do():
    import brush_amd as ba
    with pytest.raises(ValueError, match="envmap is not available"):
        ba.SplatTrainer(ba.TrainConfig(), partition="tiles", envmap=object())
    with pytest.raises(ValueError, match="background_color"):
        ba.SplatTrainer(ba.TrainConfig(background_color=(0.0, 0.1, 0.0)), envmap=object())
    with pytest.raises(ValueError, match="pose_optimizer"):
        ba.SplatTrainer(ba.TrainConfig(), envmap=object(), pose_optimizer=object())
    assert ba.SplatTrainer(ba.TrainConfig(), envmap=None).envmap is None
