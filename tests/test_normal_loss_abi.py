"""Normal consistency (include/brush_hip_normal_loss.h) without a GPU: the header declares exactly the binding's NORMAL_LOSS_SYMBOLS
and parses as C and as C++, the library exports them, _ffi.py and brush_hip.hpp mirror the struct's size, the older headers declare
what they declared before (brush_hip.h its 82 entry points), and argument checks run before the device is touched."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bh_normal_consistency_value_and_grad", "bh_train_set_normal"}


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def test_header_parses_as_c_and_as_cpp(tmp_path):
    inc = os.path.join(ROOT, "include")
    for lang, std, ext in (("c", "-std=c11", "c"), ("c++", "-std=c++17", "cpp")):
        src = tmp_path / ("parse." + ext)
        src.write_text('#include "brush_hip_normal_loss.h"\nint main(void) { return (int)sizeof(BhNormalTermConfig) - 16; }\n')
        exe = str(tmp_path / ("parse_" + ext))
        subprocess.check_call([os.environ.get("CXX", "g++"), "-x", lang, std, "-Wall", "-Werror", "-I" + inc, str(src), "-o", exe])
        assert subprocess.run([exe]).returncode == 0


def test_header_declares_the_binding_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_normal_loss.h"))
    assert declared == set(_ffi.NORMAL_LOSS_SYMBOLS) == NAMES, declared ^ set(_ffi.NORMAL_LOSS_SYMBOLS)
    assert '#include "brush_hip_normal.h"' in src and '#include "brush_hip_depth_loss.h"' in src
    # the struct: the header pins its size with a static_assert, the mirror has the same size and field order
    sizes = set(re.findall(r"static_assert\(sizeof\(BhNormalTermConfig\) == (\d+)", src, flags=re.I))
    assert sizes == {str(C.sizeof(_ffi.BhNormalTermConfig))} == {"16"}, sizes
    assert [f[0] for f in _ffi.BhNormalTermConfig._fields_] == ["weight", "reserved"]
    assert _ffi.BhNormalTermConfig.weight.offset == 0 and _ffi.BhNormalTermConfig.reserved.offset == 4
    # the older headers declare what they declared before
    base, _ = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    normal, _ = _declared(os.path.join(ROOT, "include", "brush_hip_normal.h"))
    depth_loss, _ = _declared(os.path.join(ROOT, "include", "brush_hip_depth_loss.h"))
    # (82 entry points; the header also names the test-hooks build's bh_debug_fill_train_scratch)
    assert len(_ffi.SYMBOLS) == 82 and base == set(_ffi.SYMBOLS) | {"bh_debug_fill_train_scratch"} and not (base & declared)
    assert normal == set(_ffi.NORMAL_SYMBOLS) and len(normal) == 5 and not (normal & declared)
    assert depth_loss == set(_ffi.DEPTH_LOSS_SYMBOLS) and len(depth_loss) == 3 and not (depth_loss & declared)
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
    lib = _ffi.load()
    for name in NAMES:
        assert getattr(lib, name) is not None
    assert [len(_ffi.NORMAL_LOSS_SYMBOLS[k][1]) for k in ("bh_normal_consistency_value_and_grad", "bh_train_set_normal")] == [12, 2]
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_normal_loss.h"' in hpp
    for name in ("normal_consistency_value_and_grad(", "train_set_normal(", "bh_train_set_normal(", "sizeof(BhNormalTermConfig) == 16"):
        assert name in hpp, name
    import brush_amd as ba
    assert hasattr(ba, "normal_consistency_value_and_grad")
    assert ba.TrainConfig().normal_loss_weight == 0.0 and ba.TrainConfig().normal_loss_from_iter == 0
    mk = open(os.path.join(ROOT, "brush_amd", "csrc", "Makefile")).read()
    assert " normal_loss.hip" in mk and mk.count("brush_hip_normal_loss.h") == 2 and mk.count("device_depth_normal.h") == 2


def test_entry_points_reject_a_null_context_without_a_device():
    from brush_amd import _ffi
    lib = _ffi.load()
    cfg = _ffi.BhNormalTermConfig(weight=0.5)
    cam = _ffi.BhCamera()
    assert lib.bh_normal_consistency_value_and_grad(None, C.byref(cam), None, None, None, 4, 4, 1.0, 0, None, None, None) == -1
    assert lib.bh_train_set_normal(None, C.byref(cfg)) == -1 and lib.bh_train_set_normal(None, None) == -1
