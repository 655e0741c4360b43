"""Depth maps (include/brush_hip_depth.h) without a GPU: the header declares exactly the binding's DEPTH_SYMBOLS and the three mode
constants, the library exports them, _ffi.py and brush_hip.hpp mirror the same values, and argument checks run before the device
is touched."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def test_header_declares_the_binding_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_depth.h"))
    assert declared == set(_ffi.DEPTH_SYMBOLS) == {"bh_render_depth", "bh_render_backward_depth_saved"}, declared ^ set(_ffi.DEPTH_SYMBOLS)
    assert '#include "brush_hip.h"' in src
    modes = dict(re.findall(r"#define\s+BH_DEPTH_([A-Z]+)\s+(\d+)u", src))
    assert modes == {"ACCUMULATED": "0", "EXPECTED": "1", "MEDIAN": "2"}, modes
    assert (_ffi.DEPTH_ACCUMULATED, _ffi.DEPTH_EXPECTED, _ffi.DEPTH_MEDIAN) == (0, 1, 2)
    # brush_hip.h gains nothing: its set stays the binding's SYMBOLS, disjoint from the depth table
    base, _ = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    assert set(_ffi.SYMBOLS) <= base and not (base & declared)
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in _ffi.DEPTH_SYMBOLS:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
    lib = _ffi.load()
    for name in _ffi.DEPTH_SYMBOLS:
        assert getattr(lib, name) is not None
    assert len(_ffi.DEPTH_SYMBOLS["bh_render_depth"][1]) == 4 and len(_ffi.DEPTH_SYMBOLS["bh_render_backward_depth_saved"][1]) == 12
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_depth.h"' in hpp
    for name in ("depth(uint32_t mode", "bh_render_depth(", "bh_render_backward_depth_saved(", "BH_DEPTH_EXPECTED"):
        assert name in hpp, name
    import brush_amd as ba
    from brush_amd import host
    assert hasattr(ba, "render_depth") and hasattr(ba.RenderNode, "depth")
    assert host.DEPTH_MODES == {"accumulated": 0, "expected": 1, "median": 2}


def test_entry_points_reject_a_null_context_without_a_device():
    from brush_amd import _ffi
    lib = _ffi.load()
    out = _ffi.BhRenderOut()
    assert lib.bh_render_depth(None, out, 0, None) == -1
    assert lib.bh_render_backward_depth_saved(None, out, None, None, 0, None, None, None, None, None, None, None) == -1
