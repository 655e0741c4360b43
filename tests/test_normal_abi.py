"""Normal maps (include/brush_hip_normal.h) without a GPU: the header declares exactly the binding's NORMAL_SYMBOLS and the two mode
constants, the library exports them, _ffi.py, host.py and brush_hip.hpp mirror the same values, and argument checks run before the
device is touched."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bh_splat_normals", "bh_render_normal", "bh_render_backward_normal_saved", "bh_depth_to_normal", "bh_depth_to_normal_backward"}


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def test_header_declares_the_binding_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_normal.h"))
    assert declared == set(_ffi.NORMAL_SYMBOLS) == NAMES, declared ^ set(_ffi.NORMAL_SYMBOLS)
    assert '#include "brush_hip.h"' in src
    modes = dict(re.findall(r"#define\s+BH_NORMAL_([A-Z]+)\s+(\d+)u", src))
    assert modes == {"ACCUMULATED": "0", "UNIT": "1"}, modes
    assert (_ffi.NORMAL_ACCUMULATED, _ffi.NORMAL_UNIT) == (0, 1)
    # brush_hip.h and brush_hip_depth.h gain nothing: their sets stay disjoint from the normal table
    base, _ = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    depth, _ = _declared(os.path.join(ROOT, "include", "brush_hip_depth.h"))
    assert set(_ffi.SYMBOLS) <= base and not (base & declared) and not (depth & declared)
    assert depth == set(_ffi.DEPTH_SYMBOLS)
    for path in (_ffi.LIB_PATH, _ffi.TEST_HOOKS_LIB_PATH):
        exported = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in _ffi.NORMAL_SYMBOLS:
            assert re.search(r"\bT %s$" % name, exported, flags=re.M), (path, name)
    for lib in (_ffi.load(), _ffi.load_test_hooks()):   # both _bind calls carry the table
        for name, (_, args) in _ffi.NORMAL_SYMBOLS.items():
            assert getattr(lib, name).argtypes == args
    counts = {name: len(args) for name, (_, args) in _ffi.NORMAL_SYMBOLS.items()}
    assert counts == {"bh_splat_normals": 5, "bh_render_normal": 5, "bh_render_backward_normal_saved": 14, "bh_depth_to_normal": 6,
                      "bh_depth_to_normal_backward": 7}
    # the argument counts of the header's prototypes
    for name, want in counts.items():
        proto = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert proto.count(",") + 1 == want, (name, proto)
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_normal.h"' in hpp
    for name in ("normal(uint32_t mode", "backward_normal(", "splat_normals(", "depth_to_normal(", "depth_to_normal_backward(", "bh_render_normal(",
                 "bh_render_backward_normal_saved(", "bh_splat_normals(", "bh_depth_to_normal(", "bh_depth_to_normal_backward(",
                 "BH_NORMAL_ACCUMULATED == 0u && BH_NORMAL_UNIT == 1u"):
        assert name in hpp, name
    import brush_amd as ba
    from brush_amd import host
    for name in ("splat_normals", "render_normal", "depth_to_normal", "depth_to_normal_backward"):
        assert hasattr(ba, name), name
    assert hasattr(ba.RenderNode, "normal")
    assert host.NORMAL_MODES == {"accumulated": 0, "unit": 1}


def test_entry_points_reject_a_null_context_without_a_device():
    from brush_amd import _ffi
    lib = _ffi.load()
    out, cam = _ffi.BhRenderOut(), _ffi.BhCamera()
    assert lib.bh_splat_normals(None, cam, None, 0, None) == -1
    assert lib.bh_render_normal(None, out, None, 0, None) == -1
    assert lib.bh_render_backward_normal_saved(None, out, None, None, 0, None, 0, None, None, None, None, None, None, None) == -1
    assert lib.bh_depth_to_normal(None, cam, None, 4, 4, None) == -1
    assert lib.bh_depth_to_normal_backward(None, cam, None, None, 4, 4, None) == -1
