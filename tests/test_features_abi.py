"""Feature maps (include/brush_hip_features.h) without a GPU: the header declares exactly the binding's FEATURE_SYMBOLS, the channel
cap and the two loss kinds, the library exports them, _ffi.py, host.py and brush_hip.hpp mirror the same values and the struct's
layout, brush_hip.h declares what it declared before, and argument checks run before the device is touched."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bh_render_features", "bh_render_backward_features_saved", "bh_feature_loss_value_and_grad"}


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def test_header_declares_the_binding_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_features.h"))
    assert declared == set(_ffi.FEATURE_SYMBOLS) == NAMES, declared ^ set(_ffi.FEATURE_SYMBOLS)
    assert '#include "brush_hip.h"' in src
    assert re.findall(r"#define\s+BH_FEATURE_MAX_CHANNELS\s+(\d+)u", src) == ["256"] and _ffi.FEATURE_MAX_CHANNELS == 256
    kinds = dict(re.findall(r"#define\s+BH_FEATURE_LOSS_([A-Z0-9_]+)\s+(\d+)u", src))
    assert kinds == {"L1": "0", "CROSS_ENTROPY": "1"}, kinds
    assert (_ffi.FEATURE_LOSS_L1, _ffi.FEATURE_LOSS_CROSS_ENTROPY) == (0, 1)
    # the struct: the header pins its size with a static_assert, the mirror has the same size, field order and offsets
    sizes = set(re.findall(r"static_assert\(sizeof\(BhFeatureTarget\) == (\d+)", src, flags=re.I))
    assert sizes == {str(C.sizeof(_ffi.BhFeatureTarget))} == {"32"}, sizes
    body = re.search(r"typedef struct BhFeatureTarget \{(.*?)\} BhFeatureTarget;", src, flags=re.S).group(1)
    fields = [n for decl in re.findall(r"(?:const\s+)?(?:void\*|float|uint32_t)\s+([^;]+);", body) for n in re.split(r"\s*,\s*", decl.strip())]
    assert fields == [f[0] for f in _ffi.BhFeatureTarget._fields_] == ["target", "h", "w", "channels", "kind", "weight", "reserved"], fields
    assert [getattr(_ffi.BhFeatureTarget, f).offset for f in fields] == [0, 8, 12, 16, 20, 24, 28]
    # brush_hip.h declares what it declared before (82 entry points; it also names the test-hooks build's bh_debug_fill_train_scratch)
    base, _ = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    assert len(_ffi.SYMBOLS) == 82 and base == set(_ffi.SYMBOLS) | {"bh_debug_fill_train_scratch"} and not (base & declared)
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
    lib = _ffi.load()
    for name in NAMES:
        assert getattr(lib, name) is not None
    assert [len(_ffi.FEATURE_SYMBOLS[k][1]) for k in ("bh_render_features", "bh_render_backward_features_saved", "bh_feature_loss_value_and_grad")] == [5, 14, 5]
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_features.h"' in hpp
    for name in ("DeviceBuffer<float> features(", "backward_features(", "feature_loss_value_and_grad(", "feature_target(",
                 "BH_FEATURE_LOSS_L1 == 0u && BH_FEATURE_LOSS_CROSS_ENTROPY == 1u && BH_FEATURE_MAX_CHANNELS == 256u"):
        assert name in hpp, name
    import brush_amd as ba
    from brush_amd import host
    for name in ("render_features", "feature_loss_value_and_grad", "FeatureField"):
        assert hasattr(ba, name), name
    assert host.FEATURE_LOSS_KINDS == {"l1": 0, "cross_entropy": 1} and host.FEATURE_MAX_CHANNELS == 256
    assert hasattr(ba.RenderNode, "features")
    import inspect
    params = list(inspect.signature(ba.RenderNode.backward).parameters)
    assert params[-2:] == ["v_features", "features"], params   # new trailing keywords: every earlier position is what it was
    # the option that forces a chunk width is listed and documented like every other key
    names = [lib.bh_option_name(i).decode() for i in range(lib.bh_option_count())]
    assert names[-1] == "feature_chunk"


def test_entry_points_reject_a_null_context_without_a_device():
    from brush_amd import _ffi
    lib = _ffi.load()
    t = _ffi.BhFeatureTarget()
    out = _ffi.BhRenderOut()
    assert lib.bh_render_features(None, C.byref(out), None, 3, None) == -1
    assert lib.bh_render_backward_features_saved(None, C.byref(out), None, None, 3, *([None] * 9)) == -1
    assert lib.bh_feature_loss_value_and_grad(None, None, C.byref(t), None, None) == -1
