"""Depth supervision (include/brush_hip_depth_loss.h) without a GPU: the header declares exactly the binding's DEPTH_LOSS_SYMBOLS and
the two kind constants, the library exports them, _ffi.py and brush_hip.hpp mirror the same values and the struct's size, the older
headers declare what they declared before, and argument checks run before the device is touched."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bh_depth_loss_value_and_grad", "bh_train_set_depth", "bh_eval_depth_metrics"}


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def test_header_declares_the_binding_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_depth_loss.h"))
    assert declared == set(_ffi.DEPTH_LOSS_SYMBOLS) == NAMES, declared ^ set(_ffi.DEPTH_LOSS_SYMBOLS)
    assert '#include "brush_hip_depth.h"' in src
    kinds = dict(re.findall(r"#define\s+BH_DEPTH_LOSS_([A-Z0-9]+)\s+(\d+)u", src))
    assert kinds == {"L1": "0", "DISPARITY": "1"}, kinds
    assert (_ffi.DEPTH_LOSS_L1, _ffi.DEPTH_LOSS_DISPARITY) == (0, 1)
    # the struct: the header pins its size with a static_assert, the mirror has the same size and field order
    sizes = set(re.findall(r"static_assert\(sizeof\(BhDepthTarget\) == (\d+)", src, flags=re.I))
    assert sizes == {str(C.sizeof(_ffi.BhDepthTarget))} == {"32"}, sizes
    body = re.search(r"typedef struct BhDepthTarget \{(.*?)\} BhDepthTarget;", src, flags=re.S).group(1)
    fields = [n for decl in re.findall(r"(?:const\s+)?(?:float\*?|uint32_t)\s+([^;]+);", body) for n in re.split(r"\s*,\s*", decl.strip())]
    assert fields == [f[0] for f in _ffi.BhDepthTarget._fields_] == ["gt", "h", "w", "kind", "weight", "scale", "offset"], fields
    assert [getattr(_ffi.BhDepthTarget, f).offset for f in fields] == [0, 8, 12, 16, 20, 24, 28]
    # the older headers declare what they declared before
    base, _ = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    depth, _ = _declared(os.path.join(ROOT, "include", "brush_hip_depth.h"))
    # (82 entry points; the header also names the test-hooks build's bh_debug_fill_train_scratch)
    assert len(_ffi.SYMBOLS) == 82 and base == set(_ffi.SYMBOLS) | {"bh_debug_fill_train_scratch"} and not (base & declared)
    assert depth == set(_ffi.DEPTH_SYMBOLS) == {"bh_render_depth", "bh_render_backward_depth_saved"} and not (depth & declared)
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
    lib = _ffi.load()
    for name in NAMES:
        assert getattr(lib, name) is not None
    assert [len(_ffi.DEPTH_LOSS_SYMBOLS[k][1]) for k in ("bh_depth_loss_value_and_grad", "bh_train_set_depth", "bh_eval_depth_metrics")] == [5, 2, 4]
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_depth_loss.h"' in hpp
    for name in ("depth_loss_value_and_grad(", "eval_depth_metrics(", "train_set_depth(", "bh_train_set_depth(", "BH_DEPTH_LOSS_L1 == 0u && BH_DEPTH_LOSS_DISPARITY == 1u"):
        assert name in hpp, name
    import brush_amd as ba
    from brush_amd import host
    assert hasattr(ba, "depth_loss_value_and_grad") and hasattr(ba, "eval_depth_metrics")
    assert host.DEPTH_LOSS_KINDS == {"l1": 0, "disparity": 1}
    batch_fields = ba.SceneBatch.__dataclass_fields__
    assert batch_fields["depth"].default is None and batch_fields["depth_scale"].default == 1.0 and batch_fields["depth_offset"].default == 0.0
    cfg = ba.TrainConfig(depth_loss_weight=0.5, depth_loss_weight_end=0.005, total_train_iters=1000)
    assert ba.TrainConfig().depth_loss_weight == 0.0 and ba.TrainConfig().depth_loss_kind == "l1"
    assert cfg.depth_weight_at(1) == 0.5 and abs(cfg.depth_weight_at(501) - 0.05) < 1e-12 and abs(cfg.depth_weight_at(1001) - 0.005) < 1e-12
    assert ba.TrainConfig(depth_loss_weight=0.5).depth_weight_at(700) == 0.5


def test_entry_points_reject_a_null_context_without_a_device():
    from brush_amd import _ffi
    lib = _ffi.load()
    t = _ffi.BhDepthTarget()
    assert lib.bh_depth_loss_value_and_grad(None, None, C.byref(t), None, None) == -1
    assert lib.bh_train_set_depth(None, C.byref(t)) == -1 and lib.bh_train_set_depth(None, None) == -1
    assert lib.bh_eval_depth_metrics(None, None, C.byref(t), None) == -1
