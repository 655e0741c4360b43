"""Feature fields trained with the splats (include/brush_hip_feature_train.h) without a GPU: the header declares exactly the binding's
FEATURE_TRAIN_SYMBOLS and the two carry modes, the library exports them, _ffi.py, host.py and brush_hip.hpp mirror the struct's layout
and the surface, brush_hip_features.h and brush_hip.h declare what they declared before, the option list is what it was, and both
entry points refuse a null context before the device is touched."""
import ctypes as C
import dataclasses
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bh_train_set_features", "bh_refine_carry_rows"}
FEATURE_NAMES = {"bh_render_features", "bh_render_backward_features_saved", "bh_feature_loss_value_and_grad"}


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def test_header_declares_the_binding_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_feature_train.h"))
    assert declared == set(_ffi.FEATURE_TRAIN_SYMBOLS) == NAMES, declared ^ set(_ffi.FEATURE_TRAIN_SYMBOLS)
    assert '#include "brush_hip_features.h"' in src
    modes = dict(re.findall(r"#define\s+BH_CARRY_([A-Z_]+)\s+(\d+)u", src))
    assert modes == {"COPY": "0", "ZERO_SPLIT": "1", "MAX_CHANNELS": "4096"}, modes
    assert (_ffi.CARRY_COPY, _ffi.CARRY_ZERO_SPLIT, _ffi.CARRY_MAX_CHANNELS) == (0, 1, 4096)
    # the struct: the header pins its size with a static_assert, the mirror has the same size, field order and offsets
    sizes = set(re.findall(r"static_assert\(sizeof\(BhFeatureField\) == (\d+)", src, flags=re.I))
    assert sizes == {str(C.sizeof(_ffi.BhFeatureField))} == {"56"}, sizes
    body = re.search(r"typedef struct BhFeatureField \{(.*?)\} BhFeatureField;", src, flags=re.S).group(1)
    fields = [n.lstrip("*") for decl in re.findall(r"(?:float|uint32_t)\s+([^;]+);", body) for n in re.split(r"\s*,\s*", decl.strip())]
    want = ["features", "m1", "m2", "n", "channels", "step", "lr", "beta1", "beta2", "eps", "reserved"]
    assert fields == [f[0] for f in _ffi.BhFeatureField._fields_] == want, fields
    assert [getattr(_ffi.BhFeatureField, f).offset for f in fields] == [0, 8, 16, 24, 28, 32, 36, 40, 44, 48, 52]
    assert [len(_ffi.FEATURE_TRAIN_SYMBOLS[k][1]) for k in ("bh_train_set_features", "bh_refine_carry_rows")] == [3, 5]
    # what the earlier headers declare is what they declared before
    feats, _ = _declared(os.path.join(ROOT, "include", "brush_hip_features.h"))
    assert feats == set(_ffi.FEATURE_SYMBOLS) == FEATURE_NAMES and not (feats & declared)
    base, _ = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    assert len(_ffi.SYMBOLS) == 82 and base == set(_ffi.SYMBOLS) | {"bh_debug_fill_train_scratch"} and not (base & declared)
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
    lib = _ffi.load()
    for name in NAMES:
        assert getattr(lib, name) is not None
    # the option list is what it was: no key was added
    names = [lib.bh_option_name(i).decode() for i in range(lib.bh_option_count())]
    assert names[-1] == "feature_chunk" and not [k for k in names if "carry" in k or "feature_t" in k], names


def test_hpp_and_host_mirrors_exist():
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_feature_train.h"' in hpp
    for name in ("struct FeatureField {", "inline void train_set_features(", "inline void refine_carry_rows(", "FeatureField* feature_field = nullptr",
                 "BH_CARRY_COPY == 0u && BH_CARRY_ZERO_SPLIT == 1u && BH_CARRY_MAX_CHANNELS == 4096u"):
        assert name in hpp, name
    import brush_amd as ba
    for name in ("as_struct", "carry", "gather", "render", "backward", "step"):
        assert hasattr(ba.FeatureField, name), name
    fields = {f.name: f for f in dataclasses.fields(ba.SceneBatch)}
    assert fields["features"].default is None and list(fields)[-1] == "features"
    cfg = ba.TrainConfig()
    assert (cfg.feature_loss_weight, cfg.feature_loss_kind, cfg.feature_loss_from_iter) == (0.0, "l1", 0)
    params = list(inspect.signature(ba.SplatTrainer.__init__).parameters)
    assert params[-1] == "feature_field" and inspect.signature(ba.SplatTrainer.__init__).parameters["feature_field"].default is None
    try:
        ba.SplatTrainer(cfg, partition="tiles", feature_field=object())
    except ValueError as e:
        assert "feature_field" in str(e)
    else:
        raise AssertionError("a feature field was accepted with partition 'tiles'")
    try:
        ba.SplatTrainer(cfg, pose_optimizer=object(), feature_field=object())
    except ValueError as e:
        assert "feature_field" in str(e) and "pose_optimizer" in str(e)
    else:
        raise AssertionError("a feature field was accepted together with a pose optimizer")
    # RenderNode.backward is what it was: the feature cotangent stays last and keeps refusing the other cotangents
    params = list(inspect.signature(ba.RenderNode.backward).parameters)
    assert params[-2:] == ["v_features", "features"], params


def test_entry_points_reject_a_null_context_without_a_device():
    from brush_amd import _ffi
    lib = _ffi.load()
    f, t = _ffi.BhFeatureField(), _ffi.BhFeatureTarget()
    assert lib.bh_train_set_features(None, C.byref(f), C.byref(t)) == -1
    assert lib.bh_train_set_features(None, None, None) == -1
    assert lib.bh_refine_carry_rows(None, None, None, 3, 0) == -1
