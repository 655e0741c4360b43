"""Distortion maps (include/brush_hip_distortion.h) without a GPU: the header declares exactly the binding's DISTORTION_SYMBOLS and
parses as C and as C++, the library exports them, _ffi.py and brush_hip.hpp mirror the structs' sizes and field order, the older
headers declare what they declared before (brush_hip.h its 82 entry points), and argument checks run before the device is touched."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bh_render_distortion", "bh_render_distortion_moments", "bh_render_backward_distortion_saved", "bh_distortion_loss", "bh_train_set_distortion"}


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def test_header_parses_as_c_and_as_cpp(tmp_path):
    inc = os.path.join(ROOT, "include")
    for lang, std, ext in (("c", "-std=c11", "c"), ("c++", "-std=c++17", "cpp")):
        src = tmp_path / ("parse." + ext)
        src.write_text('#include "brush_hip_distortion.h"\nint main(void) { return (int)sizeof(BhDistortionConfig) + (int)sizeof(BhDistortionTermConfig) - 32; }\n')
        exe = str(tmp_path / ("parse_" + ext))
        subprocess.check_call([os.environ.get("CXX", "g++"), "-x", lang, std, "-Wall", "-Werror", "-I" + inc, str(src), "-o", exe])
        assert subprocess.run([exe]).returncode == 0


def test_header_declares_the_binding_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_distortion.h"))
    assert declared == set(_ffi.DISTORTION_SYMBOLS) == NAMES, declared ^ set(_ffi.DISTORTION_SYMBOLS)
    assert '#include "brush_hip_depth.h"' in src and '#include "brush_hip_normal.h"' in src
    assert re.search(r"#define BH_DISTORTION_Z 0u", src) and re.search(r"#define BH_DISTORTION_NDC 1u", src)
    assert (_ffi.DISTORTION_Z, _ffi.DISTORTION_NDC) == (0, 1)
    # the structs: the header pins their sizes with a static_assert, the mirrors have the same size and field order
    for name, mirror, fields in (("BhDistortionConfig", _ffi.BhDistortionConfig, ["kind", "near_z", "far_z", "reserved"]),
                                ("BhDistortionTermConfig", _ffi.BhDistortionTermConfig, ["weight", "kind", "near_z", "far_z"])):
        sizes = set(re.findall(r"static_assert\(sizeof\(%s\) == (\d+)" % name, src, flags=re.I))
        assert sizes == {str(C.sizeof(mirror))} == {"16"}, (name, sizes)
        assert [f[0] for f in mirror._fields_] == fields
        assert [getattr(mirror, f).offset for f in fields] == [0, 4, 8, 12]
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
        assert re.findall(r"\b(\w+);", body) == fields, (name, body)
    # the older headers declare what they declared before
    base, _ = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    depth, _ = _declared(os.path.join(ROOT, "include", "brush_hip_depth.h"))
    normal, _ = _declared(os.path.join(ROOT, "include", "brush_hip_normal.h"))
    normal_loss, _ = _declared(os.path.join(ROOT, "include", "brush_hip_normal_loss.h"))
    # (82 entry points; the header also names the test-hooks build's bh_debug_fill_train_scratch)
    assert len(_ffi.SYMBOLS) == 82 and base == set(_ffi.SYMBOLS) | {"bh_debug_fill_train_scratch"} and not (base & declared)
    assert depth == set(_ffi.DEPTH_SYMBOLS) and not (depth & declared)
    assert normal == set(_ffi.NORMAL_SYMBOLS) and len(normal) == 5 and not (normal & declared)
    assert normal_loss == set(_ffi.NORMAL_LOSS_SYMBOLS) and len(normal_loss) == 2 and not (normal_loss & declared)
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
    lib = _ffi.load()
    for name in NAMES:
        assert getattr(lib, name) is not None
    assert [len(_ffi.DISTORTION_SYMBOLS[k][1]) for k in ("bh_render_distortion", "bh_render_distortion_moments", "bh_render_backward_distortion_saved",
                                                         "bh_distortion_loss", "bh_train_set_distortion")] == [4, 4, 16, 7, 2]
    # every parameter the header names is one the mirror passes
    for name in NAMES:
        proto = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len([p for p in proto.split(",") if p.strip()]) == len(_ffi.DISTORTION_SYMBOLS[name][1]), name
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_distortion.h"' in hpp
    for name in ("DeviceBuffer<float> distortion(", "backward_distortion(", "distortion_loss(", "train_set_distortion(", "bh_train_set_distortion(",
                 "sizeof(BhDistortionConfig) == 16", "sizeof(BhDistortionTermConfig) == 16"):
        assert name in hpp, name
    import brush_amd as ba
    assert hasattr(ba, "render_distortion") and hasattr(ba, "distortion_loss") and hasattr(ba.RenderNode, "distortion")
    cfg = ba.TrainConfig()
    assert cfg.distortion_loss_weight == 0.0 and cfg.distortion_loss_from_iter == 0 and cfg.distortion_kind == "z"
    assert 0.0 < cfg.distortion_near < cfg.distortion_far
    mk = open(os.path.join(ROOT, "brush_amd", "csrc", "Makefile")).read()
    assert " distortion.hip" in mk and mk.count("brush_hip_distortion.h") == 2


def test_entry_points_reject_a_null_context_without_a_device():
    from brush_amd import _ffi
    lib = _ffi.load()
    cfg = _ffi.BhDistortionConfig(kind=0)
    term = _ffi.BhDistortionTermConfig(weight=0.5)
    out = _ffi.BhRenderOut()
    assert lib.bh_render_distortion(None, C.byref(out), C.byref(cfg), None) == -1
    assert lib.bh_render_distortion_moments(None, C.byref(out), C.byref(cfg), None) == -1
    assert lib.bh_render_backward_distortion_saved(None, C.byref(out), None, None, 0, None, 0, None, C.byref(cfg), None, None, None, None, None, None, None) == -1
    assert lib.bh_distortion_loss(None, None, 4, 4, 1, 1.0, None) == -1
    assert lib.bh_train_set_distortion(None, C.byref(term)) == -1 and lib.bh_train_set_distortion(None, None) == -1
