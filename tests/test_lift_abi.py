"""Mask lifting (include/brush_hip_lift.h) without a GPU: the header declares exactly the binding's LIFT_SYMBOLS and parses as C and as
C++, the library exports them, _ffi.py mirrors BhLiftSelect's size, field order and offsets and the header's constants, brush_hip.h
declares what it declared before (its 82 entry points, the same ABI version), brush_hip.hpp includes the header and names the
mirrors, brush_amd exports the new names, and argument checks run before the device is touched."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bh_lift_accumulate", "bh_lift_assign", "bh_lift_select"}
SELECT_FIELDS = [("label", 0), ("min_share", 4), ("min_weight", 8), ("min_max_weight", 12), ("min_pixels", 16), ("invert", 20)]


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def _lib():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    return _ffi.load(), _ffi


def test_header_parses_as_c_and_as_cpp(tmp_path):
    inc = os.path.join(ROOT, "include")
    for lang, std, ext in (("c", "-std=c11", "c"), ("c++", "-std=c++17", "cpp")):
        src = tmp_path / ("parse." + ext)
        src.write_text('#include "brush_hip_lift.h"\nint main(void) { return (int)sizeof(BhLiftSelect) - 24 + (BH_LIFT_ANY_LABEL != 0xFFFFFFFFu); }\n')
        exe = str(tmp_path / ("parse_" + ext))
        subprocess.check_call([os.environ.get("CXX", "g++"), "-x", lang, std, "-Wall", "-Werror", "-I" + inc, str(src), "-o", exe])
        assert subprocess.run([exe]).returncode == 0


def test_header_declares_the_binding_and_the_library_exports_it():
    lib, _ffi = _lib()
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_lift.h"))
    assert declared == set(_ffi.LIFT_SYMBOLS) == NAMES, declared ^ set(_ffi.LIFT_SYMBOLS)
    assert '#include "brush_hip.h"' in src
    assert re.findall(r"#define\s+BH_LIFT_MAX_LABELS\s+(\d+)u", src) == ["256"] and _ffi.LIFT_MAX_LABELS == 256
    assert re.findall(r"#define\s+BH_LIFT_UNASSIGNED\s+(\d+)u", src) == ["255"] and _ffi.LIFT_UNASSIGNED == 255
    assert re.findall(r"#define\s+BH_LIFT_IGNORE_LABEL\s+(\d+)u", src) == ["255"]
    assert re.findall(r"#define\s+BH_LIFT_ANY_LABEL\s+(0x[0-9A-F]+)u", src) == ["0xFFFFFFFF"] and _ffi.LIFT_ANY_LABEL == 0xFFFFFFFF
    assert re.findall(r"#define\s+BH_LIFT_VOTE_ONE\s+([0-9.]+)f", src) == ["16777216.0"] and _ffi.LIFT_VOTE_ONE == 2.0 ** 24
    # the struct: the header pins its size with a static_assert (C and C++), the mirror has the same size, field order and offsets
    sizes = re.findall(r"static_assert\(sizeof\(BhLiftSelect\) == (\d+)", src, flags=re.I)
    assert len(sizes) == 2 and set(sizes) == {str(C.sizeof(_ffi.BhLiftSelect))} == {"24"}, sizes
    body = re.search(r"typedef struct BhLiftSelect \{(.*?)\} BhLiftSelect;", src, flags=re.S).group(1)
    assert re.findall(r"\b(?:uint32_t|float)\s+(\w+);", body) == [f for f, _ in SELECT_FIELDS], body
    assert [f[0] for f in _ffi.BhLiftSelect._fields_] == [f for f, _ in SELECT_FIELDS]
    assert [getattr(_ffi.BhLiftSelect, f).offset for f, _ in SELECT_FIELDS] == [o for _, o in SELECT_FIELDS]
    # brush_hip.h declares what it declared before (82 entry points and the test-hooks build's bh_debug_fill_train_scratch), same ABI version
    base, base_src = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    assert len(_ffi.SYMBOLS) == 82 and base == set(_ffi.SYMBOLS) | {"bh_debug_fill_train_scratch"} and not (base & declared)
    assert re.findall(r"#define\s+BH_ABI_VERSION\s+(\d+)", base_src) == [str(_ffi.ABI_VERSION)] == ["7"] and lib.bh_abi_version() == 7
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
        assert getattr(lib, name) is not None
        proto = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len([p for p in proto.split(",") if p.strip()]) == len(_ffi.LIFT_SYMBOLS[name][1]), name
    assert [len(_ffi.LIFT_SYMBOLS[k][1]) for k in ("bh_lift_accumulate", "bh_lift_assign", "bh_lift_select")] == [7, 7, 8]
    # no option was added for it
    assert not [i for i in range(lib.bh_option_count()) if b"lift" in lib.bh_option_name(i)]
    mk = open(os.path.join(ROOT, "brush_amd", "csrc", "Makefile")).read()
    assert " lift.hip" in mk and mk.count("brush_hip_lift.h") == 2


def test_the_other_mirrors_carry_the_names():
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_lift.h"' in hpp
    for name in ("class LiftAccumulator", "void add(const RenderNode& node, const uint8_t* labels)", "bh_lift_accumulate(", "bh_lift_assign(", "bh_lift_select(",
                 "inline Splats compact_splats(", "sizeof(BhLiftSelect) == 24", "BH_LIFT_MAX_LABELS == 256u"):
        assert name in hpp, name
    import brush_amd as ba
    for name in ("LiftAccumulator", "lift_labels", "compact_splats"):
        assert hasattr(ba, name), name
    for name in ("add", "weights", "assign", "select", "clear"):
        assert hasattr(ba.LiftAccumulator, name), name
    assert list(inspect.signature(ba.LiftAccumulator.select).parameters)[1:] == ["label", "min_share", "min_weight", "min_max_weight", "min_pixels", "invert"]
    assert list(inspect.signature(ba.lift_labels).parameters)[:6] == ["splats", "views", "num_labels", "img_size", "pass_", "ctx"]
    assert list(inspect.signature(ba.compact_splats).parameters)[:3] == ["splats", "keep", "return_indices"]
    # crop_splats is what it was: select, count, decimate_to_count
    src = inspect.getsource(ba.crop_splats)
    assert "select_region(splats, region, ctx=ctx, return_count=True)" in src and "decimate_to_count(splats, keep, count" in src and "compact_splats" not in src


def test_entry_points_reject_a_null_context_without_a_device():
    lib, _ffi = _lib()
    out = _ffi.BhRenderOut()
    sel = _ffi.BhLiftSelect(label=_ffi.LIFT_ANY_LABEL)
    assert lib.bh_lift_accumulate(None, C.byref(out), None, 2, None, None, None) == -1
    assert lib.bh_lift_assign(None, None, 4, 2, 0.0, None, None) == -1
    assert lib.bh_lift_select(None, None, None, None, 4, 2, C.byref(sel), None) == -1
