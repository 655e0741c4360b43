"""Mesh extraction (include/brush_hip_mesh.h) without a GPU: the header parses as C and as C++, declares exactly the binding's
MESH_SYMBOLS, both libraries export them, _ffi.py and brush_hip.hpp mirror the structs' sizes and field order, brush_hip.h keeps its
82 entry points, a null context is refused before the device is touched, and the Python mirror refuses what needs no device."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bh_tsdf_clear", "bh_tsdf_integrate", "bh_tsdf_extract_count", "bh_tsdf_extract", "bh_mesh_to_ply"}


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def _fields(body):
    """Field names of a struct body, in order: `float origin[3];` and `uint32_t nx, ny, nz;` included."""
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names = decl.split(None, 1)[1] if "*" not in decl else decl.split("*", 1)[1]
            out += [re.match(r"\w+", n.strip()).group(0) for n in names.split(",")]
    return out


def test_header_parses_as_c_and_as_cpp(tmp_path):
    inc = os.path.join(ROOT, "include")
    for lang, std, ext in (("c", "-std=c11", "c"), ("c++", "-std=c++17", "cpp")):
        src = tmp_path / ("parse." + ext)
        src.write_text('#include "brush_hip_mesh.h"\nint main(void) { return (int)sizeof(BhTsdfGrid) + (int)sizeof(BhTsdfIntegrateConfig) - 72 + (int)BH_TSDF_MAX_BATCH - 8; }\n')
        exe = str(tmp_path / ("parse_" + ext))
        subprocess.check_call([os.environ.get("CXX", "g++"), "-x", lang, std, "-Wall", "-Werror", "-I" + inc, str(src), "-o", exe])
        assert subprocess.run([exe]).returncode == 0


def test_header_declares_the_binding_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_mesh.h"))
    assert declared == set(_ffi.MESH_SYMBOLS) == NAMES, declared ^ set(_ffi.MESH_SYMBOLS)
    assert '#include "brush_hip.h"' in src and re.search(r"#define BH_TSDF_MAX_BATCH 8u", src) and _ffi.TSDF_MAX_BATCH == 8
    for name, mirror, fields, offsets, size in (
            ("BhTsdfGrid", _ffi.BhTsdfGrid, ["origin", "voxel_size", "nx", "ny", "nz", "trunc", "max_weight", "reserved", "tw", "rgb"],
             [0, 12, 16, 20, 24, 28, 32, 36, 40, 48], 56),
            ("BhTsdfIntegrateConfig", _ffi.BhTsdfIntegrateConfig, ["depth_min", "depth_max", "alpha_min", "reserved"], [0, 4, 8, 12], 16)):
        sizes = set(re.findall(r"static_assert\(sizeof\(%s\) == (\d+)" % name, src, flags=re.I))
        assert sizes == {str(C.sizeof(mirror))} == {str(size)}, (name, sizes)
        assert [f[0] for f in mirror._fields_] == fields
        assert [getattr(mirror, f).offset for f in fields] == offsets
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
        assert _fields(body) == fields, (name, _fields(body))
    base, _ = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    assert len(_ffi.SYMBOLS) == 82 and base == set(_ffi.SYMBOLS) | {"bh_debug_fill_train_scratch"} and not (base & declared)
    for path in (_ffi.LIB_PATH, _ffi.TEST_HOOKS_LIB_PATH):
        exported = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert re.search(r"\bT %s$" % name, exported, flags=re.M), (path, name)
    lib = _ffi.load()
    for name in NAMES:
        assert getattr(lib, name) is not None
        proto = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len([p for p in proto.split(",") if p.strip()]) == len(_ffi.MESH_SYMBOLS[name][1]), name
    assert [len(_ffi.MESH_SYMBOLS[k][1]) for k in ("bh_tsdf_clear", "bh_tsdf_integrate", "bh_tsdf_extract_count", "bh_tsdf_extract", "bh_mesh_to_ply")] == [2, 7, 4, 9, 9]
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_mesh.h"' in hpp and "class TsdfVolume" in hpp
    for pin in ("sizeof(BhTsdfGrid) == 56", "offsetof(BhTsdfGrid, tw) == 40", "offsetof(BhTsdfGrid, rgb) == 48", "sizeof(BhTsdfIntegrateConfig) == 16",
                "offsetof(BhTsdfIntegrateConfig, alpha_min) == 8"):
        assert pin in hpp, pin
    for name in NAMES:
        assert name + "(" in hpp, name
    mk = open(os.path.join(ROOT, "brush_amd", "csrc", "Makefile")).read()
    assert " tsdf.hip" in mk and mk.count("brush_hip_mesh.h") == 2


def test_python_mirror_has_the_surface():
    import brush_amd as ba
    for name in ("clear", "integrate", "extract_mesh", "to_ply", "from_bounds", "count", "grid"):
        assert hasattr(ba.TsdfVolume, name), name
    init = inspect.signature(ba.TsdfVolume.__init__).parameters
    assert list(init)[1:4] == ["origin", "voxel_size", "dims"] and init["trunc"].default is None and init["colour"].default is True
    assert init["max_weight"].default >= 1.0
    sig = inspect.signature(ba.TsdfVolume.integrate).parameters
    assert list(sig)[1:4] == ["depths", "cameras", "images"] and sig["images"].default is None
    assert sig["depth_max"].default == math.inf and sig["alpha_min"].default == 0.5
    sig = inspect.signature(ba.fuse_views).parameters
    assert list(sig)[:4] == ["splats", "cameras", "img_size", "volume"] and sig["depth_mode"].default == "expected" and "pass_" in sig
    assert callable(ba.mesh_to_ply)


def test_entry_points_reject_a_null_context_without_a_device():
    from brush_amd import _ffi
    lib = _ffi.load()
    grid = _ffi.BhTsdfGrid(voxel_size=1.0, nx=4, ny=4, nz=4, trunc=4.0, max_weight=8.0)
    cfg = _ffi.BhTsdfIntegrateConfig(0.0, math.inf, 0.5, 0)
    nv, nt, size = C.c_uint32(7), C.c_uint32(7), C.c_uint64(7)
    assert lib.bh_tsdf_clear(None, C.byref(grid)) == -1
    assert lib.bh_tsdf_integrate(None, C.byref(grid), 0, None, None, None, C.byref(cfg)) == -1
    assert lib.bh_tsdf_extract_count(None, C.byref(grid), C.byref(nv), C.byref(nt)) == -1
    assert lib.bh_tsdf_extract(None, C.byref(grid), None, None, None, 0, 0, C.byref(nv), C.byref(nt)) == -1
    assert lib.bh_mesh_to_ply(None, None, None, 0, None, 0, None, 0, C.byref(size)) == -1
    assert (nv.value, nt.value, size.value) == (7, 7, 7)


def test_argument_refusals_that_need_no_device():
    """The Python mirror refuses, before it asks for a device (this machine may have none): dimensions below 2, more than 2^31 - 1
    samples, trunc <= 0, a lens model other than the pinhole, a tile-row window, a camera of another size than its depth map.  The
    library refuses the same on the GPU (tests/test_gpu_mesh.py)."""
    import brush_amd as ba
    for kw in (dict(dims=(1, 4, 4)), dict(dims=(4, 4, 0)), dict(dims=(2048, 1024, 1024)), dict(dims=(4, 4, 4), trunc=0.0), dict(dims=(4, 4, 4), trunc=-1.0),
               dict(dims=(4, 4, 4), trunc=math.nan), dict(dims=(4, 4, 4), voxel_size=0.0), dict(dims=(4, 4, 4), max_weight=0.5)):
        args = dict(origin=(0.0, 0.0, 0.0), voxel_size=0.1)
        args.update(kw)
        with pytest.raises(ValueError):
            ba.TsdfVolume(**args)
    assert 2048 * 1024 * 1024 == 2 ** 31   # one more than the limit
    pin = ba.Camera(fov_x=1.0, fov_y=0.8)
    cams = ba.TsdfVolume.check_views([pin, pin], [(30, 40), (30, 40)])
    assert len(cams) == 2 and (cams[1].img_w, cams[1].img_h, cams[1].model) == (40, 30, 0)
    with pytest.raises(ValueError, match="pinhole"):
        ba.TsdfVolume.check_views([pin, ba.Camera(fov_x=1.0, fov_y=0.8, camera_model="kb4", dist=(0.01, 0.0, 0.0, 0.0))], [(30, 40), (30, 40)])
    with pytest.raises(ValueError, match="tile-row"):
        ba.TsdfVolume.check_views([pin.uniforms((40, 32), tile_rows=(0, 1))], [(32, 40)])
    with pytest.raises(ValueError, match="its depth map"):
        ba.TsdfVolume.check_views([pin.uniforms((40, 32))], [(30, 40)])
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        ba.TsdfVolume.check_views([pin], [(30, 40, 1)])
