"""Sparse TSDF volumes (include/brush_hip_sparse_mesh.h) without a GPU: the header parses as C and as C++, declares exactly the
binding's SPARSE_MESH_SYMBOLS, both libraries export them, _ffi.py and brush_hip.hpp mirror the struct's size and field order,
brush_hip.h keeps its 82 entry points and brush_hip_mesh.h its five, a null context is refused before the device is touched, and the
Python mirror refuses what needs no device."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bh_sptsdf_mark_clear", "bh_sptsdf_mark", "bh_sptsdf_commit", "bh_sptsdf_clear", "bh_sptsdf_integrate", "bh_sptsdf_extract_count", "bh_sptsdf_extract",
         "bh_sptsdf_to_dense"}
FIELDS = ["origin", "voxel_size", "nx", "ny", "nz", "trunc", "max_weight", "n_blocks", "bits", "rank", "keys", "tw", "rgb"]


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def _fields(body):
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
        src.write_text('#include "brush_hip_sparse_mesh.h"\nint main(void) { return (int)sizeof(BhSparseTsdf) - 80 + (int)BH_SPTSDF_BLOCK - 8 + (int)BH_SPTSDF_MAX_DIM - 8192 '
                       '+ (int)BH_SPTSDF_MAX_STEPS - 64 + (int)sizeof(BhTsdfGrid) - 56; }\n')
        exe = str(tmp_path / ("parse_" + ext))
        subprocess.check_call([os.environ.get("CXX", "g++"), "-x", lang, std, "-Wall", "-Werror", "-I" + inc, str(src), "-o", exe])
        assert subprocess.run([exe]).returncode == 0


def test_header_declares_the_binding_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_sparse_mesh.h"))
    assert declared == set(_ffi.SPARSE_MESH_SYMBOLS) == NAMES, declared ^ set(_ffi.SPARSE_MESH_SYMBOLS)
    assert '#include "brush_hip_mesh.h"' in src and re.search(r"#define BH_SPTSDF_BLOCK 8u", src)
    assert (_ffi.SPTSDF_BLOCK, _ffi.SPTSDF_MAX_DIM, _ffi.SPTSDF_MAX_STEPS) == (8, 8192, 64)
    sizes = set(re.findall(r"static_assert\(sizeof\(BhSparseTsdf\) == (\d+)", src, flags=re.I))
    assert sizes == {str(C.sizeof(_ffi.BhSparseTsdf))} == {"80"}
    assert [f[0] for f in _ffi.BhSparseTsdf._fields_] == FIELDS
    assert [getattr(_ffi.BhSparseTsdf, f).offset for f in FIELDS] == [0, 12, 16, 20, 24, 28, 32, 36, 40, 48, 56, 64, 72]
    body = re.search(r"typedef struct BhSparseTsdf \{(.*?)\} BhSparseTsdf;", src, flags=re.S).group(1)
    assert _fields(body) == FIELDS, _fields(body)
    # the other headers keep what they had
    base, _ = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    mesh, _ = _declared(os.path.join(ROOT, "include", "brush_hip_mesh.h"))
    assert len(_ffi.SYMBOLS) == 82 and base == set(_ffi.SYMBOLS) | {"bh_debug_fill_train_scratch"} and len(mesh) == len(_ffi.MESH_SYMBOLS) == 5
    assert not (base & declared) and not (mesh & declared)
    for path in (_ffi.LIB_PATH, _ffi.TEST_HOOKS_LIB_PATH):
        exported = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert re.search(r"\bT %s$" % name, exported, flags=re.M), (path, name)
    lib = _ffi.load()
    for name in NAMES:
        assert getattr(lib, name) is not None
        proto = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len([p for p in proto.split(",") if p.strip()]) == len(_ffi.SPARSE_MESH_SYMBOLS[name][1]), name
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_sparse_mesh.h"' in hpp and "class SparseTsdfVolume" in hpp
    for pin in ("sizeof(BhSparseTsdf) == 80", "offsetof(BhSparseTsdf, n_blocks) == 36", "offsetof(BhSparseTsdf, bits) == 40", "offsetof(BhSparseTsdf, rgb) == 72"):
        assert pin in hpp, pin
    for name in NAMES:
        assert name + "(" in hpp, name
    mk = open(os.path.join(ROOT, "brush_amd", "csrc", "Makefile")).read()
    assert " sparse_tsdf.hip" in mk and mk.count("brush_hip_sparse_mesh.h") == 2 and mk.count(" device_tsdf.h") == 2
    # one copy of the shared device code: tsdf.hip and sparse_tsdf.hip both take it from device_tsdf.h
    csrc = os.path.join(ROOT, "brush_amd", "csrc")
    for unit in ("tsdf.hip", "sparse_tsdf.hip"):
        text = open(os.path.join(csrc, unit)).read()
        # (the fusion rule is reached through the one load / fuse / store around it, tsdf_fuse_at)
        assert '#include "device_tsdf.h"' in text and "TSDF_CASE[16]" not in text and "tsdf_fuse_at<" in text and "tsdf_classify_word(" in text, unit
        assert "tsdf_update_sample<" not in text, unit
    shared = open(os.path.join(csrc, "device_tsdf.h")).read()
    assert shared.count("TSDF_CASE[16]") == 1 and shared.count("tsdf_update_sample<COLOUR>(") == 1


def test_python_mirror_has_the_surface():
    import brush_amd as ba
    for name in ("mark", "mark_clear", "commit", "clear", "integrate", "count", "extract_mesh", "to_ply", "to_dense", "from_bounds", "vol"):
        assert hasattr(ba.SparseTsdfVolume, name), name
    init = inspect.signature(ba.SparseTsdfVolume.__init__).parameters
    assert list(init)[1:4] == ["origin", "voxel_size", "dims"] and init["trunc"].default is None and init["colour"].default is True and init["max_weight"].default == 64
    assert inspect.signature(ba.SparseTsdfVolume.commit).parameters["dilate"].default == 1
    sig = inspect.signature(ba.SparseTsdfVolume.integrate).parameters
    assert list(sig)[1:4] == ["depths", "cameras", "images"] and sig["images"].default is None and sig["depth_max"].default == math.inf
    sig = inspect.signature(ba.fuse_views).parameters
    assert list(sig)[:4] == ["splats", "cameras", "img_size", "volume"] and sig["depth_mode"].default == "expected" and "pass_" in sig


def test_entry_points_reject_a_null_context_without_a_device():
    from brush_amd import _ffi
    lib = _ffi.load()
    vol = _ffi.BhSparseTsdf(voxel_size=1.0, nx=16, ny=16, nz=16, trunc=4.0, max_weight=8.0)
    grid = _ffi.BhTsdfGrid(voxel_size=1.0, nx=4, ny=4, nz=4, trunc=4.0, max_weight=8.0)
    cfg = _ffi.BhTsdfIntegrateConfig(0.0, math.inf, 0.5, 0)
    nv, nt, nb = C.c_uint32(7), C.c_uint32(7), C.c_uint32(7)
    assert lib.bh_sptsdf_mark_clear(None, C.byref(vol)) == -1
    assert lib.bh_sptsdf_mark(None, C.byref(vol), 0, None, None, None, C.byref(cfg)) == -1
    assert lib.bh_sptsdf_commit(None, C.byref(vol), 1, C.byref(nb)) == -1
    assert lib.bh_sptsdf_clear(None, C.byref(vol)) == -1
    assert lib.bh_sptsdf_integrate(None, C.byref(vol), 0, None, None, None, C.byref(cfg)) == -1
    assert lib.bh_sptsdf_extract_count(None, C.byref(vol), C.byref(nv), C.byref(nt)) == -1
    assert lib.bh_sptsdf_extract(None, C.byref(vol), None, None, None, 0, 0, C.byref(nv), C.byref(nt)) == -1
    assert lib.bh_sptsdf_to_dense(None, C.byref(vol), 0, 0, 0, C.byref(grid)) == -1
    assert (nv.value, nt.value, nb.value) == (7, 7, 7)


def test_argument_refusals_that_need_no_device():
    """The Python mirror refuses, before it asks for a device (this machine may have none): dimensions below 2 or above 8192, numbers
    that are not finite and positive, max_weight below 1.  The library refuses the same on the GPU (tests/test_gpu_sparse_mesh.py)."""
    import brush_amd as ba
    for kw in (dict(dims=(1, 16, 16)), dict(dims=(16, 16, 0)), dict(dims=(8193, 16, 16)), dict(dims=(16, 16, 10 ** 6)), dict(dims=(16, 16)), dict(trunc=0.0),
               dict(trunc=-1.0), dict(trunc=math.nan), dict(voxel_size=0.0), dict(voxel_size=math.inf), dict(max_weight=0.5)):
        args = dict(origin=(0.0, 0.0, 0.0), voxel_size=0.1, dims=(16, 16, 16))
        args.update(kw)
        with pytest.raises(ValueError):
            ba.SparseTsdfVolume(**args)
    with pytest.raises(ValueError, match="resolution"):
        ba.SparseTsdfVolume.from_bounds(((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), 1)
    with pytest.raises(ValueError, match="8192"):
        ba.SparseTsdfVolume.from_bounds(((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), 10000)
