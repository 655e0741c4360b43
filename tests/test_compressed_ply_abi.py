"""Compressed PLY export (include/brush_hip_compressed_ply.h) without a GPU: the header declares exactly the binding's
COMPRESSED_PLY_SYMBOLS and the library exports them, the Python and C++ mirrors exist, and the numpy restatement
tests/compressed_ply_ref.py writes files the library's header parser and oracle/ply.load_compressed_ply accept, whose decoded rows lie
within the quantisation bounds of DESIGN.md §6g."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import compressed_ply_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def test_header_declares_the_binding_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_compressed_ply.h"))
    assert declared == set(_ffi.COMPRESSED_PLY_SYMBOLS), declared ^ set(_ffi.COMPRESSED_PLY_SYMBOLS)
    assert '#include "brush_hip.h"' in src
    base, _ = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    assert not (base & declared) and not (set(_ffi.SYMBOLS) & declared) and not (set(_ffi.LPIPS_SYMBOLS) & declared)
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in _ffi.COMPRESSED_PLY_SYMBOLS:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
    lib = _ffi.load()
    for name in _ffi.COMPRESSED_PLY_SYMBOLS:
        assert getattr(lib, name) is not None
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_compressed_ply.h"' in hpp and "splat_to_compressed_ply(" in hpp
    import brush_amd as ba
    assert callable(ba.splat_to_compressed_ply)


def test_entry_point_rejects_a_missing_context():
    from brush_amd import _ffi
    lib = _ffi.load()
    need = C.c_uint64(0)
    assert lib.bh_splat_to_compressed_ply(None, None, None, None, None, 0, 0, 0, None, None, None, 0, C.byref(need)) == -1


@pytest.mark.parametrize("n,d", [(1, 0), (255, 1), (256, 2), (257, 3), (4097, 4), (3000, 0)])
def test_restated_files_parse_and_round_trip_within_bounds(n, d):
    from brush_amd import _ffi
    t, sh, o = ref.random_scene(n, d, seed=n + d)
    up = (0.0, -1.0, 0.25) if n % 2 else None
    data, order = ref.compressed_ply(t, sh, o, render_mip=bool(d % 2), up_axis=up, return_order=True)
    assert len(data) == len(ref.header(n, d, bool(d % 2), up)) + ref.body_size(n, d)
    assert sorted(order.tolist()) == list(range(n))
    info = _ffi.BhPlyInfo()
    assert _ffi.load().bh_ply_parse_header(data, len(data), C.byref(info)) == 0
    assert info.compressed == 1 and info.num_splats == n and info.sh_degree == d and info.render_mode == d % 2
    assert info.has_up_axis == 1
    assert tuple(info.up_axis) == ((0.0, -1.0, 0.25) if up else (0.0, -1.0, 0.0))
    bad = ref.round_trip_violations(data, order, t, sh, o)
    assert not any(bad.values()), bad


@pytest.mark.parametrize("d", [0, 1, 4])
def test_restated_edge_rows_round_trip_within_bounds(d):
    t, sh, o = ref.edge_scene(d)
    data, order = ref.compressed_ply(t, sh, o, return_order=True)
    assert sorted(order[:256].tolist()) == list(range(256))      # the degenerate chunk is chunk 0
    cr = ref.chunk_rows(data)
    assert np.array_equal(cr[0, 0:3], cr[0, 3:6]) and np.array_equal(cr[0, 6:9], cr[0, 9:12])
    assert np.isfinite(cr).all() and not np.signbit(cr[cr == 0]).any()   # ranges over finite values, +0 only
    bad = ref.round_trip_violations(data, order, t, sh, o)
    assert not any(bad.values()), bad


def test_restated_words_follow_the_formulas():
    # unorm, rotation and SH bytes on hand-picked values
    assert ref.unorm(np.array([0.0, 1.0, 0.5, -0.0, -1e-9, np.nan, np.inf, 2.0], np.float32), 8).tolist() == [0, 255, 128, 0, 0, 0, 255, 255]
    assert ref.sh_bytes(np.array([-4.0, 0.0, 3.96875, 4.0, np.nan, -np.inf, np.inf, -3.99], np.float32)).tolist() == [0, 128, 255, 255, 0, 0, 255, 0]
    w = ref.rotation_words(np.array([[1, 0, 0, 0], [0, 0, 0, 0], [0.1, -0.9, 0.2, 0.3], [0.5, -0.5, 0.5, -0.5]], np.float32))
    assert (w >> 30).tolist() == [0, 0, 1, 0]
    assert [(int(x) >> 20) & 0x3FF for x in w[:2]] == [512, 512]   # 0 * 0.7071 + 0.5 -> 511.5 + 0.5 = 512
    # Morton keys: the box corners, NaN -> cell 0, +inf -> cell 1023
    k = ref.morton_keys(np.array([[0, 0, 0], [1, 1, 1], [np.nan, np.inf, 0.5], [1, 0, 0]], np.float32))
    assert k[0] == 0 and k[1] == (1 << 30) - 1 and k[3] == ref.part1by2(np.uint32(1023))
    assert k[2] == (ref.part1by2(np.uint32(512)) << np.uint32(2)) | (ref.part1by2(np.uint32(1023)) << np.uint32(1))


def test_empty_export_is_a_header_with_zero_counts():
    from brush_amd import _ffi
    for d in (0, 2):
        data = ref.compressed_ply(np.zeros((0, 10), np.float32), np.zeros((0, (d + 1) ** 2, 3), np.float32), np.zeros(0, np.float32))
        assert b"element chunk 0\n" in data and b"element vertex 0\n" in data and data.endswith(b"end_header\n")
        assert (b"element sh 0\n" in data) == (d > 0)
        info = _ffi.BhPlyInfo()
        assert _ffi.load().bh_ply_parse_header(data, len(data), C.byref(info)) == 0
        assert info.compressed == 1 and info.num_splats == 0 and info.sh_degree == d
