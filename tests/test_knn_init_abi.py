"""Point-cloud initialisation (brush-train/src/splat_init.rs:179-242) without a GPU: the two C-ABI entry points are declared,
bound and exported; bh_ply_vertex_has_property (host code) answers has_property("scale_0") the way import.rs:332 needs it; the C++
program tests/cpp/test_knn.cpp compiles and links against the header's wrappers; and tests/knn_ref.py — the reference
tests/test_gpu_knn_init.py holds the device to — agrees with a literal restatement of the reference's query (all distances of a
point, itself included, sorted, the first one skipped: `nn(p).skip(1)`)."""
import os
import re
import subprocess

import numpy as np
import pytest

import knn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNN_SYMBOLS = ("bh_knn_log_scales", "bh_ply_vertex_has_property")


def test_symbols_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "brush_hip.h")).read(), flags=re.S)
    lib = _ffi.load()
    for name in KNN_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _ffi.SYMBOLS
        assert getattr(lib, name) is not None
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    for name in ("knn_log_scales", "to_init_splats", "load_init_splats"):
        assert re.search(r"inline [\w:<>, ]+ %s\(" % name, hpp), name
    import brush_amd as ba
    for name in ("knn_log_scales", "to_init_splats", "load_init_splats"):
        assert callable(getattr(ba, name))


def _has(data, name):
    from brush_amd import _ffi
    return _ffi.load().bh_ply_vertex_has_property(data, len(data), name.encode())


def test_has_property_on_plain_points_and_splat_files():
    from oracle import ply
    pts = knn_ref.points_ply(knn_ref.cloud("uniform", 50), rgb=np.zeros((50, 3), np.uint8))
    assert _has(pts, "scale_0") == 0 and _has(pts, "x") == 1 and _has(pts, "red") == 1 and _has(pts, "rot_0") == 0
    assert _has(pts, "scale") == 0 and _has(pts, "") == 0
    rng = np.random.default_rng(1)
    full = ply.splat_to_ply(rng.normal(size=(7, 10)).astype(np.float32), rng.normal(size=(7, 4, 3)).astype(np.float32),
                            rng.normal(size=7).astype(np.float32))
    for nm in ("x", "scale_0", "scale_2", "opacity", "rot_3", "f_dc_0", "f_rest_8"):
        assert _has(full, nm) == 1, nm
    assert _has(full, "f_rest_9") == 0 and _has(full, "red") == 0
    # a property of another element does not count
    other = pts.replace(b"end_header\n", b"element face 0\nproperty float scale_0\nend_header\n")
    assert _has(other, "scale_0") == 0 and _has(other, "x") == 1


def test_has_property_on_a_compressed_file():
    from oracle import ply
    data = ply.make_compressed_ply(600, 1, seed=2)
    assert _has(data, "scale_0") == 1   # compressed files always have scales
    assert _has(data, "packed_position") == 1 and _has(data, "x") == 1 and _has(data, "rot_0") == 1
    assert _has(data, "f_rest_8") == 1 and _has(data, "f_rest_9") == 0 and _has(data, "red") == 0
    assert _has(ply.make_compressed_ply(300, 0, seed=3), "f_rest_0") == 0


def test_has_property_rejects_a_malformed_header():
    pts = knn_ref.points_ply(knn_ref.cloud("uniform", 10))
    assert _has(b"not a ply at all", "scale_0") < 0
    assert _has(pts.replace(b"end_header", b"end_headex"), "x") < 0              # no header end
    assert _has(pts[:-5], "x") < 0                                                # body shorter than the header says
    assert _has(pts.replace(b"binary_little_endian", b"ascii"), "x") < 0          # only binary little endian is read
    import brush_amd as ba
    with pytest.raises(ba.BrushHipError):
        ba.ply_vertex_has_property(b"ply\nformat ascii 1.0\nend_header\n", "x")
    assert ba.ply_vertex_has_property(pts, "x") and not ba.ply_vertex_has_property(pts, "scale_0")


def build_knn_cpp(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "test_knn")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "brush_amd")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "test_knn.cpp"), "-o", exe, "-L" + lib, "-lbrush_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-ldl", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_knn_program_compiles_and_links(tmp_path):
    assert os.path.exists(build_knn_cpp(tmp_path))


def _literal_reference(pos):
    """compute_knn_scales as the reference writes it, one point at a time: every finite point's distances (itself included) in
    f32, sorted, skip(1), a1 a2; ln of the clamp in float64 then f32.  Non-finite rows: +inf neighbours (this library's rule)."""
    pos = np.asarray(pos, np.float32)
    n = pos.shape[0]
    fin = knn_ref.finite_rows(pos)
    nn = np.full((n, 2), np.inf, np.float32)
    for i in range(n):
        if not fin[i]:
            continue
        d = sorted(float(np.sqrt(knn_ref.sq_dist_f32(pos[i], pos[j]))) for j in range(n) if fin[j])
        rest = d[1:] + [np.inf, np.inf]
        nn[i] = (rest[0], rest[1])
    return nn


@pytest.mark.parametrize("kind", knn_ref.KINDS)
def test_numpy_reference_matches_the_literal_query(kind):
    pos = knn_ref.cloud(kind, 150 if kind != "tripled" else 160, seed=5)
    lit = _literal_reference(pos)
    nn = knn_ref.nn2_brute(pos, chunk=37)
    assert np.array_equal(nn, lit)
    ls = knn_ref.log_scales(pos, nn)
    upper = knn_ref.median_size(pos) * np.float32(0.1)
    fin = knn_ref.finite_rows(pos)
    assert np.all(ls <= np.log(np.float64(upper)) + 1e-6) and np.all(ls >= np.log(1e-3) - 1e-6)
    assert np.all(ls[~fin] == np.float32(np.log(np.float64(upper))))
    if kind == "tiny":
        assert knn_ref.median_size(pos) == np.float32(0.01) and np.all(ls == np.float32(np.log(np.float64(np.float32(1e-3)))))
    if kind == "tripled":
        assert np.all(nn[fin][:, 0] == 0.0)   # every point has a duplicate


def test_numpy_reference_small_counts():
    for n in range(0, 3):
        assert np.array_equal(knn_ref.log_scales(knn_ref.cloud("uniform", 3)[:n]), np.zeros(n, np.float32))
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32)
    nn = knn_ref.nn2_brute(pos)
    assert np.array_equal(nn, np.array([[1, 2], [1, np.sqrt(np.float32(5))], [2, np.sqrt(np.float32(5))]], np.float32))
    allbad = np.full((5, 3), np.nan, np.float32)
    ls = knn_ref.log_scales(allbad)
    assert np.all(ls == np.float32(np.log(0.2)))   # unit-box fallback: median_size 2, upper 0.2


def test_ulp_helper():
    a = np.array([1.0, -2.0, np.inf, 0.0], np.float32)
    b = np.nextafter(a, np.float32(10))
    assert list(knn_ref.ulp_diff(a, a)) == [0, 0, 0, 0]
    assert list(knn_ref.ulp_diff(a[:2], b[:2])) == [1, 1]
