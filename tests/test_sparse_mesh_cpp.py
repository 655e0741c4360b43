"""Sparse TSDF volumes through the C++ host mirror (include/brush_hip.hpp SparseTsdfVolume): tests/cpp/test_sparse_mesh.cpp, compiled
with the g++ line of tests/cpp/Makefile into a temporary directory.  CPU: it compiles, links and passes its host checks (the program
stops there without a device); GPU: the whole program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "test_sparse_mesh")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "brush_amd")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "test_sparse_mesh.cpp"), "-o", exe, "-L" + lib, "-lbrush_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-ldl", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_sparse_mesh_program_compiles_and_passes_its_host_checks(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "ok sparse mesh host checks" in r.stdout


@pytest.mark.gpu
def test_cpp_sparse_mesh_program_passes_on_the_gpu(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    for line in ("ok sparse mesh host checks", "ok sparse mesh sphere", "ok sparse mesh ply", "ok sparse mesh integrate", "ok sparse mesh refusals",
                 "all C++ sparse mesh checks passed"):
        assert line in r.stdout, line
