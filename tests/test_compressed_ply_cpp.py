"""Compressed PLY export through the C++ host mirror (include/brush_hip.hpp): tests/cpp/test_compressed_ply.cpp, compiled with the
g++ line of tests/cpp/Makefile into a temporary directory.  CPU: it compiles and links; GPU: the export's size is the restated
72 ceil(n/256) + 16 n + 3K n behind the header, and the file reads back through the header."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "test_compressed_ply")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "brush_amd")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "test_compressed_ply.cpp"), "-o", exe, "-L" + lib, "-lbrush_hip", "-L/opt/rocm/lib",
                           "-lamdhip64", "-ldl", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_compressed_ply_program_compiles_and_links(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_cpp_compressed_ply_program_passes_on_the_gpu(tmp_path):
    exe = _build(tmp_path)
    p = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert "ok round_trip n=5000 d=4" in p.stdout and "all C++ compressed PLY checks passed" in p.stdout
