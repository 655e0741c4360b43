"""Mask lifting through the C++ host mirror (include/brush_hip.hpp LiftAccumulator / compact_splats): tests/cpp/test_lift.cpp,
compiled with the g++ line of tests/cpp/Makefile into a temporary directory.  CPU: it compiles and links; GPU: one view accumulated
through the mirror against a loop over RenderNode::features weights, assign / select / compact_splats against loops, the refusals."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "test_lift")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "brush_amd")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "test_lift.cpp"), "-o", exe, "-L" + lib, "-lbrush_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-ldl", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_lift_program_compiles_and_links(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_cpp_lift_program_passes_on_the_gpu(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "ok lift accumulate" in r.stdout and "ok lift assign select compact" in r.stdout and "ok lift refusals" in r.stdout
    assert "all C++ lift checks passed" in r.stdout
