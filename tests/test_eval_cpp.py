"""Held-out evaluation through the C++ host mirror (include/brush_hip.hpp): tests/cpp/test_eval.cpp, compiled with the g++ line of
tests/cpp/Makefile into a temporary directory.  CPU: it compiles and links; GPU: eval_metrics, eval_stats and run_eval agree with a
host restatement, with render + metrics and with each other."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "test_eval")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "brush_amd")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "test_eval.cpp"), "-o", exe, "-L" + lib, "-lbrush_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-ldl", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_eval_program_compiles_and_links(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_cpp_eval_program_passes_on_the_gpu(tmp_path):
    exe = _build(tmp_path)
    p = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert "ok eval_metrics" in p.stdout and "ok eval_view" in p.stdout and "ok run_eval" in p.stdout and "all C++ eval checks passed" in p.stdout
