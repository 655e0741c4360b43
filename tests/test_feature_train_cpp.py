"""Feature fields trained with the splats through the C++ host mirror (include/brush_hip.hpp FeatureField / train_set_features /
refine_carry_rows / SplatTrainer::refine with a field): tests/cpp/test_feature_train.cpp, compiled with the g++ line of
tests/cpp/Makefile into a temporary directory.  CPU: it compiles and links; GPU: one step with the term against the hand-composed
loss, bit for bit, and the carry pinned to what refine does to the splats' own SH rows."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "test_feature_train")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "brush_amd")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "test_feature_train.cpp"), "-o", exe, "-L" + lib, "-lbrush_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-ldl", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_feature_train_program_compiles_and_links(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_cpp_feature_train_program_passes_on_the_gpu(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "ok feature train step" in r.stdout and "ok refine carry" in r.stdout
    assert "all C++ feature-train checks passed" in r.stdout
