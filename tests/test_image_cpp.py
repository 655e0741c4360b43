"""Mask merge and resampling through the C++ host mirror (include/brush_hip.hpp): tests/cpp/test_image.cpp, compiled with the g++
line of tests/cpp/Makefile into a temporary directory.  CPU: it compiles and links; GPU: the hashes of its resize_u8 and
submit_view results equal those of the numpy restatement tests/image_ref.py on the same generated inputs."""
import os
import re
import subprocess

import numpy as np
import pytest

import image_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "test_image")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "brush_amd")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "test_image.cpp"), "-o", exe, "-L" + lib, "-lbrush_hip", "-L/opt/rocm/lib",
                           "-lamdhip64", "-ldl", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _pattern(w, h, c, salt):
    y, x, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    return ((x * 37 + y * 91 + k * 53 + salt + (x * y) % 17) & 255).astype(np.uint8)


def _fnv(b):
    h = 1469598103934665603
    for v in bytes(b):
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def test_cpp_image_program_compiles_and_links(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_cpp_image_program_matches_the_restatement_on_the_gpu(tmp_path):
    exe = _build(tmp_path)
    p = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert "all C++ image checks passed" in p.stdout
    img = _pattern(211, 105, 3, 1)
    for f, name in ((0, ref.LANCZOS3), (1, ref.TRIANGLE)):
        want = _fnv(ref.resize(img, 100, 50, name).tobytes())
        assert re.search(r"^resize filter=%d %s$" % (f, want), p.stdout, flags=re.M), (name, want)
    packed, _ = ref.load_view(_pattern(160, 120, 4, 2), _pattern(61, 47, 1, 3)[:, :, 0], invert=True, max_resolution=100, premultiply=True)
    assert packed.shape == (75, 100)
    assert re.search(r"^view 100x75 %s$" % _fnv(packed.astype("<u4").tobytes()), p.stdout, flags=re.M)
