"""LPIPS through the C++ host mirror (include/brush_hip.hpp): tests/cpp/test_lpips.cpp, compiled with the g++ line of
tests/cpp/Makefile into a temporary directory.  CPU: it compiles and links; GPU: it runs on inputs written here and its value and
dL/dimg equal the Python binding's, bit for bit."""
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "test_lpips")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "brush_amd")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "test_lpips.cpp"), "-o", exe, "-L" + lib, "-lbrush_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-ldl", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_lpips_program_compiles_and_links(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_cpp_lpips_program_agrees_with_python(tmp_path, dev):
    import brush_amd as ba
    import lpips_ref
    exe = _build(tmp_path)
    h, w, bg = 48, 40, (0.2, 0.4, 0.6)
    rng = np.random.default_rng(12)
    flat = ba.Lpips.random_params(seed=8)
    img = rng.uniform(0, 1, (h, w, 4)).astype(np.float32)
    b = rng.integers(0, 256, (h, w, 4)).astype(np.uint32)
    gt = lpips_ref.pack_rgba8(b[..., 0], b[..., 1], b[..., 2], b[..., 3])
    d = tmp_path
    flat.tofile(str(d / "params.f32"))
    img.tofile(str(d / "img.f32"))
    gt.tofile(str(d / "gt.u32"))
    (d / "shape.txt").write_text("%d %d 1 %r %r %r\n" % (h, w, bg[0], bg[1], bg[2]))
    p = subprocess.run([exe, str(d)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert "ok wrong_count" in p.stdout and "ok value_and_grad" in p.stdout and "ok identity" in p.stdout and "all C++ lpips checks passed" in p.stdout
    m = ba.Lpips.from_params(flat, ctx=ba.get_context(dev))
    try:
        bgf = tuple(float(np.float32(v)) for v in bg)
        val, g = ba.lpips_value_and_grad(torch.from_numpy(img).to(dev), torch.from_numpy(gt.view(np.int32)).to(dev), m, composite_bg=bgf)
        val, g = val.cpu().numpy(), g.cpu().numpy()
    finally:
        m.close()
    assert np.array_equal(np.fromfile(str(d / "value.f32"), np.float32).view(np.int32), val.view(np.int32))
    assert np.array_equal(np.fromfile(str(d / "grad.f32"), np.float32).reshape(h, w, 4).view(np.int32), g.view(np.int32))
