"""Depth maps through the C++ host mirror (include/brush_hip.hpp RenderNode::depth and the backward overload):
tests/cpp/test_depth.cpp, compiled with the g++ line of tests/cpp/Makefile into a temporary directory.  CPU: it compiles and links;
GPU: accumulated depth of a depth-coloured scene against the CPU oracle's image within the derived bound, bit identity (two calls,
a retained forward, expected == accumulated / alpha), and the backward overload."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C0 = 0.2820947917738781


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "test_depth")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "brush_amd")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "test_depth.cpp"), "-o", exe, "-L" + lib, "-lbrush_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-ldl", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_depth_program_compiles_and_links(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_cpp_depth_program_passes_on_the_gpu(tmp_path, oracle_lib):
    from brush_amd import synth
    bo = oracle_lib
    exe = _build(tmp_path)
    # the depth-coloured scene (sh = (z - 0.5) / C0 at the default camera, whose z is the mean's) and the oracle's image of it
    n, w, h = 20000, 256, 160
    cp = synth.default_camera_params(w, h)
    sc = synth.make_scene(n, 0xC99, log_scale_range=(math.log(0.03), math.log(0.3)),
                          tan_half_fov=(math.tan(cp["fov_x"] / 2.0), math.tan(cp["fov_y"] / 2.0)))
    z = sc["transforms"][:, 2].astype(np.float32)
    sh = np.ascontiguousarray(np.repeat(((z - np.float32(0.5)) / np.float32(C0)).astype(np.float32)[:, None, None], 3, axis=2))
    p = {k: v for k, v in cp.items() if k not in ("img_w", "img_h")}
    ref = bo.Render().forward(bo.camera(img_w=w, img_h=h, **p), sc["transforms"], sh, sc["raw_opac"], bg=(0.0, 0.0, 0.0), flags=bo.FLAG_BWD_INFO)
    d = tmp_path / "scene"
    d.mkdir()
    sc["transforms"].astype(np.float32).tofile(str(d / "transforms.bin"))
    sh.tofile(str(d / "sh.bin"))
    sc["raw_opac"].astype(np.float32).tofile(str(d / "raw_opac.bin"))
    np.ascontiguousarray(ref.image()[..., 0].astype(np.float32)).tofile(str(d / "oracle_channel0.bin"))
    for args in ([str(d), str(n), str(w), str(h)], []):
        r = subprocess.run([exe] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)
        print(r.stdout[-3000:])
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        assert "ok accumulated depth" in r.stdout and "ok depth bit identity" in r.stdout and "ok depth backward" in r.stdout
        assert "all C++ depth checks passed" in r.stdout
        assert ("oracle reference" in r.stdout) == bool(args)
