"""Distortion maps through the C++ host mirror (include/brush_hip.hpp RenderNode::distortion / backward_distortion, distortion_loss,
train_set_distortion): tests/cpp/test_distortion.cpp, compiled with the g++ line of tests/test_normal_cpp.py into a temporary directory.
CPU: it compiles, links and starts; GPU: the maps, the loss and one backward per kind against numbers this file writes from
brush_amd/host.py on the same scene, and the refusals."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "test_distortion")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "brush_amd")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "test_distortion.cpp"), "-o", exe, "-L" + lib, "-lbrush_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-ldl", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_distortion_program_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)   # (no input file: nothing touches a device)
    assert r.returncode == 0 and "compile-only run" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_distortion_program_passes_on_the_gpu(tmp_path, dev):
    import torch
    import brush_amd as ba
    from brush_amd import synth
    import util
    exe = _build(tmp_path)
    n, w, h = 3000, 123, 82
    near, far, weight = 0.5, 20.0, 0.37
    cp = synth.default_camera_params(w, h)
    sc = synth.make_scene(n, 0x9A11, sh_degree=0, log_scale_range=(math.log(0.03), math.log(0.3)), z_range=(2.0, 12.0),
                          tan_half_fov=(math.tan(cp["fov_x"] / 2.0), math.tan(cp["fov_y"] / 2.0)))
    rng = np.random.default_rng(5)
    v_dist = (rng.uniform(-1.0, 1.0, (h, w)) / (h * w)).astype(np.float32)
    v_out = (rng.uniform(-1.0, 1.0, (h, w, 4)) / (h * w)).astype(np.float32)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    ctx = ba.Context(dev)
    try:
        node = ba.render_splats_diff(spl, util.hip_camera(ba, cp), (w, h), ctx=ctx)
        maps = [node.distortion("z").cpu().numpy(), node.distortion("ndc", near, far).cpu().numpy()]
        loss = ba.distortion_loss(node.distortion("z"), weight, ctx=ctx).cpu().numpy()
        grads = []
        for kind in ("z", "ndc"):
            g = node.backward(None, v_distortion=torch.from_numpy(v_dist).to(dev), distortion=kind, distortion_near=near, distortion_far=far)
            grads += [g["v_transforms"].cpu().numpy(), g["v_raw_opacities"].cpu().numpy()]
    finally:
        ctx.close()
    path = tmp_path / "distortion_case.bin"
    with open(path, "wb") as f:
        f.write(np.asarray([n, w, h, sc["sh"].shape[1]], np.uint32).tobytes())
        f.write(np.asarray([near, far, weight, 0.0], np.float32).tobytes())
        for a in [sc["transforms"], sc["sh"], sc["raw_opac"], v_dist, v_out] + maps + [loss] + grads:
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    r = subprocess.run([exe, str(path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    for line in ("ok distortion forward", "ok distortion loss", "ok distortion backward", "ok distortion arguments", "all C++ distortion checks passed"):
        assert line in r.stdout, line
