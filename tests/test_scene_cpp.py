"""Scene editing through the C++ host mirror (include/brush_hip.hpp SceneTransform / transform_splats / transformed_splats /
select_region / crop_splats): tests/cpp/test_scene.cpp, compiled with the g++ line of tests/test_normal_cpp.py into a temporary
directory.  CPU: it compiles, links and starts; GPU: the transform, the select and the crop against bits this file writes from
brush_amd/host.py on the same scene, and the refusals.
And the host arithmetic alone (brush_amd/csrc/scene_math.h) as a stand-alone program under AddressSanitizer and UBSan:
tests/cpp/scene_math_sanitize.cpp, g++ only, run directly."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "test_scene")
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "brush_amd")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "test_scene.cpp"), "-o", exe, "-L" + lib, "-lbrush_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-ldl", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_scene_program_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)   # (no input file: nothing touches a device)
    assert r.returncode == 0 and "compile-only run" in r.stdout, r.stdout + r.stderr


def test_host_arithmetic_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "scene_math_sanitize")
    # (the runtimes are linked into the program: it needs nothing preloaded and does not mind what is)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "cpp", "scene_math_sanitize.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "scene math ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_cpp_scene_program_passes_on_the_gpu(tmp_path, dev):
    import brush_amd as ba
    from brush_amd import synth
    exe = _build(tmp_path)
    n, deg = 3000, 3
    sc = synth.make_scene(n, 0x5CE2E, sh_degree=deg, log_scale_range=(math.log(0.03), math.log(0.3)))
    rng = np.random.default_rng(21)
    ms = rng.uniform(0.0, 0.05, n).astype(np.float32)
    q, t, s = rng.normal(size=4), rng.uniform(-2, 2, 3), 1.6
    T = ba.SceneTransform.from_quat(q, t, s)
    means = sc["transforms"][:, :3]
    region = ba.SceneRegion("ellipsoid", center=tuple(np.median(means, axis=0)), half_extent=tuple(1.2 * means.std(axis=0) + 1e-3),
                            rotation=tuple(T.matrix()[:3, :3].reshape(-1) / s), min_raw_opacity=float(np.median(sc["raw_opac"])) - 1.0)
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev, min_scale=ms)
    ctx = ba.Context(dev)
    try:
        moved = spl.transformed(T, ctx=ctx)
        keep, count = ba.select_region(spl, region, ctx=ctx, return_count=True)
        crop, idx = ba.crop_splats(spl, region, return_indices=True, ctx=ctx)
        want = [moved.transforms.cpu().numpy(), moved.sh_coeffs.cpu().numpy(), moved.min_scale.cpu().numpy(), keep.cpu().numpy(),
                crop.transforms.cpu().numpy(), idx.cpu().numpy().astype(np.float32)]
    finally:
        ctx.close()
    assert 0 < count < n and crop.num_splats() == count
    path = tmp_path / "scene_case.bin"
    with open(path, "wb") as f:
        f.write(np.asarray([n, sc["sh"].shape[1], count, 0], np.uint32).tobytes())
        f.write(np.asarray(list(T.quat) + list(T.translation) + [T.scale], np.float64).tobytes())
        f.write(bytes(region.as_struct()))
        for a in [sc["transforms"], sc["sh"], sc["raw_opac"], ms] + want:
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    r = subprocess.run([exe, str(path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    for line in ("ok scene record", "ok scene transform", "ok scene crop", "ok scene arguments", "all C++ scene checks passed"):
        assert line in r.stdout, line
