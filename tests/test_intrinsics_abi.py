"""Camera intrinsics gradients (include/brush_hip_intrinsics.h) without a GPU: the header declares exactly the binding's
INTRINSICS_SYMBOLS, both libraries export them, brush_hip.h keeps its 82, brush_hip.hpp and host.py mirror the surface, a null context
is refused before the device is touched, bh_camera_set_intrinsics reproduces bh_camera_setup_model's BhCamera byte for byte for the
four lens models and refuses what is no focal length, and SplatTrainer refuses what the pass cannot carry."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import pytest

import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bh_render_backward_intrinsics_saved", "bh_render_backward_camera_saved", "bh_train_set_intrinsics_grad", "bh_camera_set_intrinsics"}


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def test_header_declares_the_binding_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_intrinsics.h"))
    assert declared == set(_ffi.INTRINSICS_SYMBOLS) == NAMES, declared ^ set(_ffi.INTRINSICS_SYMBOLS)
    assert '#include "brush_hip.h"' in src
    base, _ = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    assert set(_ffi.SYMBOLS) <= base and not (base & declared)
    assert len(_ffi.SYMBOLS) == 82
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported_th = subprocess.run(["nm", "-D", "--defined-only", _ffi.TEST_HOOKS_LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = _ffi.load()
    for name in _ffi.INTRINSICS_SYMBOLS:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
        assert re.search(r"\bT %s$" % name, exported_th, flags=re.M), name
        assert getattr(lib, name) is not None
    assert [len(_ffi.INTRINSICS_SYMBOLS[k][1]) for k in sorted(NAMES)] == [5, 13, 12, 2]
    assert C.sizeof(_ffi.BhCameraGradTerms) == 48
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_intrinsics.h"' in hpp
    for name in ("backward_intrinsics(", "backward_camera(", "train_set_intrinsics_grad(", "camera_set_intrinsics("):
        assert name in hpp, name
    pose = open(os.path.join(ROOT, "include", "brush_hip_pose.h")).read()
    assert "brush_hip_intrinsics.h" in pose


def test_python_mirror_has_the_surface():
    import brush_amd as ba
    assert "intrinsics" in inspect.signature(ba.RenderNode.backward).parameters
    assert inspect.signature(ba.RenderNode.backward).parameters["intrinsics"].default is False
    assert list(inspect.signature(ba.Camera.with_intrinsics).parameters) == ["self", "fx", "fy", "cx", "cy", "img_size"]
    for name in ("camera", "bind", "update", "step"):
        assert hasattr(ba.IntrinsicsOptimizer, name) and hasattr(ba.PoseOptimizer, name), name
    init = inspect.signature(ba.IntrinsicsOptimizer.__init__).parameters
    assert init["lr_focal"].default == 1e-3 and init["lr_center"].default == 1e-4
    assert init["sensor_of"].default is None and init["share_focal"].default is False
    assert "intrinsics_optimizer" in inspect.signature(ba.SplatTrainer.__init__).parameters


def test_entry_points_reject_null_arguments_without_a_device():
    from brush_amd import _ffi
    lib = _ffi.load()
    assert lib.bh_render_backward_intrinsics_saved(None, None, *([None] * 10)) == -1
    assert lib.bh_render_backward_camera_saved(None, None, None, None, *([None] * 9)) == -1
    assert lib.bh_train_set_intrinsics_grad(None, None) == -1
    assert lib.bh_camera_set_intrinsics(None, 1.0, 1.0, 0.0, 0.0) == -1


LENSES = ["pinhole", "kb4", "rt8", "tpf"]


def _setup(model, w, h, center=(0.47, 0.53)):
    import brush_amd as ba
    dist = () if model == "pinhole" else util.REF_LENSES[model][1]
    cam = ba.Camera(position=(0.1, -0.2, 0.3), rotation=util.quat_from_axis_angle((0.3, 1.0, 0.1), 0.2), fov_x=0.9, fov_y=0.7, center_uv=center,
                    camera_model=model, dist=tuple(dist))
    return cam, cam.uniforms((w, h))


@pytest.mark.parametrize("model", LENSES)
def test_set_intrinsics_reproduces_the_camera_set_up_byte_for_byte(model):
    """Handed the camera's own intrinsics — the f64 focal lengths bh_fov_to_focal gives for its fields of view, which the f32 fields
    fx, fy are the rounding of, and its cx, cy — on a copy whose derived fields are spoilt first."""
    import brush_amd as ba
    from brush_amd import _ffi
    lib = _ffi.load()
    w, h = 123, 82
    cam, u = _setup(model, w, h)
    fx = ba.fov_to_focal(cam.fov_x, w, cam.camera_model, cam.dist)
    fy = ba.fov_to_focal(cam.fov_y, h, cam.camera_model, cam.dist)
    assert C.c_float(fx).value == u.fx and C.c_float(fy).value == u.fy
    out = _ffi.BhCamera()
    C.memmove(C.byref(out), C.byref(u), C.sizeof(_ffi.BhCamera))
    out.fx, out.fy, out.cx, out.cy = 1.0, 2.0, 3.0, 4.0
    out.lim_pos_x = out.lim_pos_y = out.lim_neg_x = out.lim_neg_y = 7.0
    out.half_max_render_fov = 9.0
    assert bytes(out) != bytes(u)
    assert lib.bh_camera_set_intrinsics(C.byref(out), fx, fy, float(u.cx), float(u.cy)) == 0
    assert bytes(out) == bytes(u)
    if model == "rt8":
        assert out.lim_pos_x > 0.0 > out.lim_neg_x and out.lim_pos_x != (1.15 * w - u.cx) / u.fx   # the undistorted edges
    if model in ("kb4", "tpf"):
        assert out.lim_pos_x == out.lim_pos_y == out.lim_neg_x == out.lim_neg_y == 0.0
    # other intrinsics: the limits follow them (pinhole: the image edges +-15 % in normalised coordinates, in f32)
    assert lib.bh_camera_set_intrinsics(C.byref(out), 1.25 * fx, fy, float(u.cx) + 2.0, float(u.cy)) == 0
    assert out.fx == C.c_float(1.25 * fx).value and out.cx == u.cx + 2.0 and out.fy == u.fy and out.cy == u.cy
    assert list(out.vm) == list(u.vm) and list(out.cam_pos) == list(u.cam_pos) and (out.img_w, out.img_h) == (w, h)
    if model == "pinhole":
        f32 = lambda v: C.c_float(v).value
        assert out.lim_pos_x == f32(f32(f32(f32(1.15) * w) - out.cx) / out.fx) and out.lim_pos_x < u.lim_pos_x
        assert out.half_max_render_fov < u.half_max_render_fov


@pytest.mark.parametrize("model", LENSES)
def test_set_intrinsics_refuses_what_is_no_focal_length(model):
    from brush_amd import _ffi
    lib = _ffi.load()
    _, u = _setup(model, 64, 48)
    for bad in [(0.0, 50.0, 1.0, 1.0), (50.0, -1.0, 1.0, 1.0), (float("nan"), 50.0, 1.0, 1.0), (50.0, float("inf"), 1.0, 1.0),
                (50.0, 50.0, float("nan"), 1.0), (50.0, 50.0, 1.0, float("-inf")), (1e-60, 50.0, 1.0, 1.0), (1e60, 50.0, 1.0, 1.0)]:
        out = _ffi.BhCamera()
        C.memmove(C.byref(out), C.byref(u), C.sizeof(_ffi.BhCamera))
        assert lib.bh_camera_set_intrinsics(C.byref(out), *bad) == -1, bad
        assert bytes(out) == bytes(u), bad


def test_camera_with_intrinsics_and_the_optimizer_mirror():
    import brush_amd as ba
    w, h = 96, 64
    cam, u = _setup("kb4", w, h)
    same = cam.with_intrinsics(u.fx, u.fy, u.cx, u.cy, (w, h))
    assert abs(same.fov_x - cam.fov_x) <= 1e-6 and abs(same.fov_y - cam.fov_y) <= 1e-6
    assert max(abs(a - b) for a, b in zip(same.center_uv, cam.center_uv)) <= 1e-7
    moved = cam.with_intrinsics(1.1 * u.fx, u.fy, u.cx + 3.0, u.cy, (w, h)).uniforms((w, h))
    assert abs(moved.fx - 1.1 * u.fx) <= 1e-4 * u.fx and abs(moved.cx - (u.cx + 3.0)) <= 1e-4 and abs(moved.fy - u.fy) <= 1e-4 * u.fy
    with pytest.raises(ValueError):
        cam.with_intrinsics(0.0, u.fy, u.cx, u.cy, (w, h))
    # the optimizer: an untouched sensor renders the base camera to the bit; one update moves against the gradient by lr (Adam's
    # first step), per sensor, and the parameters are free of the resolution
    io = ba.IntrinsicsOptimizer(sensor_of={1: 0, 2: 0, 3: 5})
    assert bytes(io.camera(1, cam, (w, h))) == bytes(u)
    g = io.update(1, u, [2.0, -1.0, 0.5, -0.25])
    assert list(g) == [2.0 * u.fx, -1.0 * u.fy, 0.5 * w, -0.25 * h]
    p = io.params(2)
    assert all(abs(a - b) <= 1e-9 for a, b in zip(p, [-1e-3, 1e-3, -1e-4, 1e-4]))
    assert list(io.params(3)) == [0.0] * 4 and list(io.params(9)) == list(p)   # a view no sensor names belongs to sensor 0
    c1, c2 = io.camera(2, cam, (w, h)), io.camera(2, cam, (2 * w, 2 * h))
    u2 = cam.uniforms((2 * w, 2 * h))
    assert abs(c1.fx - u.fx * math.exp(-1e-3)) <= 1e-5 * u.fx and abs(c2.fx - u2.fx * math.exp(-1e-3)) <= 1e-5 * u2.fx
    assert abs(c1.cx - (u.cx - 1e-4 * w)) <= 1e-5 and abs(c2.cx - (u2.cx - 1e-4 * 2 * w)) <= 1e-5
    tied = ba.IntrinsicsOptimizer(share_focal=True)
    g = tied.update(1, u, [2.0, -1.0, 0.0, 0.0])
    assert g[0] == g[1] == 2.0 * u.fx - 1.0 * u.fy and tied.params(1)[0] == tied.params(1)[1]
    with pytest.raises(ValueError):
        io.camera(0, cam, (w, h))


def test_trainer_refuses_what_the_pass_cannot_carry():
    import brush_amd as ba
    io = ba.IntrinsicsOptimizer()
    with pytest.raises(ValueError, match="intrinsics_optimizer is not available"):
        ba.SplatTrainer(ba.TrainConfig(), partition="tiles", intrinsics_optimizer=io)
    with pytest.raises(ValueError, match="envmap and intrinsics_optimizer"):
        ba.SplatTrainer(ba.TrainConfig(), envmap=object(), intrinsics_optimizer=io)
    with pytest.raises(ValueError, match="normal_loss_weight"):
        ba.SplatTrainer(ba.TrainConfig(normal_loss_weight=0.1), intrinsics_optimizer=io)
    t = ba.SplatTrainer(ba.TrainConfig(), intrinsics_optimizer=io, pose_optimizer=ba.PoseOptimizer())
    assert t.intrinsics_optimizer is io and t.pose_optimizer is not None
