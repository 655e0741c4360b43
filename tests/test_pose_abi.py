"""Camera pose gradients (include/brush_hip_pose.h) without a GPU: the header declares exactly the binding's POSE_SYMBOLS, the
library exports them, brush_hip.h gains nothing, brush_hip.hpp and host.py mirror the surface, a null context is refused before the
device is touched, and the host arithmetic (bh_pose_twist, bh_camera_apply_twist) agrees with tests/pose_ref.py in float64."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bh_render_backward_pose_saved", "bh_train_set_pose_grad", "bh_pose_twist", "bh_camera_apply_twist"}


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def test_header_declares_the_binding_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_pose.h"))
    assert declared == set(_ffi.POSE_SYMBOLS) == NAMES, declared ^ set(_ffi.POSE_SYMBOLS)
    assert '#include "brush_hip.h"' in src
    base, _ = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    assert set(_ffi.SYMBOLS) <= base and not (base & declared)
    assert len(_ffi.SYMBOLS) == 82
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = _ffi.load()
    for name in _ffi.POSE_SYMBOLS:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
        assert getattr(lib, name) is not None
    assert len(_ffi.POSE_SYMBOLS["bh_render_backward_pose_saved"][1]) == 11
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_pose.h"' in hpp
    for name in ("bh_render_backward_pose_saved(", "bh_train_set_pose_grad(", "bh_pose_twist(", "bh_camera_apply_twist("):
        assert name in hpp, name
    import inspect
    import brush_amd as ba
    assert "pose" in inspect.signature(ba.RenderNode.backward).parameters
    assert "pose_optimizer" in inspect.signature(ba.SplatTrainer.__init__).parameters
    assert hasattr(ba, "PoseOptimizer") and hasattr(ba, "pose_twist") and hasattr(ba.Camera, "apply_twist")


def test_entry_points_reject_a_null_context_without_a_device():
    from brush_amd import _ffi
    lib = _ffi.load()
    out = _ffi.BhRenderOut()
    assert lib.bh_render_backward_pose_saved(None, out, None, None, None, None, None, None, None, None, None) == -1
    assert lib.bh_train_set_pose_grad(None, None) == -1
    assert lib.bh_pose_twist(None, None, None) == -1
    assert lib.bh_camera_apply_twist(None, None) == -1


def _camera():
    import brush_amd as ba
    import util
    return ba.Camera(position=(0.3, -0.2, -3.5), rotation=util.quat_from_axis_angle((0.2, 1.0, -0.4), 0.35), fov_x=0.7, fov_y=0.6)


def test_pose_twist_is_the_references():
    import brush_amd as ba
    import pose_ref
    cam = _camera().uniforms((64, 48))
    vm = np.array(list(cam.vm), np.float64)
    rng = np.random.default_rng(3)
    for _ in range(4):
        v = rng.uniform(-1.0, 1.0, 12).astype(np.float32)
        got = ba.pose_twist(vm, v)
        want = pose_ref.twist(vm, v.astype(np.float64))
        assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
    # ... and it is the directional derivative of a linear functional <v, vm(twist)> along apply_twist
    v = rng.uniform(-1.0, 1.0, 12)
    w_mat, t = pose_ref.unpack(vm)
    e = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = e
        hi, lo = pose_ref.pack(*pose_ref.apply_twist(w_mat, t, d)), pose_ref.pack(*pose_ref.apply_twist(w_mat, t, -d))
        num = float(v @ (hi - lo)) / (2 * e)
        assert abs(num - pose_ref.twist(vm, v)[k]) <= 1e-6


def test_camera_apply_twist_is_the_references():
    import brush_amd as ba
    import pose_ref
    from brush_amd import _ffi
    base = _camera()
    cam = base.uniforms((64, 48))
    same = ba.host._uniforms_apply_twist(cam, np.zeros(6))
    assert bytes(same) == bytes(cam), "a zero twist is the identity"
    assert np.abs(np.array(base.apply_twist(np.zeros(6)).uniforms((64, 48)).vm[:]) - np.array(cam.vm[:])).max() <= 4e-7
    tw = np.array([0.03, -0.02, 0.05, 0.2, -0.1, 0.15])
    got = ba.host._uniforms_apply_twist(cam, tw)
    w_mat, t = pose_ref.unpack(np.array(list(cam.vm), np.float64))
    w2, t2 = pose_ref.apply_twist(w_mat, t, tw)
    assert np.abs(w2 @ w2.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(w2) - 1.0) <= 1e-12
    # the library's f64 result, stored as f32: the reference rounded to f32, give or take the last bit
    want = pose_ref.pack(w2, t2)
    assert np.abs(np.array(list(got.vm), np.float64) - want).max() <= 2.0 ** -23 * max(1.0, np.abs(want).max())
    w_got, t_got = pose_ref.unpack(np.array(list(got.vm), np.float64))
    assert np.abs(w_got @ w_got.T - np.eye(3)).max() <= 4 * 2.0 ** -24
    assert np.abs(np.array(list(got.cam_pos), np.float64) + w2.T @ t2).max() <= 2.0 ** -23 * max(1.0, np.abs(t2).max())
    # everything else is untouched
    for f, _ in _ffi.BhCamera._fields_:
        if f not in ("vm", "cam_pos"):
            a, b = getattr(got, f), getattr(cam, f)
            assert (a[:] == b[:]) if hasattr(a, "__len__") else (a == b), f
    # Camera.apply_twist is the same map (through the library, position and rotation read back from the moved matrix)
    moved = base.apply_twist(tw).uniforms((64, 48))
    assert np.abs(np.array(list(moved.vm)) - np.array(list(got.vm))).max() <= 4e-7
    assert np.abs(np.array(list(moved.cam_pos)) - np.array(list(got.cam_pos))).max() <= 2e-6


def test_camera_apply_twist_refuses_what_is_no_pose():
    """A view matrix whose first two columns are zero or parallel, or a twist that is not finite, would end in NaN: -1, and the
    camera is left as it was."""
    from brush_amd import _ffi
    lib = _ffi.load()
    tw = (C.c_double * 6)(0.03, -0.02, 0.05, 0.2, -0.1, 0.15)
    for bad in ("zero column 0", "zero column 1", "parallel columns"):
        cam = _camera().uniforms((64, 48))
        if bad == "zero column 0":
            cam.vm[0:3] = [0.0, 0.0, 0.0]
        elif bad == "zero column 1":
            cam.vm[3:6] = [0.0, 0.0, 0.0]
        else:
            cam.vm[3:6] = [2.0 * x for x in cam.vm[0:3]]
        before = bytes(cam)
        assert lib.bh_camera_apply_twist(C.byref(cam), tw) == -1, bad
        assert bytes(cam) == before, bad
    cam = _camera().uniforms((64, 48))
    before = bytes(cam)
    for k, x in ((1, float("nan")), (4, float("inf"))):
        bad_tw = (C.c_double * 6)(*tw)
        bad_tw[k] = x
        assert lib.bh_camera_apply_twist(C.byref(cam), bad_tw) == -1 and bytes(cam) == before, (k, x)
    assert lib.bh_camera_apply_twist(C.byref(cam), tw) == 0 and np.isfinite(np.array(list(cam.vm))).all()


def test_trainer_checks_the_partition_before_the_pose_optimizer():
    import brush_amd as ba
    import pytest
    po = ba.PoseOptimizer()
    with pytest.raises(ValueError, match="partition must be"):
        ba.SplatTrainer(ba.TrainConfig(), partition="strips", pose_optimizer=po)
    with pytest.raises(ValueError, match="pose_optimizer is not available"):
        ba.SplatTrainer(ba.TrainConfig(), partition="tiles", pose_optimizer=po)


def test_pose_optimizer_is_adam_on_the_twist():
    import brush_amd as ba
    import pose_ref
    cam = _camera().uniforms((64, 48))
    po = ba.PoseOptimizer(lr_rotation=1e-2, lr_translation=2e-2)
    v = np.linspace(-1.0, 1.0, 12)
    g = po.update(7, list(cam.vm), v)
    assert np.allclose(g, pose_ref.twist(np.array(list(cam.vm), np.float64), v), atol=1e-6)
    # Adam's first step is lr * sign(g)
    assert np.allclose(po.twist(7), -np.array([1e-2] * 3 + [2e-2] * 3) * np.sign(g), rtol=1e-6)
    assert not po.twist(8).any()
    moved = po.camera(7, cam)
    assert moved.vm[:] != cam.vm[:] and po.camera(8, cam).vm[:] == cam.vm[:]
