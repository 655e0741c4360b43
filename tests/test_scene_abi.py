"""Scene editing (include/brush_hip_scene.h) without a GPU: the header declares exactly the binding's SCENE_SYMBOLS and parses as C and
as C++, the library exports them, _ffi.py mirrors the structs' sizes, field order and offsets, brush_hip.h declares what it declared
before (its 82 entry points), argument checks run before the device is touched, and the host arithmetic — the record of a transform
with its SH rotation matrices, compose, invert, the camera — agrees with tests/scene_ref.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import scene_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bh_scene_transform_make", "bh_scene_transform_compose", "bh_scene_transform_invert", "bh_camera_apply_scene_transform",
         "bh_splats_transform", "bh_splats_select_region"}
TRANSFORM_FIELDS = [("q", 0), ("t", 32), ("s", 56), ("rot", 64), ("quat", 100), ("trans", 116), ("scale", 128), ("log_scale", 132), ("sh_rot", 136),
                    ("reserved", 792)]
REGION_FIELDS = [("kind", 0), ("invert", 4), ("center", 8), ("half_extent", 20), ("rot", 32), ("min_raw_opacity", 68), ("reserved", 72)]


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", src)), src


def _lib():
    import __graft_entry__ as g
    g.build()
    from brush_amd import _ffi
    return _ffi.load(), _ffi


def _make(lib, _ffi, q, t, s):
    rec = _ffi.BhSceneTransform()
    rc = lib.bh_scene_transform_make((C.c_double * 4)(*q), (C.c_double * 3)(*t), float(s), C.byref(rec))
    return rc, rec


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))))


def test_header_parses_as_c_and_as_cpp(tmp_path):
    inc = os.path.join(ROOT, "include")
    for lang, std, ext in (("c", "-std=c11", "c"), ("c++", "-std=c++17", "cpp")):
        src = tmp_path / ("parse." + ext)
        src.write_text('#include "brush_hip_scene.h"\nint main(void) { return (int)sizeof(BhSceneTransform) + (int)sizeof(BhSceneRegion) - 876; }\n')
        exe = str(tmp_path / ("parse_" + ext))
        subprocess.check_call([os.environ.get("CXX", "g++"), "-x", lang, std, "-Wall", "-Werror", "-I" + inc, str(src), "-o", exe])
        assert subprocess.run([exe]).returncode == 0


def test_header_declares_the_binding_and_the_library_exports_it():
    lib, _ffi = _lib()
    declared, src = _declared(os.path.join(ROOT, "include", "brush_hip_scene.h"))
    assert declared == set(_ffi.SCENE_SYMBOLS) == NAMES, declared ^ set(_ffi.SCENE_SYMBOLS)
    assert re.search(r"#define BH_REGION_BOX 0u", src) and re.search(r"#define BH_REGION_ELLIPSOID 1u", src)
    assert (_ffi.REGION_BOX, _ffi.REGION_ELLIPSOID) == (0, 1)
    for name, mirror, fields, size in (("BhSceneTransform", _ffi.BhSceneTransform, TRANSFORM_FIELDS, 800), ("BhSceneRegion", _ffi.BhSceneRegion, REGION_FIELDS, 76)):
        sizes = set(re.findall(r"static_assert\(sizeof\(%s\) == (\d+)" % name, src, flags=re.I))
        assert sizes == {str(C.sizeof(mirror))} == {str(size)}, (name, sizes)
        assert [f[0] for f in mirror._fields_] == [f for f, _ in fields]
        assert [getattr(mirror, f).offset for f, _ in fields] == [o for _, o in fields]
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
        assert re.findall(r"\b(\w+)(?:\[\d+\])?;", body) == [f for f, _ in fields], (name, body)
    # brush_hip.h declares what it declared before (82 entry points and the test-hooks build's bh_debug_fill_train_scratch)
    base, _ = _declared(os.path.join(ROOT, "include", "brush_hip.h"))
    assert len(_ffi.SYMBOLS) == 82 and base == set(_ffi.SYMBOLS) | {"bh_debug_fill_train_scratch"} and not (base & declared)
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
        assert getattr(lib, name) is not None
        proto = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len([p for p in proto.split(",") if p.strip()]) == len(_ffi.SCENE_SYMBOLS[name][1]), name
    # no option was added for it
    assert not [i for i in range(lib.bh_option_count()) if b"scene" in lib.bh_option_name(i) or b"region" in lib.bh_option_name(i)]
    mk = open(os.path.join(ROOT, "brush_amd", "csrc", "Makefile")).read()
    assert " scene_edit.hip" in mk and mk.count("brush_hip_scene.h") == 2


def test_the_other_mirrors_carry_the_names():
    hpp = open(os.path.join(ROOT, "include", "brush_hip.hpp")).read()
    assert '#include "brush_hip_scene.h"' in hpp
    for name in ("struct SceneTransform", "bh_scene_transform_make(", "bh_scene_transform_compose(", "bh_scene_transform_invert(",
                 "bh_camera_apply_scene_transform(", "bh_splats_transform(", "bh_splats_select_region(", "crop_splats(", "select_region(",
                 "sizeof(BhSceneTransform) == 800", "sizeof(BhSceneRegion) == 76"):
        assert name in hpp, name
    import brush_amd as ba
    for name in ("SceneTransform", "SceneRegion", "select_region", "crop_splats"):
        assert hasattr(ba, name), name
    for cls, name in ((ba.Splats, "transformed"), (ba.Splats, "transform_"), (ba.Camera, "transformed"), (ba.SceneTransform, "from_quat"),
                      (ba.SceneTransform, "from_matrix"), (ba.SceneTransform, "inverse"), (ba.SceneTransform, "__matmul__"), (ba.SceneTransform, "matrix"),
                      (ba.SceneTransform, "as_struct"), (ba.SceneTransform, "sh_rotation")):
        assert hasattr(cls, name), (cls, name)


def test_entry_points_reject_a_null_context_without_a_device():
    lib, _ffi = _lib()
    rc, rec = _make(lib, _ffi, (1, 0, 0, 0), (0, 0, 0), 1.0)
    assert rc == 0
    region = _ffi.BhSceneRegion(kind=0)
    assert lib.bh_splats_transform(None, C.byref(rec), 4, 1, None, None, None, None, None, None) == -1
    assert lib.bh_splats_select_region(None, C.byref(region), None, None, 4, None, None) == -1


def test_make_agrees_with_the_restatement():
    lib, _ffi = _lib()
    rng = np.random.default_rng(7)
    for k in range(12):
        q, t, s = rng.normal(size=4) * (1.0 if k % 3 else 7.5), rng.uniform(-5, 5, 3), math.exp(rng.uniform(-2, 2))
        rc, rec = _make(lib, _ffi, q, t, s)
        assert rc == 0
        want, got = sr.make_record(q, t, s), sr.record_from_struct(rec)
        assert got["q"][0] >= 0 and abs(np.linalg.norm(got["q"]) - 1.0) <= 1e-15
        assert np.abs(got["q"] - want["q"]).max() <= 1e-15 and np.array_equal(got["t"], want["t"]) and got["s"] == want["s"]
        for f in ("rot", "quat", "trans", "scale", "log_scale"):
            assert _ulps(got[f], want[f]) <= 1.0, (f, got[f], want[f])
        # entries are bounded by 1; least squares on either side, through seven-digit constants
        assert float(np.abs(got["sh_rot"] - want["sh_rot"]).max()) <= 1e-6
        assert list(rec.reserved) == [0, 0]
    # the identity: exactly, and D_l = I to the fit's rounding
    rc, rec = _make(lib, _ffi, (2, 0, 0, 0), (0, 0, 0), 1.0)
    assert rc == 0 and list(rec.q) == [1, 0, 0, 0] and list(rec.rot) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and rec.scale == 1.0 and rec.log_scale == 0.0
    for l in range(1, 5):
        m = 2 * l + 1
        D = np.array(rec.sh_rot[sr.SH_ROT_OFFSET[l]:sr.SH_ROT_OFFSET[l] + m * m]).reshape(m, m)
        assert np.abs(D - np.eye(m)).max() <= 1e-6


def test_invert_and_compose():
    lib, _ffi = _lib()
    rng = np.random.default_rng(8)
    for _ in range(10):
        qa, ta, sa = rng.normal(size=4), rng.uniform(-3, 3, 3), math.exp(rng.uniform(-1, 1))
        qb, tb, sb = rng.normal(size=4), rng.uniform(-3, 3, 3), math.exp(rng.uniform(-1, 1))
        (_, a), (_, b) = _make(lib, _ffi, qa, ta, sa), _make(lib, _ffi, qb, tb, sb)
        inv, ident, ab = _ffi.BhSceneTransform(), _ffi.BhSceneTransform(), _ffi.BhSceneTransform()
        assert lib.bh_scene_transform_invert(C.byref(a), C.byref(inv)) == 0
        assert lib.bh_scene_transform_compose(C.byref(inv), C.byref(a), C.byref(ident)) == 0
        assert np.abs(np.array(ident.q) - [1, 0, 0, 0]).max() <= 1e-12 and np.abs(np.array(ident.t)).max() <= 1e-12 and abs(ident.s - 1.0) <= 1e-12
        # compose(a, b) applies b first
        assert lib.bh_scene_transform_compose(C.byref(a), C.byref(b), C.byref(ab)) == 0
        ra, rb, rab = sr.record_from_struct(a), sr.record_from_struct(b), sr.record_from_struct(ab)
        x = rng.normal(size=3)
        want = ra["s"] * ra["R"] @ (rb["s"] * rb["R"] @ x + rb["t"]) + ra["t"]
        assert np.abs(rab["s"] * rab["R"] @ x + rab["t"] - want).max() <= 1e-12
        # every derived field is refilled
        full = sr.make_record(rab["q"], rab["t"], rab["s"])
        assert _ulps(rab["rot"], full["rot"]) <= 1.0 and np.abs(rab["sh_rot"] - full["sh_rot"]).max() <= 1e-6
        # in place
        assert lib.bh_scene_transform_invert(C.byref(a), C.byref(a)) == 0
        assert bytes(a) == bytes(inv)


def test_bad_arguments_are_refused():
    lib, _ffi = _lib()
    nan, inf = math.nan, math.inf
    for q, t, s in (((0, 0, 0, 0), (0, 0, 0), 1.0), ((nan, 0, 0, 0), (0, 0, 0), 1.0), ((1, inf, 0, 0), (0, 0, 0), 1.0), ((1, 0, 0, 0), (0, nan, 0), 1.0),
                    ((1, 0, 0, 0), (inf, 0, 0), 1.0), ((1, 0, 0, 0), (0, 0, 0), 0.0), ((1, 0, 0, 0), (0, 0, 0), -2.0), ((1, 0, 0, 0), (0, 0, 0), inf),
                    ((1, 0, 0, 0), (0, 0, 0), nan)):
        rec = _ffi.BhSceneTransform()
        rec.reserved[0] = 77
        assert lib.bh_scene_transform_make((C.c_double * 4)(*q), (C.c_double * 3)(*t), float(s), C.byref(rec)) == -1, (q, t, s)
        assert rec.reserved[0] == 77 and rec.s == 0.0   # untouched
    rc, ok = _make(lib, _ffi, (1, 2, 3, 4), (1, 2, 3), 2.0)
    assert rc == 0
    out = _ffi.BhSceneTransform()
    assert lib.bh_scene_transform_make(None, (C.c_double * 3)(), 1.0, C.byref(out)) == -1
    assert lib.bh_scene_transform_compose(C.byref(ok), None, C.byref(out)) == -1 and lib.bh_scene_transform_invert(None, C.byref(out)) == -1
    bad = _ffi.BhSceneTransform()   # all zero: no transform
    assert lib.bh_scene_transform_compose(C.byref(ok), C.byref(bad), C.byref(out)) == -1 and lib.bh_scene_transform_invert(C.byref(bad), C.byref(out)) == -1
    cam = _ffi.BhCamera()
    assert lib.bh_camera_apply_scene_transform(None, C.byref(ok), C.byref(cam)) == -1
    assert lib.bh_camera_apply_scene_transform(C.byref(cam), None, C.byref(cam)) == -1
    assert lib.bh_camera_apply_scene_transform(C.byref(cam), C.byref(bad), C.byref(cam)) == -1


def test_camera_transform_agrees_with_the_formulas():
    lib, _ffi = _lib()
    import brush_amd as ba
    import util
    rng = np.random.default_rng(9)
    for k in range(6):
        q, t, s = rng.normal(size=4), rng.uniform(-3, 3, 3), math.exp(rng.uniform(-1, 1))
        T = ba.SceneTransform.from_quat(q, t, s)
        base = ba.Camera(position=tuple(rng.uniform(-2, 2, 3)), rotation=util.quat_from_axis_angle(rng.normal(size=3), rng.uniform(0, 3)), fov_x=0.8, fov_y=0.6,
                         camera_model=("pinhole", "kb4")[k % 2], dist=((), (-0.05, 0.01, -0.001, 5e-5))[k % 2])
        cam = base.uniforms((96, 80))
        out = _ffi.BhCamera()
        assert lib.bh_camera_apply_scene_transform(C.byref(cam), C.byref(T.as_struct()), C.byref(out)) == 0
        vm, pos = sr.camera_apply(list(cam.vm), list(cam.cam_pos), sr.record_from_struct(T.as_struct()))
        assert np.abs(np.array(out.vm) - vm).max() <= 1e-6 * max(1.0, np.abs(vm).max()) and np.abs(np.array(out.cam_pos) - pos).max() <= 1e-6 * max(1.0, np.abs(pos).max())
        # everything else is copied
        keep_vm, keep_pos = list(out.vm), list(out.cam_pos)
        out.vm[:], out.cam_pos[:] = list(cam.vm), list(cam.cam_pos)
        assert bytes(out) == bytes(cam)
        # camera space is s times the old one: W' x' + tv' = s (W x + tv)
        x = rng.normal(size=3)
        W, tv = np.array(cam.vm[:9]).reshape(3, 3).T, np.array(cam.vm[9:])
        W2, tv2 = np.array(keep_vm[:9]).reshape(3, 3).T, np.array(keep_vm[9:])
        assert np.abs(W2 @ (T.matrix() @ np.append(x, 1.0))[:3] + tv2 - s * (W @ x + tv)).max() <= 1e-5 * s * (1.0 + np.abs(W @ x + tv).max())
        # the Python Camera: the same pose, and cam_pos = -W^T tv again
        moved = base.transformed(T).uniforms((96, 80))
        assert np.abs(np.array(moved.vm) - np.array(keep_vm)).max() <= 1e-5 * max(1.0, np.abs(vm).max())
        assert np.abs(np.array(moved.cam_pos) - np.array(keep_pos)).max() <= 1e-5 * max(1.0, np.abs(pos).max())


def test_scene_transform_class():
    import brush_amd as ba
    rng = np.random.default_rng(10)
    q, t, s = rng.normal(size=4), rng.uniform(-3, 3, 3), 1.7
    T = ba.SceneTransform.from_quat(q, t, s)
    M = T.matrix()
    assert M.shape == (4, 4) and abs(np.linalg.det(M[:3, :3]) - s ** 3) <= 1e-12 and np.array_equal(M[3], [0, 0, 0, 1])
    back = ba.SceneTransform.from_matrix(M)
    assert np.abs(back.matrix() - M).max() <= 1e-12
    assert np.abs((T @ T.inverse()).matrix() - np.eye(4)).max() <= 1e-12
    U = ba.SceneTransform.from_quat(rng.normal(size=4), rng.uniform(-1, 1, 3), 0.5)
    assert np.abs((T @ U).matrix() - T.matrix() @ U.matrix()).max() <= 1e-12
    for l in range(1, 5):
        D = T.sh_rotation(l)
        assert D.shape == (2 * l + 1, 2 * l + 1) and D.dtype == np.float32
        assert np.abs(D - sr.sh_rotation_matrices(M[:3, :3] / s)[l - 1]).max() <= 1e-6
    assert isinstance(T.as_struct(), type(ba.SceneTransform().as_struct())) and ba.SceneTransform().scale == 1.0
    # a matrix stored in f32 passes the stated tolerance; shear, a reflection and a projective row do not
    assert np.abs(ba.SceneTransform.from_matrix(M.astype(np.float32)).matrix() - M).max() <= 1e-5
    shear, mirror, proj = M.copy(), M.copy(), M.copy()
    shear[0, 1] += 0.01
    mirror[:3, 0] = -mirror[:3, 0]
    proj[3, 0] = 0.01
    nonuniform = M @ np.diag([1.0, 1.0, 1.01, 1.0])
    for bad in (shear, mirror, proj, nonuniform, M[:3]):
        with pytest.raises(ValueError):
            ba.SceneTransform.from_matrix(bad)
    with pytest.raises(ba.BrushHipError):
        ba.SceneTransform.from_quat((0, 0, 0, 0))
