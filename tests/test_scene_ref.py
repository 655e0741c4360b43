"""tests/scene_ref.py pinned without a GPU: its SH rotation matrices are orthogonal, a homomorphism, and rotate the function they
describe; and the float32 restatement of the scene transform passes the end-to-end invariant on the CPU oracle — the transformed
scene from the transformed camera is the same image — while the same scene with its SH left unrotated does not."""
import ctypes as C

import numpy as np
import pytest

import scene_ref as sr


def _rotation(rng):
    q = rng.normal(size=4)
    return sr.quat_to_matrix(q / np.linalg.norm(q))


def test_sh_rotation_matrices_are_orthogonal():
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(10):
        for D in sr.sh_rotation_matrices(_rotation(rng)):
            worst = max(worst, float(np.abs(D @ D.T - np.eye(D.shape[0])).max()))
    print("D D^T - I: %.3e" % worst)
    assert worst <= 5e-7   # (the basis constants have seven digits: measured 9e-8)


def test_sh_rotation_matrices_compose():
    rng = np.random.default_rng(2)
    worst = 0.0
    for _ in range(10):
        r1, r2 = _rotation(rng), _rotation(rng)
        for d12, d1, d2 in zip(sr.sh_rotation_matrices(r1 @ r2), sr.sh_rotation_matrices(r1), sr.sh_rotation_matrices(r2)):
            worst = max(worst, float(np.abs(d12 - d1 @ d2).max()))
    print("D(R1 R2) - D(R1) D(R2): %.3e" % worst)
    assert worst <= 1e-8   # (measured 5e-10)


def test_rotated_coefficients_describe_the_rotated_function():
    rng = np.random.default_rng(3)
    for _ in range(5):
        R = _rotation(rng)
        d = rng.normal(size=(1000, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        Y, Yr = sr.sh_basis(d), sr.sh_basis(d @ R)   # rows of d @ R are R^T d
        for l, D in enumerate(sr.sh_rotation_matrices(R), start=1):
            sl = slice(l * l, (l + 1) * (l + 1))
            a = rng.normal(size=2 * l + 1)
            err = np.abs(Y[:, sl] @ (D @ a) - Yr[:, sl] @ a).max()
            assert err <= 1e-6 * np.linalg.norm(a), (l, err)


def _oracle_pair(bo, degree, mip, seed, rotate_sh=True):
    sc, (q, t, s) = sr.invariant_case(degree, seed)
    rec = sr.make_record(q, t, s)
    cam = bo.camera(img_w=sr.IMG_W, img_h=sr.IMG_H, **sr.CAM)
    moved = bo.BoCamera()
    C.memmove(C.byref(moved), C.byref(cam), C.sizeof(cam))
    vm, pos = sr.camera_apply(list(cam.vm), list(cam.cam_pos), rec)
    moved.vm[:] = [float(v) for v in vm]
    moved.cam_pos[:] = [float(v) for v in pos]
    tr2, sh2, _ = sr.transform_f32(rec, sc["transforms"], sc["sh"])
    flags = bo.FLAG_BWD_INFO | (bo.FLAG_MIP if mip else 0)
    a = bo.Render().forward(cam, sc["transforms"], sc["sh"], sc["raw_opac"], flags=flags).image()
    b = bo.Render().forward(moved, tr2, sh2 if rotate_sh else sc["sh"], sc["raw_opac"], flags=flags).image()
    return a, b


@pytest.mark.parametrize("degree,mip,seed", sr.INVARIANT_CASES)
def test_transformed_scene_from_transformed_camera_is_the_same_image(oracle_lib, degree, mip, seed):
    a, b = _oracle_pair(oracle_lib, degree, mip, seed)
    assert float(a[..., 3].max()) > 0.5   # (the scene is in view)
    sr.assert_same_image(a, b)
    if degree >= 1:
        # the control: means and rotations moved, SH left as it was
        a, b = _oracle_pair(oracle_lib, degree, mip, seed, rotate_sh=False)
        diff = float(np.abs(a - b).max())
        print("SH left unrotated: %.3f" % diff)
        assert diff > 0.1
