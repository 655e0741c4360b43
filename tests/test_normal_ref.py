"""tests/normal_ref.py pinned without a GPU: its RGBA is oracle/autograd_ref.render's exactly (pinhole, a fisheye model, Mip), its
accumulated normals are 2 rgb - A of the scene coloured by (1 + n) / 2, the splat normals are unit, face the camera, ignore the
quaternion's sign and length and differentiate as central differences say, and depth_to_normal returns the normal of an analytic
plane with exact zeros on the border and around a hole."""
import numpy as np
import pytest
import torch

from oracle import autograd_ref
import normal_ref
import util

CASES = [("pinhole", False), ("kb4", False), ("pinhole", True)]
C0 = 0.2820947917738781


def _case(model, seed=3, n=6):
    sc = util.random_scene(seed, n)
    camp = dict(util.random_camera(seed))
    if model != "pinhole":
        camp["model"], camp["dist"] = util.REF_LENSES[model]
    return sc, camp


def _tensors(sc):
    # (leaves that require grad: the lens models take their Jacobian by autograd)
    return [torch.tensor(np.asarray(sc[k], np.float64), requires_grad=True) for k in ("transforms", "sh", "raw_opac")]


@pytest.mark.parametrize("model,mip", CASES)
def test_rgba_is_autograd_refs_exactly(model, mip):
    w = h = 40
    for seed in (3, 7):
        sc, camp = _case(model, seed, 2 + seed % 7)
        intr = normal_ref.intrinsics(camp, w, h)
        tr, sh, op = _tensors(sc)
        bg = (0.1, 0.3, 0.2)
        a = autograd_ref.render(tr, sh, op, camp, w, h, bg, intr, mip)
        out = normal_ref.render(tr, sh, op, camp, w, h, bg, intr, mip)
        assert torch.equal(a, out["img"])
        assert torch.equal(out["alpha"], a[..., 3])
    sc, camp = util.base_scene(), util.STD_CAM
    tr, sh, op = _tensors(sc)
    assert torch.equal(autograd_ref.render(tr, sh, op, camp, 32, 32), normal_ref.render(tr, sh, op, camp, 32, 32)["img"])


@pytest.mark.parametrize("model,mip", CASES)
def test_accumulated_normals_are_the_image_of_the_normal_coloured_scene(model, mip):
    """N = 2 rgb - A where the colour of splat i is (1 + n_i) / 2: sh0 = ((1 + n) / 2 - 0.5) / C0 at degree 0, black background."""
    w = h = 40
    sc, camp = _case(model, 7, 9)
    intr = normal_ref.intrinsics(camp, w, h)
    tr, sh, op = _tensors(sc)
    with torch.enable_grad():
        out = normal_ref.render(tr, sh, op, camp, w, h, intrinsics=intr, mip=mip)
    n = out["splat_normals"].detach()
    sh_n = (((1.0 + n) / 2.0 - 0.5) / C0)[:, None, :].clone().requires_grad_(True)
    with torch.enable_grad():
        img = autograd_ref.render(tr, sh_n, op, camp, w, h, (0.0, 0.0, 0.0), intr, mip).detach()
    want = 2.0 * img[..., :3] - img[..., 3:4]
    assert float(out["alpha"].detach().max()) > 0.1 and float(out["normal"].detach().abs().max()) > 0.05
    assert float((out["normal"].detach() - want).abs().max()) <= 1e-12
    u = out["unit"].detach()
    length = u.norm(dim=-1)
    seen = out["normal"].detach().norm(dim=-1) > 0
    assert bool(((length[seen] - 1.0).abs() <= 1e-12).all()) and bool((u[~seen] == 0).all())


def test_splat_normals_are_unit_face_the_camera_and_ignore_the_quaternions_sign_and_length():
    sc = util.random_scene(11, 40)
    camp = util.random_camera(11)
    rc, tc = normal_ref.camera_rt(camp, 40, 40)
    tr = torch.tensor(np.asarray(sc["transforms"], np.float64))
    n, k, facing = normal_ref.splat_normals(tr, rc, tc)
    assert bool(((n.norm(dim=1) - 1.0).abs() <= 1e-12).all())
    mean_c = tr[:, :3] @ rc.T + tc
    assert bool(((n * mean_c).sum(1) <= 0).all())
    assert set(k.tolist()) == {0, 1, 2}
    assert bool((k == torch.argmin(tr[:, 7:10], dim=1)).all())
    for factor in (-1.0, 3.0):
        t2 = tr.clone()
        t2[:, 3:7] *= factor
        n2, k2, _ = normal_ref.splat_normals(t2, rc, tc)
        assert bool((k2 == k).all()) and float((n2 - n).abs().max()) <= 1e-14
    # an exact tie takes the lowest index
    t3 = tr.clone()
    t3[:, 7:10] = -1.0
    assert bool((normal_ref.splat_normals(t3, rc, tc)[1] == 0).all())
    t3[:, 7] = -0.5
    assert bool((normal_ref.splat_normals(t3, rc, tc)[1] == 1).all())


def test_splat_normal_autograd_agrees_with_central_differences_and_reaches_the_quaternion_only():
    sc = util.random_scene(5, 6)
    camp = util.random_camera(5)
    rc, tc = normal_ref.camera_rt(camp, 40, 40)
    rng = np.random.default_rng(4)
    v = torch.tensor(rng.uniform(-1.0, 1.0, (6, 3)))

    def value(t):
        return (normal_ref.splat_normals(t, rc, tc)[0] * v).sum()
    tr = torch.tensor(np.asarray(sc["transforms"], np.float64), requires_grad=True)
    value(tr).backward()
    g = tr.grad
    assert float(g[:, :3].abs().max()) == 0.0 and float(g[:, 7:].abs().max()) == 0.0 and float(g[:, 3:7].abs().max()) > 0.0
    eps = 1e-6
    for i in range(6):
        for c in range(3, 7):
            def pert(d):
                x = tr.detach().clone()
                x[i, c] += d
                return float(value(x))
            num = (pert(eps) - pert(-eps)) / (2 * eps)
            an = float(g[i, c])
            assert abs(num - an) <= 1e-6 * max(abs(num), abs(an)) + 1e-9, (i, c, num, an)


def _plane_depth(h, w, fx, fy, cx, cy, nrm, d0):
    """z-depth of the plane n . P = n_z d0 (through (0, 0, d0)) along the rays of the pixel centres."""
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    kx, ky = (xs + 0.5 - cx) / fx, (ys + 0.5 - cy) / fy
    return nrm[2] * d0 / (nrm[0] * kx + nrm[1] * ky + nrm[2])


def test_depth_to_normal_of_a_tilted_plane_with_a_hole():
    h, w = 21, 37
    fx, fy, cx, cy = 40.0, 42.0, 18.2, 10.1
    nrm = torch.tensor([0.3, -0.2, -1.0], dtype=torch.float64)
    nrm = nrm / nrm.norm()
    depth = _plane_depth(h, w, fx, fy, cx, cy, nrm, 4.0)
    assert float(depth.min()) > 1.0
    depth[7, 9] = 0.0
    depth[12, 30] = float("nan")
    out, valid = normal_ref.depth_to_normal(depth, fx, fy, cx, cy)
    want = torch.ones((h, w), dtype=torch.bool)
    want[0, :] = want[-1, :] = want[:, 0] = want[:, -1] = False
    for (y, x) in ((7, 9), (12, 30)):
        for (dy, dx) in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
            want[y + dy, x + dx] = False
    assert torch.equal(valid, want)
    assert bool((out[~valid] == 0).all()) and bool(torch.isfinite(out).all())
    # a plane is reproduced exactly by central differences: the plane's own normal, facing the camera (-z)
    assert float((out[valid] - nrm).abs().max()) <= 1e-12
    assert float(nrm[2]) < 0
    # the gradient exists, is finite and is zero at pixels no valid stencil reads
    d = depth.clone().requires_grad_(True)
    o, _ = normal_ref.depth_to_normal(d, fx, fy, cx, cy)
    (o * torch.tensor(np.random.default_rng(2).uniform(-1, 1, (h, w, 3)))).sum().backward()
    assert bool(torch.isfinite(d.grad).all()) and float(d.grad.abs().max()) > 0
    assert float(d.grad[0, 0]) == 0.0 and float(d.grad[7, 9]) == 0.0
