"""Mesh extraction on the GPU (include/brush_hip_mesh.h) against the float32 numpy restatement tests/tsdf_ref.py:
integration bit for bit (with and without colour, skips, batching, the weight clamp, view order), extraction (counts, vertices and
colours bit-equal in order, triangles equal after rotating each to its smallest index and sorting rows, closedness and orientation
rechecked on the GPU's output), ragged and degenerate grids, the refusals, the PLY bytes, and fuse_views on a small scene.

Shapes are the smallest at which an index or order mistake shows: a 24x20x16 grid (no two dimensions equal, a non-zero origin: one
block row of the integration kernel is ragged in x and y), 67x5x3 (more than one block along x, a ragged tail), 2x2x2 (one cube)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import tsdf_ref as tr

pytestmark = pytest.mark.gpu
F = np.float32
DIMS, ORIGIN, VOXEL = (24, 20, 16), (-0.62, -0.96, -0.1), 0.08
CENTRE, RADIUS = np.asarray([0.3, -0.2, 0.5]), 0.5
W, H = 40, 30
ALPHA_MIN, DEPTH_MIN = 0.5, 0.25
_CACHE = {}


@pytest.fixture
def ctx(dev):
    import brush_amd as ba
    c = ba.Context(dev)
    yield c
    c.close()


def _bh_camera(pos, target, w=W, h=H, f=38.0, cx=None, cy=None, roll=0.35):
    """A pinhole BhCamera at `pos` looking at `target`, rolled about its axis, with an off-centre principal point."""
    from brush_amd import _ffi
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    fwd = (target - pos) / np.linalg.norm(target - pos)
    helper = np.asarray([math.sin(roll), math.cos(roll), 0.1])
    right = np.cross(helper, fwd)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    rwc = np.stack([right, down, fwd])   # world -> camera rows
    t = -rwc @ pos
    cam = _ffi.BhCamera()
    for c in range(3):
        for r in range(3):
            cam.vm[3 * c + r] = rwc[r, c]
    for r in range(3):
        cam.vm[9 + r] = t[r]
        cam.cam_pos[r] = pos[r]
    cam.fx, cam.fy = f, f * 1.07
    cam.cx = 0.5 * w - 2.3 if cx is None else cx
    cam.cy = 0.5 * h + 1.7 if cy is None else cy
    cam.img_w, cam.img_h, cam.model = w, h, _ffi.CAMERA_PINHOLE
    return cam


def _cam_dict(cam):
    return dict(vm=[cam.vm[n] for n in range(12)], fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, w=cam.img_w, h=cam.img_h)


def _sphere_depth(cam):
    """z-depth of the analytic sphere through every pixel centre (0 where the ray misses), f64 -> f32."""
    vm = np.asarray([cam.vm[n] for n in range(12)], np.float64).reshape(4, 3).T   # 3x4
    c = vm[:, :3] @ CENTRE + vm[:, 3]
    assert c[2] > RADIUS, "the camera does not look at the sphere"
    ys, xs = np.mgrid[0:cam.img_h, 0:cam.img_w]
    d = np.stack([(xs + 0.5 - cam.cx) / cam.fx, (ys + 0.5 - cam.cy) / cam.fy, np.ones(xs.shape)], axis=-1)
    a, b, cc = (d * d).sum(-1), (d * c).sum(-1), c @ c - RADIUS ** 2
    disc = b * b - a * cc
    t = np.where(disc > 0, (b - np.sqrt(np.maximum(disc, 0))) / a, 0.0)
    return t.astype(F)


def _views(n=3):
    """n cameras around the sphere with their depth maps (a block of zeros, one NaN, one negative pixel) and images (alpha around
    ALPHA_MIN); computed once, shared, never modified."""
    if ("views", n) not in _CACHE:
        rng = np.random.default_rng(11)
        cams, depths, images = [], [], []
        for v in range(n):
            ang = 0.9 * v + 0.2
            pos = CENTRE + np.asarray([1.7 * math.cos(ang), 0.5 * math.sin(1.3 * v), 1.7 * math.sin(ang)]) * (1.0 - 0.04 * (v % 3))
            cam = _bh_camera(pos, CENTRE + 0.05 * np.asarray([math.sin(v), math.cos(v), 0.0]), roll=0.35 + 0.2 * v)
            depth = _sphere_depth(cam)
            assert (depth > 0).sum() > 100
            depth[12:16, 18:23] = 0.0
            depth[14, 10], depth[15, 11] = np.nan, -0.7
            img = rng.uniform(0.0, 1.0, (H, W, 4)).astype(F)
            img[..., 3] = rng.uniform(0.3, 1.0, (H, W)).astype(F)
            for a in (depth, img):
                a.setflags(write=False)
            cams.append(cam); depths.append(depth); images.append(img)
        _CACHE[("views", n)] = (cams, depths, images)
    return _CACHE[("views", n)]


def _ref_fused(n=3, colour=True, max_weight=64.0, order=None):
    key = ("fused", n, colour, max_weight, order)
    if key not in _CACHE:
        cams, depths, images = _views(n)
        idx = list(order) if order is not None else list(range(n))
        tw, rgb = tr.new_volume(DIMS, colour)
        tr.integrate(tw, rgb, ORIGIN, VOXEL, 4 * F(VOXEL), max_weight, [_cam_dict(cams[i]) for i in idx], [depths[i] for i in idx],
                     [images[i] for i in idx], depth_min=DEPTH_MIN, alpha_min=ALPHA_MIN)
        tw.setflags(write=False)
        if rgb is not None:
            rgb.setflags(write=False)
        _CACHE[key] = (tw, rgb)
    return _CACHE[key]


def _volume(ctx, dims=DIMS, origin=ORIGIN, voxel=VOXEL, colour=True, max_weight=64.0, trunc=None):
    import brush_amd as ba
    return ba.TsdfVolume(origin, voxel, dims, trunc=float(4 * F(voxel)) if trunc is None else trunc, max_weight=max_weight, colour=colour, ctx=ctx)


def _integrate(vol, idx, n=3, with_images=True):
    cams, depths, images = _views(n)
    dev = vol.device
    vol.integrate([torch.tensor(depths[i], device=dev) for i in idx], [cams[i] for i in idx],
                  [torch.tensor(images[i], device=dev) for i in idx] if with_images else None, depth_min=DEPTH_MIN, alpha_min=ALPHA_MIN)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(vol, tw, rgb):
    got = vol.tw.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(tw)), "%d samples differ" % (_bits(got) != _bits(tw)).any(axis=-1).sum()
    if rgb is not None:
        assert np.array_equal(_bits(vol.rgb.cpu().numpy()), _bits(rgb))


@pytest.mark.parametrize("colour", [True, False])
def test_integrate_matches_the_restatement_bit_for_bit(ctx, colour):
    tw, rgb = _ref_fused(3, colour)
    seen = tw[..., 1] > 0
    assert 500 < seen.sum() < seen.size - 500 and (tw[..., 1] == 3).any() and (tw[..., 0][seen] < 0).any()
    vol = _volume(ctx, colour=colour)
    assert (vol.tw.cpu().numpy() == np.asarray([1.0, 0.0], F)).all()
    _integrate(vol, [0, 1, 2])
    _same(vol, tw, rgb)
    # samples behind every camera's depth_min plane or outside every frustum were left as cleared, bit for bit
    got = vol.tw.cpu().numpy()
    assert np.array_equal(_bits(got[~seen]), np.broadcast_to(_bits(np.asarray([1.0, 0.0], F)), got[~seen].shape))
    if colour:
        assert (vol.rgb.cpu().numpy()[~seen] == 0).all()


def test_integrate_without_images_skips_the_alpha_test_and_the_colour(ctx):
    cams, depths, _ = _views(3)
    tw, rgb = tr.new_volume(DIMS, True)
    tr.integrate(tw, None, ORIGIN, VOXEL, 4 * F(VOXEL), 64.0, [_cam_dict(c) for c in cams], depths, None, depth_min=DEPTH_MIN)
    assert (tw[..., 1] > 0).sum() > (_ref_fused(3)[0][..., 1] > 0).sum()   # the alpha test removed pixels
    vol = _volume(ctx)
    _integrate(vol, [0, 1, 2], with_images=False)
    _same(vol, tw, rgb)


def test_a_batch_of_eleven_views_equals_eleven_single_calls(ctx):
    tw, rgb = _ref_fused(11, True, 4.0)
    assert tw[..., 1].max() == 4.0 and (tw[..., 1] == 4.0).sum() > 100   # the clamp is reached
    batched, single = _volume(ctx, max_weight=4.0), _volume(ctx, max_weight=4.0)
    _integrate(batched, list(range(11)), 11)
    for i in range(11):
        _integrate(single, [i], 11)
    _same(batched, tw, rgb)
    _same(single, tw, rgb)


def test_the_result_depends_on_view_order_as_the_restatement_says(ctx):
    fwd, rev = _ref_fused(3, True, 2.0, (0, 1, 2)), _ref_fused(3, True, 2.0, (2, 1, 0))
    assert not np.array_equal(_bits(fwd[0]), _bits(rev[0]))
    for order, ref in (((0, 1, 2), fwd), ((2, 1, 0), rev)):
        vol = _volume(ctx, max_weight=2.0)
        _integrate(vol, list(order))
        _same(vol, *ref)


def _check_extract(vol, tw, rgb, origin, voxel, closed=False):
    want_v, want_c, want_t = tr.extract(tw, rgb, origin, voxel)
    assert vol.count() == (len(want_v), len(want_t))
    v, c, t = vol.extract_mesh()
    v, t = v.cpu().numpy(), t.cpu().numpy().view(np.uint32)
    assert v.shape == want_v.shape and t.shape == want_t.shape
    assert np.array_equal(_bits(v), _bits(want_v))
    if rgb is not None:
        assert np.array_equal(_bits(c.cpu().numpy()), _bits(want_c))
    else:
        assert c is None
    if len(t):
        assert t.max() < len(v) and np.array_equal(np.unique(t), np.arange(len(v)))
    assert np.array_equal(tr.canonical(t), tr.canonical(want_t))
    if closed:
        e = tr.directed_edges(t)
        assert len(np.unique(e[:, 0] * len(v) + e[:, 1])) == len(e) and len(tr.boundary_edges(t)) == 0 and tr.signed_volume(v, t) > 0
    again = vol.extract_mesh()
    assert np.array_equal(_bits(again[0].cpu().numpy()), _bits(v)) and np.array_equal(again[2].cpu().numpy().view(np.uint32), t)
    return v, c, t


def _analytic_sphere(hide_below=0):
    n = 20
    tw, _ = tr.new_volume((n, n, n), False)
    px, py, pz = tr.sample_positions((-0.95,) * 3, 0.1, (n, n, n))
    r = np.sqrt(px * px + py * py + pz * pz).astype(F)
    tw[..., 0] = np.clip((r - F(0.6)) / F(0.3), -1, 1).astype(F)
    tw[..., 1] = 1.0
    tw[:, :, :hide_below, 1] = 0.0
    return tw


@pytest.mark.parametrize("hide_below,counts", [(0, (2030, 4056)), (8, (1302, 2520))])
def test_extract_the_analytic_sphere(ctx, hide_below, counts):
    tw = _analytic_sphere(hide_below)
    vol = _volume(ctx, (20, 20, 20), (-0.95,) * 3, 0.1, colour=False)
    vol.tw.copy_(torch.from_numpy(tw))
    v, _, t = _check_extract(vol, tw, None, (-0.95,) * 3, 0.1, closed=hide_below == 0)
    assert (len(v), len(t)) == counts
    if hide_below:
        assert v[:, 0].min() >= F(-0.95) + F(0.1) * F(8)


def test_extract_the_fused_volume_with_colours(ctx):
    tw, rgb = _ref_fused(3, True)
    vol = _volume(ctx)
    _integrate(vol, [0, 1, 2])
    v, c, t = _check_extract(vol, tw, rgb, ORIGIN, VOXEL)
    assert len(t) > 200
    # the fused surface is the sphere the depth maps were cast from, to a fraction of a voxel
    err = np.abs(np.linalg.norm(v.astype(np.float64) - CENTRE, axis=1) - RADIUS) / VOXEL
    print("fused sphere: %d vertices, %d triangles, radial error mean %.3f / max %.3f voxel" % (len(v), len(t), err.mean(), err.max()))


def test_ragged_and_degenerate_grids(ctx):
    rng = np.random.default_rng(5)
    # 67 x 5 x 3 cut by a plane, a few samples unobserved
    dims, origin, voxel = (67, 5, 3), (0.5, -1.0, 2.0), 0.25
    px, py, pz = tr.sample_positions(origin, voxel, dims)
    tw, rgb = tr.new_volume(dims, True)
    tw[..., 0] = np.clip((F(0.11) * px + F(0.7) * py + F(0.5) * pz - F(1.61)) / F(1.0), -1, 1).astype(F)
    tw[..., 1] = (rng.uniform(size=tw.shape[:3]) > 0.03).astype(F)
    rgb[...] = rng.uniform(size=rgb.shape).astype(F)
    vol = _volume(ctx, dims, origin, voxel)
    vol.tw.copy_(torch.from_numpy(tw)); vol.rgb.copy_(torch.from_numpy(rgb))
    v, _, t = _check_extract(vol, tw, rgb, origin, voxel)
    assert len(t) > 300
    # 2 x 2 x 2: one cube, every sign pattern of its corners
    for pattern in (0x01, 0x17, 0x3C, 0x69, 0x80, 0xFE, 0xA5):
        tw, _ = tr.new_volume((2, 2, 2), False)
        bits = np.asarray([(pattern >> n) & 1 for n in range(8)], bool).reshape(2, 2, 2)
        tw[..., 0] = np.where(bits, -rng.uniform(0.1, 1.0, (2, 2, 2)), rng.uniform(0.1, 1.0, (2, 2, 2))).astype(F)
        tw[..., 1] = 1.0
        vol = _volume(ctx, (2, 2, 2), (0.0, 0.0, 0.0), 1.0, colour=False)
        vol.tw.copy_(torch.from_numpy(tw))
        _, _, t = _check_extract(vol, tw, None, (0.0, 0.0, 0.0), 1.0)
        assert len(t) > 0
    # an all-positive grid: counts 0, and extract succeeds with null outputs
    vol = _volume(ctx, (9, 4, 3), (0.0, 0.0, 0.0), 1.0, colour=False)
    vol.tw[..., 1] = 1.0
    assert vol.count() == (0, 0)
    g = vol.grid()
    nv, nt = C.c_uint32(9), C.c_uint32(9)
    assert ctx.lib.bh_tsdf_extract(ctx._h, C.byref(g), None, None, None, 0, 0, C.byref(nv), C.byref(nt)) == 0 and (nv.value, nt.value) == (0, 0)
    v, c, t = vol.extract_mesh()
    assert v.shape == (0, 3) and t.shape == (0, 3)


def test_refusals(ctx):
    from brush_amd import _ffi
    tw = _analytic_sphere()
    vol = _volume(ctx, (20, 20, 20), (-0.95,) * 3, 0.1, colour=False)
    vol.tw.copy_(torch.from_numpy(tw))
    g = vol.grid()
    nv, nt = C.c_uint32(), C.c_uint32()
    verts = torch.full((2030, 3), 7.0, device=vol.device)
    tris = torch.full((4056, 3), 7, dtype=torch.int32, device=vol.device)
    lib, h = ctx.lib, ctx._h
    for cap_v, cap_t in ((2029, 4056), (2030, 4055), (0, 0)):   # capacities too small: refused, the counts returned, nothing written
        nv.value = nt.value = 0
        assert lib.bh_tsdf_extract(h, C.byref(g), verts.data_ptr(), None, tris.data_ptr(), cap_v, cap_t, C.byref(nv), C.byref(nt)) == -1
        assert (nv.value, nt.value) == (2030, 4056)
    assert (verts == 7.0).all() and (tris == 7).all()
    colours = torch.empty((2030, 3), device=vol.device)
    assert lib.bh_tsdf_extract(h, C.byref(g), verts.data_ptr(), colours.data_ptr(), tris.data_ptr(), 2030, 4056, C.byref(nv), C.byref(nt)) == -1   # no rgb
    assert lib.bh_tsdf_extract(h, C.byref(g), verts.data_ptr(), None, tris.data_ptr(), 2030, 4056, C.byref(nv), C.byref(nt)) == 0
    # the grid
    for field, value in (("nx", 1), ("nz", 0), ("trunc", 0.0), ("trunc", -1.0), ("trunc", math.nan), ("voxel_size", 0.0), ("max_weight", 0.5), ("tw", None)):
        bad = vol.grid()
        setattr(bad, field, value)
        assert lib.bh_tsdf_clear(h, C.byref(bad)) == -1, field
        assert lib.bh_tsdf_extract_count(h, C.byref(bad), C.byref(nv), C.byref(nt)) == -1, field
    bad = vol.grid()
    bad.nx, bad.ny, bad.nz = 2048, 1024, 1024   # 2^31 samples
    assert lib.bh_tsdf_clear(h, C.byref(bad)) == -1
    # the views: a lens model other than the pinhole, a tile-row window, a null depth map
    cams, depths, _ = _views(3)
    d = torch.tensor(depths[0], device=vol.device)
    cfg = _ffi.BhTsdfIntegrateConfig(0.0, math.inf, 0.5, 0)
    for change in ("model", "window", "depth"):
        arr = (_ffi.BhCamera * 2)(cams[0], cams[1])
        ptrs = (C.c_void_p * 2)(d.data_ptr(), d.data_ptr())
        if change == "model":
            arr[1].model = _ffi.CAMERA_KANNALA_BRANDT_4
        elif change == "window":
            arr[1].tile_row_begin, arr[1].tile_row_end = 0, 1
        else:
            ptrs[1] = None
        assert lib.bh_tsdf_integrate(h, C.byref(g), 2, arr, ptrs, None, C.byref(cfg)) == -1, change
    assert np.array_equal(_bits(vol.tw.cpu().numpy()), _bits(tw))   # nothing was launched


def _read_ply(data):
    """A 20-line reader of the mesh PLY: (vertex count, vertex properties, face count, body)."""
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[2] == "comment Exported from Brush" and lines[-1] == ""
    elements, props = [], {}
    for line in lines[3:-1]:
        words = line.split()
        if words[0] == "element":
            elements.append((words[1], int(words[2])))
            props[words[1]] = []
        else:
            assert words[0] == "property"
            props[elements[-1][0]].append(" ".join(words[1:]))
    assert [e[0] for e in elements] == ["vertex", "face"] and props["face"] == ["list uchar uint vertex_indices"]
    return elements[0][1], props["vertex"], elements[1][1], body


def test_mesh_ply_bytes(ctx):
    import brush_amd as ba
    tw, rgb = _ref_fused(3, True)
    want_v, want_c, want_t = tr.extract(tw, rgb, ORIGIN, VOXEL)
    want_c = want_c.copy()
    want_c[:7] = np.asarray([[0.1, 0.3, 0.5], [-1.0, 2.0, np.nan], [0.5 / 255, 1.5 / 255, 2.5 / 255], [1.0, 0.0, 0.999], [0.9, 0.7, 0.2], [0.498, 0.502, 0.25],
                             [1e-9, 0.75, 0.125]], F)   # ties (half to even), the clamp, not a number
    dev = ctx.device
    v, c, t = torch.from_numpy(want_v).to(dev), torch.from_numpy(want_c).to(dev), torch.from_numpy(want_t.view(np.int32)).to(dev)
    for colours, ref_c in ((c, want_c), (None, None)):
        data = ba.mesh_to_ply(v, t, colours, ctx=ctx)
        assert data == tr.mesh_to_ply(want_v, ref_c, want_t)
        n_v, vprops, n_t, body = _read_ply(data)
        assert (n_v, n_t) == (len(want_v), len(want_t))
        assert vprops == ["float x", "float y", "float z"] + (["uchar red", "uchar green", "uchar blue"] if colours is not None else [])
        row = 15 if colours is not None else 12
        assert len(body) == n_v * row + n_t * 13
        rows = np.frombuffer(body[:n_v * row], np.uint8).reshape(n_v, row)
        assert np.array_equal(rows[:, :12].copy().view("<f4").view(np.uint32), _bits(want_v))
        faces = np.frombuffer(body[n_v * row:], np.uint8).reshape(n_t, 13)
        assert (faces[:, 0] == 3).all() and np.array_equal(faces[:, 1:].copy().view("<u4"), want_t)
    # the volume's own export is the same file
    vol = _volume(ctx)
    _integrate(vol, [0, 1, 2])
    mesh = vol.extract_mesh()
    assert vol.to_ply() == ba.mesh_to_ply(mesh[0], mesh[2], mesh[1], ctx=ctx) == tr.mesh_to_ply(*tr.extract(tw, rgb, ORIGIN, VOXEL))
    assert ba.mesh_to_ply(v[:0], t[:0], None, ctx=ctx) == tr.mesh_to_ply(want_v[:0], None, want_t[:0])


@pytest.mark.parametrize("mode", ["expected", "median"])
def test_fuse_views_on_a_small_scene(ctx, mode):
    """About 300 splats on a sphere of radius 1 around (0, 0, 3), four cameras of 64x48.  fuse_views' volume is bit-equal to the one
    fused by hand (forward, RenderNode.depth, bh_tsdf_integrate) and to the restatement run on the depth maps and images read back.
    Measured on an MI355X, not a pass / fail figure: the mean distance of the mesh's vertices from the shell is 1.389 voxel with
    expected depth (2794 vertices, 5182 triangles) and 1.554 voxel with median depth (3201 vertices, 5698 triangles): the splats are
    blobs of 1.2 to 2 voxels, so the depth they blend to sits about one splat radius in front of the shell."""
    import brush_amd as ba
    from brush_amd import _ffi
    n, w, h = 300, 64, 48
    rng = np.random.default_rng(3)
    p = rng.normal(size=(n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    centre = np.asarray([0.0, 0.0, 3.0])
    tf = np.zeros((n, 10), F)
    tf[:, :3] = p + centre
    tf[:, 3] = 1.0
    tf[:, 7:] = np.log(rng.uniform(0.12, 0.2, (n, 3)))
    splats = ba.Splats(tf, rng.uniform(0.0, 1.5, (n, 1, 3)).astype(F), np.full(n, 4.0, F), device=ctx.device)
    cams = [ba.Camera(position=pos, fov_x=0.9, fov_y=0.7, center_uv=(0.52, 0.47)) for pos in ((0.6, 0.3, 0.0), (-0.6, 0.3, 0.1), (0.5, -0.4, -0.1), (-0.4, -0.5, 0.0))]
    dims, origin, voxel = (26, 27, 28), (-1.25, -1.3, 1.65), 0.1
    fused = ba.fuse_views(splats, cams, (w, h), _volume(ctx, dims, origin, voxel, trunc=0.4), depth_mode=mode)
    by_hand = _volume(ctx, dims, origin, voxel, trunc=0.4)
    depths, images, bh_cams = [], [], (_ffi.BhCamera * 4)()
    for v, cam in enumerate(cams):
        node = ba.render_splats_diff(splats, cam, (w, h), ctx=ctx)
        depths.append(node.depth(mode))
        images.append(node.img.clone())
        bh_cams[v] = cam.uniforms((w, h))
    g = by_hand.grid()
    cfg = _ffi.BhTsdfIntegrateConfig(0.0, math.inf, 0.5, 0)
    dptr, iptr = (C.c_void_p * 4)(*[d.data_ptr() for d in depths]), (C.c_void_p * 4)(*[i.data_ptr() for i in images])
    ctx.check(ctx.lib.bh_tsdf_integrate(ctx._h, C.byref(g), 4, bh_cams, dptr, iptr, C.byref(cfg)))
    tw, rgb = tr.new_volume(dims, True)
    tr.integrate(tw, rgb, origin, voxel, 0.4, 64.0, [_cam_dict(c) for c in bh_cams], [d.cpu().numpy() for d in depths], [i.cpu().numpy() for i in images])
    assert (tw[..., 1] > 0).sum() > 2000
    _same(fused, tw, rgb)
    _same(by_hand, tw, rgb)
    v, c, t = fused.extract_mesh()
    assert len(v) > 300 and len(t) > 300 and c.shape == v.shape
    dist = np.abs(np.linalg.norm(v.cpu().numpy().astype(np.float64) - centre, axis=1) - 1.0) / voxel
    print("fuse_views(%s): %d vertices, %d triangles, mean distance from the shell %.3f voxel" % (mode, len(v), len(t), dist.mean()))
