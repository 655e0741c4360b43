"""The numpy restatement of include/brush_hip_mesh.h (tests/tsdf_ref.py) held to the properties a mesh must have, on an analytic
sphere: 20^3 samples, voxel 0.1, origin -0.95, T = clip((|p| - 0.6) / 0.3, -1, 1) in f32, W = 1.  No GPU."""
import numpy as np

import tsdf_ref as tr

F = np.float32
ORIGIN, VOXEL, N, R = (-0.95, -0.95, -0.95), 0.1, 20, 0.6


def sphere_volume(hide_below=0):
    tw, _ = tr.new_volume((N, N, N), colour=False)
    px, py, pz = tr.sample_positions(ORIGIN, VOXEL, (N, N, N))
    r = np.sqrt(px * px + py * py + pz * pz).astype(F)
    tw[..., 0] = np.clip((r - F(R)) / F(0.3), -1, 1).astype(F)
    tw[..., 1] = 1.0
    tw[:, :, :hide_below, 1] = 0.0
    return tw


def undirected(tris):
    return np.unique(np.sort(tr.directed_edges(tris), axis=1), axis=0)


def test_case_table_is_consistent():
    """Every case lists the cut edges of its mask exactly (once with one or three inside vertices, the quad's four with two), the
    complementary mask lists the same triangles reversed, and the six tetrahedra tile the cube: their corner chains are the six
    monotone paths from (0,0,0) to (1,1,1)."""
    for m in range(1, 15):
        cut = {e for e, (a, b) in enumerate(tr.TET_EDGES) if ((m >> a) & 1) != ((m >> b) & 1)}
        tris = tr.CASES[m]
        assert {e for t in tris for e in t} == cut, m
        assert len(tris) == (2 if len(cut) == 4 else 1)
        if len(tris) == 2:
            assert tris[0][0] == tris[1][0] and tris[0][2] == tris[1][1]   # the shared diagonal
        assert sorted(tr.canonical(np.asarray(tr.CASES[15 - m])).tolist()) == sorted(tr.canonical(np.asarray(tris)[:, ::-1]).tolist()), m
    chains = {tuple(tr.tet_corners(t)) for t in range(6)}
    assert len(chains) == 6
    for t in range(6):
        c = np.asarray(tr.tet_corners(t))
        assert tuple(c[0]) == (0, 0, 0) and tuple(c[3]) == (1, 1, 1) and (np.diff(c, axis=0).sum(axis=1) == 1).all()
        det = np.linalg.det((c[1:] - c[0]).astype(np.float64))
        assert (det < 0) == tr.NEGATIVE[t] and abs(abs(det) - 1.0) < 1e-12


def test_sphere_is_a_closed_oriented_surface():
    """Counts and combinatorics are exact.  The two metric figures were measured with this restatement: volume ratio 0.98610 (a
    piecewise-linear surface inscribed between samples of a convex body loses volume; bound: within 0.02 of 1, below 1), largest
    | |v| - r | = 0.0581 voxel (linear interpolation of a clipped distance that is itself linear in |p|: the error is the f32 rounding
    of t plus the chord sag of the interpolation across a voxel diagonal; bound 0.07 voxel = measured + 20 %)."""
    tw = sphere_volume()
    v, c, t = tr.extract(tw, None, ORIGIN, VOXEL)
    assert c is None and v.dtype == F and t.dtype == np.uint32
    assert (len(v), len(t), len(undirected(t))) == (2030, 4056, 6084)
    assert len(v) - 6084 + len(t) == 2
    e = tr.directed_edges(t)
    key = e[:, 0] * len(v) + e[:, 1]
    assert len(np.unique(key)) == len(key)               # no directed edge twice ...
    assert len(tr.boundary_edges(t)) == 0                # ... and each one's reverse is there: two triangles per edge, opposite ways
    assert np.array_equal(np.unique(t), np.arange(len(v)))
    assert tr.triangle_areas(v, t).min() > 0.0
    ratio = tr.signed_volume(v, t) / (4.0 / 3.0 * np.pi * R ** 3)
    worst = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - R).max() / VOXEL
    print("volume ratio %.5f, largest radial error %.4f voxel" % (ratio, worst))
    assert 0.98 <= ratio < 1.0
    assert worst <= 0.07


def test_vertex_and_triangle_order():
    tw = sphere_volume()
    v, _, t = tr.extract(tw, None, ORIGIN, VOXEL)
    active, valid = tr.classify(tw)
    owner, d = np.nonzero(active.reshape(-1, 7))
    assert len(owner) == len(v) and (np.diff(owner * 7 + d) > 0).all()
    # a vertex lies on its edge: between the owner and the owner + d
    k, j, i = owner // (N * N), (owner // N) % N, owner % N
    lo = np.stack([F(ORIGIN[0]) + F(VOXEL) * i.astype(F), F(ORIGIN[1]) + F(VOXEL) * j.astype(F), F(ORIGIN[2]) + F(VOXEL) * k.astype(F)], axis=1)
    step = np.asarray(tr.D, np.float64)[d] * VOXEL
    rel = (v.astype(np.float64) - lo) / VOXEL
    assert (rel >= -1e-5).all() and (rel <= np.asarray(tr.D)[d] + 1e-5).all() and (np.abs(rel[step == 0]) < 1e-5).all()
    # triangles come cube by cube: the smallest owner among a triangle's vertices never runs ahead of the cube order by more than a cube
    first_owner = owner[t.astype(np.int64)].min(axis=1)
    assert (np.diff(first_owner) >= -(N * N + N + 1)).all()


def test_half_observed_sphere_is_cut_at_the_unobserved_samples():
    tw = sphere_volume(hide_below=8)
    v, _, t = tr.extract(tw, None, ORIGIN, VOXEL)
    assert (len(v), len(t)) == (1302, 2520)
    assert np.array_equal(np.unique(t), np.arange(len(v)))
    assert v[:, 0].min() >= F(ORIGIN[0]) + F(VOXEL) * F(8)
    assert len(tr.boundary_edges(t)) > 0   # open where the field is not observed


def test_unobserved_and_one_sided_volumes_are_empty():
    tw, _ = tr.new_volume((5, 4, 3), colour=False)
    for w in (0.0, 1.0):
        tw[..., 1] = w
        v, _, t = tr.extract(tw, None, (0, 0, 0), 1.0)
        assert len(v) == 0 and t.shape == (0, 3)
    tw[..., 0] = -1.0
    v, _, t = tr.extract(tw, None, (0, 0, 0), 1.0)
    assert len(v) == 0 and len(t) == 0
    tw[1, 1, 1, 0] = 0.0    # exactly 0 is outside: a closed surface around the sample, collapsed onto it (14 edges meet there)
    v, _, t = tr.extract(tw, None, (0, 0, 0), 1.0)
    assert len(v) == 14 and len(t) == 24 and len(tr.boundary_edges(t)) == 0 and (v == 1.0).all()
    tw[1, 1, 1, 0] = 0.5    # an outside pocket in a negative field: the surface faces the pocket, so its signed volume is negative
    v, _, t = tr.extract(tw, None, (0, 0, 0), 1.0)
    assert len(v) == 14 and len(t) == 24 and len(tr.boundary_edges(t)) == 0 and tr.signed_volume(v, t) < 0.0


def test_integration_follows_the_running_mean_and_its_skips():
    """One sample column in front of a camera at the origin looking down +z (vm = identity): the update rule, the clamp, the
    truncation on both sides, the skips and the order dependence, by hand."""
    dims = (2, 2, 9)
    tw, rgb = tr.new_volume(dims)
    cam = dict(vm=[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], fx=4.0, fy=4.0, cx=2.0, cy=2.0, w=4, h=4)
    depth = np.full((4, 4), 1.0, F)
    img = np.zeros((4, 4, 4), F)
    img[..., 0], img[..., 3] = 0.5, 1.0
    args = dict(origin=(0.0, 0.0, 0.25), voxel_size=0.25, trunc=0.5, max_weight=2.0)
    tr.integrate(tw, rgb, cams=[cam], depths=[depth], images=[img], depth_min=0.3, **args)
    z = 0.25 + 0.25 * np.arange(9)
    want = np.minimum(1.0, (1.0 - z) / 0.5)
    seen = (z > 0.3) & (1.0 - z >= -0.5)
    assert np.array_equal(tw[:, 0, 0, 1], seen.astype(F)) and np.array_equal(tw[seen, 0, 0, 0], want[seen].astype(F))
    assert (tw[~seen, 0, 0, 0] == 1.0).all() and np.array_equal(rgb[seen, 0, 0, 0], np.full(seen.sum(), 0.5, F)) and (rgb[~seen] == 0).all()
    # a second and third view at depth 1.25: the mean, then the clamp of W at 2 weighs the newest view 1/3
    d2 = np.full((4, 4), 1.25, F)
    tr.integrate(tw, rgb, cams=[cam, cam], depths=[d2, d2], images=[img, img], depth_min=0.3, **args)
    s1, s2 = F(min(1.0, (1.0 - 0.75) / 0.5)), F(min(1.0, (1.25 - 0.75) / 0.5))
    m = (s1 + s2) / F(2)
    assert tw[2, 0, 0, 1] == 2.0 and tw[2, 0, 0, 0] == (F(2) * m + s2) / F(3)
    # skips leave the bits alone: depth 0, NaN, negative, beyond depth_max, low alpha
    before = tw.copy()
    for bad in (0.0, np.nan, -1.0, np.inf, 3.0):
        tr.integrate(tw, rgb, cams=[cam], depths=[np.full((4, 4), bad, F)], images=[img], depth_max=2.0, **args)
    low = img.copy()
    low[..., 3] = 0.25
    tr.integrate(tw, rgb, cams=[cam], depths=[depth], images=[low], **args)
    assert np.array_equal(before.view(np.uint32), tw.view(np.uint32))


def test_ply_bytes():
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    c = np.asarray([[0.5 / 255, 1.5 / 255, 2.5 / 255], [-1.0, 2.0, np.nan], [0.25, 0.5, 1.0]], F)
    t = np.asarray([[0, 1, 2]], np.uint32)
    data = tr.mesh_to_ply(v, c, t)
    head, body = data.split(b"end_header\n")
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\ncomment Exported from Brush\nelement vertex 3\n")
    assert b"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 1\nproperty list uchar uint vertex_indices\n" in head
    assert len(body) == 3 * 15 + 13
    assert list(body[12:15]) == [0, 2, 2] and list(body[27:30]) == [0, 255, 0] and list(body[42:45]) == [64, 128, 255]   # half to even
    assert body[45] == 3 and np.frombuffer(body[46:], "<u4").tolist() == [0, 1, 2]
    plain = tr.mesh_to_ply(v, None, t)
    assert b"red" not in plain and len(plain.split(b"end_header\n")[1]) == 3 * 12 + 13
