"""The scenes the sparse-volume tests share (tests/test_sptsdf_ref.py on the CPU, tests/test_gpu_sparse_mesh.py on the GPU), computed
once and never modified.  The views are tests/test_gpu_mesh.py's: cameras around an analytic sphere, 40x30 depth maps with a block of
zeros, a NaN and a negative pixel, images with alpha around the threshold.

THREE: three views on a 40x33x26 grid (5x5x4 blocks whose last blocks hold 8, 1 and 2 samples per axis), placed so that the sphere
       leaves the grid through the ragged +y and +z faces: rays end outside, and the surface crosses boundary blocks.
SPHERE: eleven views all round the sphere on test_gpu_mesh's own 24x20x16 grid."""
import numpy as np

import sptsdf_ref as sr
import test_gpu_mesh as tgm
import tsdf_ref as tr

F = np.float32
ALPHA_MIN, DEPTH_MIN = tgm.ALPHA_MIN, tgm.DEPTH_MIN
VOXEL = tgm.VOXEL
TRUNC = float(4 * F(VOXEL))
SCENES = {
    "three": dict(dims=(40, 33, 26), origin=(-1.6, -2.3, -1.05), n_views=3),
    "sphere": dict(dims=tgm.DIMS, origin=tgm.ORIGIN, n_views=11),
}
_CACHE = {}


def cam_dict(cam):
    d = tgm._cam_dict(cam)
    d["cam_pos"] = [cam.cam_pos[n] for n in range(3)]
    return d


def views(n):
    """(BhCamera list, depth maps, images) of tgm._views(n)."""
    return tgm._views(n)


def marked(name, with_images=True, n_views=None):
    """[NBZ,NBY,NBX] bool: the restatement's marks of the scene's views."""
    sc = SCENES[name]
    n_views = sc["n_views"] if n_views is None else n_views
    key = ("marked", name, with_images, n_views)
    if key not in _CACHE:
        cams, depths, images = views(sc["n_views"])
        nbx, nby, nbz = sr.block_dims(sc["dims"])
        m = np.zeros((nbz, nby, nbx), bool)
        sr.mark(m, sc["origin"], VOXEL, sc["dims"], TRUNC, [cam_dict(c) for c in cams[:n_views]], depths[:n_views], images[:n_views] if with_images else None,
                alpha_min=ALPHA_MIN)
        m.setflags(write=False)
        _CACHE[key] = m
    return _CACHE[key]


def fused(name, colour=True, with_images=True, max_weight=64.0):
    """The dense restatement's volume after the scene's views in order: (tw, rgb)."""
    key = ("fused", name, colour, with_images, max_weight)
    if key not in _CACHE:
        sc = SCENES[name]
        cams, depths, images = views(sc["n_views"])
        tw, rgb = tr.new_volume(sc["dims"], colour)
        tr.integrate(tw, rgb if with_images else None, sc["origin"], VOXEL, TRUNC, max_weight, [cam_dict(c) for c in cams], depths, images if with_images else None,
                     depth_min=DEPTH_MIN, alpha_min=ALPHA_MIN)
        tw.setflags(write=False)
        if rgb is not None:
            rgb.setflags(write=False)
        _CACHE[key] = (tw, rgb)
    return _CACHE[key]


def containment(name):
    """(needed, allocated): the blocks that hold a band sample of some view plus their 26 neighbours, and the blocks mark + commit(1)
    allocate.  The sparse mesh is the dense one where needed is a subset of allocated."""
    key = ("containment", name)
    if key not in _CACHE:
        sc = SCENES[name]
        cams, depths, images = views(sc["n_views"])
        band = sr.band_blocks(sc["origin"], VOXEL, sc["dims"], TRUNC, [cam_dict(c) for c in cams], depths, images, depth_min=DEPTH_MIN, alpha_min=ALPHA_MIN)
        _CACHE[key] = (sr.dilate(band, 1), sr.dilate(marked(name), 1))
    return _CACHE[key]
