"""The image half of LoadImage::load on the GPU (include/brush_hip_image.h): bh_resize_u8 and
bh_uploader_commit_view against the numpy restatement tests/image_ref.py, bit for bit — RGB / RGBA / one channel, Lanczos3 /
Triangle, ratios 1.5 to 7.3, one axis only, outputs one pixel wide or high, odd and prime sizes; masks smaller, larger and equal to
the view, inverted or not, premultiplied or not; a 4032 x 3024 phone view to the 1920 cap.  Plain commits keep their bytes, a
SceneLoader with max_resolution delivers every view at the restated size, and training through it runs."""
import math

import numpy as np
import pytest
import torch

import image_ref as ref
import util
from brush_amd import synth
from oracle import scene as oscene

pytestmark = pytest.mark.gpu


def _img(h, w, c, seed):
    a = np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)
    # smooth areas and hard edges: overshoot of the negative lobes gets clamped at both ends
    a[: h // 3] = 255
    a[h // 3: h // 2, : w // 2] = 0
    return a


def _gpu_resize(img, nw, nh, filt, dev):
    import brush_amd as ba
    t = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
    out = ba.resize_image(t, (nw, nh), filter=filt)
    torch.cuda.synchronize()
    return out.cpu().numpy()


SIZES = [  # (w, h) -> (nw, nh)
    ((150, 90), (100, 60)),      # 1.5
    ((210, 105), (100, 50)),     # 2.1
    ((400, 240), (100, 60)),     # 4
    ((730, 365), (100, 50)),     # 7.3
    ((200, 120), (200, 37)),     # vertical only
    ((211, 64), (53, 64)),       # horizontal only
    ((300, 50), (1, 50)),        # one pixel wide
    ((97, 300), (97, 1)),        # one pixel high
    ((97, 89), (31, 13)),        # primes
    ((101, 103), (1, 1)),
    ((13, 7), (29, 17)),         # enlarging (sratio = 1)
]


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("filt", [ref.LANCZOS3, ref.TRIANGLE])
def test_resize_u8_is_bit_exact(dev, c, filt):
    for k, ((w, h), (nw, nh)) in enumerate(SIZES):
        img = _img(h, w, c, 1000 * c + k)
        src = img[:, :, 0] if c == 1 else img
        got = _gpu_resize(src, nw, nh, filt, dev)
        want = ref.resize(src, nw, nh, filt)
        assert got.shape == want.shape, (w, h, nw, nh)
        diff = np.argwhere(got != want)
        assert diff.size == 0, (c, filt, w, h, nw, nh, diff[:5], got[tuple(diff[0])], want[tuple(diff[0])])


def test_resize_u8_same_size_is_a_copy_and_rejects_bad_input(dev):
    import brush_amd as ba
    img = _img(33, 47, 4, 5)
    assert np.array_equal(_gpu_resize(img, 47, 33, ref.LANCZOS3, dev), img)
    t = torch.from_numpy(img).to(dev)
    with pytest.raises(ValueError):
        ba.resize_image(t, (10, 10), filter="bicubic")
    with pytest.raises(ValueError):
        ba.resize_image(t.float(), (10, 10))
    with pytest.raises(ba.BrushHipError):
        ba.resize_image(t, (0, 10))


def _ring(up, img, **kw):
    slot = up.submit_view(img, **kw)
    packed, has_alpha = up.acquire(slot)
    got = util.u32(packed)
    up.release(slot)
    return got, has_alpha


CASES = [  # (h, w, c, mask shape or None, invert, max_resolution, scale, premultiply)
    (90, 150, 3, None, False, 100, 1.0, True),
    (105, 211, 4, None, False, 100, 1.0, True),
    (105, 211, 4, None, False, 100, 1.0, False),
    (240, 400, 3, None, False, 1920, 0.25, True),
    (365, 730, 4, None, False, 100, 1.0, True),
    (89, 97, 3, None, False, 0, 0.33, True),
    (60, 80, 3, (60, 80), False, 1920, 1.0, False),    # mask of the same size, no resize
    (60, 80, 4, (60, 80), True, 1920, 1.0, True),
    (60, 80, 3, (23, 37), False, 1920, 1.0, True),     # smaller mask
    (60, 80, 3, (150, 201), True, 1920, 1.0, False),   # larger mask
    (120, 160, 4, (61, 79), False, 100, 1.0, True),    # smaller mask, then the cap
    (120, 160, 3, (240, 320), True, 1920, 0.5, False),  # larger mask, then a LOD scale
    (120, 160, 3, (120, 160), False, 64, 1.0, True),
    (7, 3000, 3, None, False, 1920, 0.1, True),          # the short side clamps to 1
]


@pytest.mark.parametrize("case", CASES, ids=[str(i) for i in range(len(CASES))])
def test_ring_view_is_bit_exact(dev, case):
    import brush_amd as ba
    h, w, c, mshape, invert, mx, scale, premul = case
    img = _img(h, w, c, h * 7 + w + c)
    if c == 4:
        img[0, 0, 3], img[-1, -1, 3] = 0, 255
    mask = None
    if mshape is not None:
        mask = np.random.default_rng(h + w).integers(0, 256, mshape, dtype=np.uint8)
        mask[: mshape[0] // 2, : mshape[1] // 3] = 0
    up = ba.BatchUploader(max(h * w, (h * w * c + (mask.size if mask is not None else 0) + 3) // 4), slots=2)
    got, has_alpha = _ring(up, img, mask=mask, invert_mask=invert, max_resolution=mx, scale=scale, premultiply=premul)
    up.close()
    want, want_alpha = ref.load_view(img, mask, invert, mx, scale, premul)
    assert got.shape == want.shape == tuple(reversed(ref.output_size(w, h, mx, scale))), (got.shape, want.shape)
    assert has_alpha == want_alpha == (c == 4 or mask is not None)
    diff = np.argwhere(got != want)
    assert diff.size == 0, (case, diff[:5], hex(int(got[tuple(diff[0])])), hex(int(want[tuple(diff[0])])))


def test_ring_phone_view_to_the_1920_cap(dev):
    import brush_amd as ba
    h, w = 3024, 4032
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 255 // w), (yy * 255 // h), ((xx ^ yy) & 255)], axis=2).astype(np.uint8)
    img[1000:1100, 2000:2100] = 255
    up = ba.BatchUploader(h * w, slots=2)
    got, has_alpha = _ring(up, img)   # max_resolution 1920, scale 1
    up.close()
    want, _ = ref.load_view(img)
    assert got.shape == (1440, 1920) and not has_alpha
    assert np.array_equal(got, want)


def test_plain_commit_keeps_its_bytes_next_to_views(dev):
    import brush_amd as ba
    up = ba.BatchUploader(200 * 300, slots=3)
    for k, (h, w, c, premul) in enumerate([(200, 300, 3, True), (33, 61, 4, True), (33, 61, 4, False), (1, 3, 3, True)]):
        img = _img(h, w, c, 50 + k)
        slot = up.submit(img, premultiply=premul)
        packed, has_alpha = up.acquire(slot)
        got = util.u32(packed)
        up.release(slot)
        want, wa = oscene.view_to_packed_data(img, transparent_alpha=premul)
        assert np.array_equal(got, want) and has_alpha == wa
        # a view that needs no resampling and no mask packs the same bytes
        got_v, ha_v = _ring(up, img, max_resolution=1920, scale=1.0, premultiply=premul)
        assert np.array_equal(got_v, want) and ha_v == wa
        # ... and a resampled view in between does not disturb the next plain commit
        _ring(up, img, max_resolution=max(1, max(h, w) // 2))
    up.close()


def test_ring_refuses_views_that_do_not_fit(dev):
    import brush_amd as ba
    up = ba.BatchUploader(100, slots=2)
    with pytest.raises(ba.BrushHipError):
        up.submit_view(_img(10, 11, 3, 1))            # 110 pixels > max_pixels
    with pytest.raises(ba.BrushHipError):
        up.submit_view(_img(10, 10, 4, 1), mask=np.zeros((10, 10), np.uint8))   # 500 bytes > 4 * max_pixels
    with pytest.raises(ba.BrushHipError):
        up.submit_view(_img(10, 10, 3, 1), scale=0.0)
    import ctypes as C
    from brush_amd import _ffi
    slot, buf = up.map(300)   # a nonzero reserved word is refused (it may take a meaning later)
    d = _ffi.BhViewLoad(w=10, h=10, channels=3, max_resolution=1920, scale=1.0, premultiply=1, reserved=1)
    assert up.lib.bh_uploader_commit_view(up._h, slot, C.byref(d)) == -1
    got, _ = _ring(up, _img(10, 10, 3, 2), mask=np.zeros((10, 10), np.uint8))   # 400 bytes fit; the ring still works
    assert got.shape == (10, 10) and ((got >> 24) == 0).all()
    up.close()


def _views(dev):
    import brush_amd as ba
    sizes = [(300, 400), (120, 90), (64, 48), (250, 250)]
    cams = []
    for k, (h, w) in enumerate(sizes):
        cp = synth.default_camera_params(w, h)
        cams.append(ba.Camera(position=cp["pos"], rotation=util.quat_from_axis_angle((0, 1, 0), 0.05 * k), fov_x=cp["fov_x"], fov_y=cp["fov_y"]))
    imgs = [_img(h, w, 3 + (k & 1), 300 + k) for k, (h, w) in enumerate(sizes)]
    return imgs, cams


def test_scene_loader_delivers_views_at_the_restated_size(dev):
    import brush_amd as ba
    imgs, cams = _views(dev)
    masks = [None, np.full((45, 60), 200, np.uint8), None, None]
    views = [(imgs[k], cams[k], None, masks[k]) for k in range(4)]
    for mx, scale in ((128, 1.0), (1920, 0.5)):
        ld = ba.SceneLoader(views, seed=4, slots=3, max_resolution=mx, image_scale=scale)
        seen = set()
        for _ in range(4):
            b = ld.next_batch()
            k = b.view_index
            seen.add(k)
            want, wa = ref.load_view(imgs[k], masks[k], False, mx, scale, premultiply=masks[k] is None)
            got = util.u32(b.img_packed)
            assert got.shape == want.shape and np.array_equal(got, want), (k, mx, scale)
            assert b.has_alpha == wa and b.alpha_is_mask == (masks[k] is not None)
        ld.close()
        assert seen == {0, 1, 2, 3}


def test_scene_loader_defaults_keep_the_plain_path(dev):
    import brush_amd as ba
    imgs, cams = _views(dev)
    ld = ba.SceneLoader(list(zip(imgs, cams)), seed=9, slots=2)
    for _ in range(4):
        b = ld.next_batch()
        k = b.view_index
        want, _ = oscene.view_to_packed_data(imgs[k], transparent_alpha=True)
        assert np.array_equal(util.u32(b.img_packed), want)
    ld.close()


def test_training_through_a_downscaling_loader(dev):
    import brush_amd as ba
    n, w, h = 3000, 320, 192
    sc = synth.make_scene(n, 0xD9, sh_degree=0, log_scale_range=(math.log(0.02), math.log(0.2)),
                          tan_half_fov=(math.tan(math.radians(30)), math.tan(math.radians(30)) * h / w))
    cp = synth.default_camera_params(w, h)
    cams = [ba.Camera(position=cp["pos"], rotation=util.quat_from_axis_angle((0, 1, 0), 0.03 * k), fov_x=cp["fov_x"], fov_y=cp["fov_y"]) for k in range(3)]
    views = [(_img(h, w, 3, 700 + k), cams[k]) for k in range(3)]
    ld = ba.SceneLoader(views, seed=2, slots=3, max_resolution=160)
    spl = ba.Splats(sc["transforms"].copy(), sc["sh"].copy(), sc["raw_opac"].copy(), device=dev)
    tr = ba.SplatTrainer(ba.TrainConfig(mean_noise_weight=0.0), median_scene_scale=3.0)
    losses = []
    for _ in range(8):
        b = ld.next_batch()
        assert b.img_size() == (96, 160)
        tr.step(b, spl)
        losses.append(tr.stats().loss)
    ld.close()
    assert all(math.isfinite(v) for v in losses), losses
    assert torch.isfinite(spl.transforms).all()
