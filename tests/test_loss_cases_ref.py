"""The image families of tests/loss_cases.py, and whether float64 autograd (oracle/autograd_loss_ref.py) is a usable yardstick
on each of them: tests/test_gpu_loss_pair_pinned.py holds the HIP kernels to a multiple of the oracle's own float32 error against
that float64 result, which means something only where the float64 gradient is not zero and the oracle's error is small.

The oracle's error, max over the image / max|g64|, the worst over the five shapes, three weight pairs and three modes (printed per
case, run with -s): noise 1.0e-6, black_bg 1.7e-5, inverted 5.2e-5, identical 1.5e-4, converged 1.6e-4, flat_bright 1.8e-4, ramp
2.1e-4.  The bound is 5e-4: about three times the worst figure measured on such images, and far below anything structural (a wrong
tap or a lost halo row is 1e-2 and more).

Pixels where float32 and float64 take different signs of (render - photo) are left out of the comparison (loss_cases.ambiguous):
the photo is k / 255 in float64 and k * (1 / 255) in float32, so an exact tie of the float32 values — nearly all of `identical`,
and about one value in 1e5 of a render within 0.003 of its photo — is a nonzero difference to float64, and the L1 term's gradient
there a convention, not an error.  They are counted: under all of `identical`, at most a thousandth of any other family."""
import numpy as np
import pytest

import loss_cases as lc

BOUND = 5e-4


def test_families_are_what_they_say():
    for name in lc.FAMILIES:
        for h, w in lc.SHAPES:
            img, gt = lc.case(name, h, w)
            again = lc.FAMILIES[name](h, w, 1)
            assert np.array_equal(img, again[0]) and np.array_equal(gt, again[1]), name   # seeded
            assert np.isfinite(img).all()
    h, w = 83, 260
    img, gt = lc.case("black_bg", h, w)
    d, inside = lc.decode_f32(gt), lc.disc(h, w)
    assert inside.any() and not inside.all()
    assert not img[~inside].any() and not gt[~inside].any() and (d[inside][:, 3] == 1.0).all()
    img, gt = lc.identical(h, w, 1, patch=False)
    assert np.array_equal(img, lc.decode_f32(gt))   # bit for bit, alpha included
    d = lc.decode_f32(gt)[..., :3]
    assert (d == 0.0).any() and (d == 1.0).any()    # saturated black and white: ties that float64 sees too
    img, gt = lc.case("identical", h, w)
    differs = (img != lc.decode_f32(gt)).any(-1)
    ys, xs = lc.identical_patch(h, w)
    assert differs[ys, xs].all() and differs.sum() == differs[ys, xs].size
    img, gt = lc.case("inverted", h, w)
    assert np.array_equal(img[..., :3], np.float32(1.0) - lc.decode_f32(gt)[..., :3])
    for name, reg in ((n, lc.regions(*s)) for n, s in (("a", (115, 40)), ("b", (83, 260)))):
        total = reg["border"].astype(int) + reg["seam"] + reg["interior"]
        assert (total == 1).all() and all(r.any() for r in reg.values())


@pytest.mark.parametrize("mode", list(lc.MODES))
@pytest.mark.parametrize("weights", lc.WEIGHTS, ids=lambda t: "l1_%g_ssim_%g" % t)
@pytest.mark.parametrize("h,w", lc.SHAPES)
@pytest.mark.parametrize("family", list(lc.FAMILIES))
def test_float64_reference_is_a_yardstick(family, h, w, weights, mode):
    y = lc.yardsticks(family, h, w, weights, mode)
    n_excl, n = int(y["excluded"].sum()), h * w
    if family == "identical":
        assert n_excl < n, "every pixel is a tie: nothing left to compare"
    else:
        # (a continuous render lands within the 6e-8 between k / 255 and k * (1 / 255) about once in 1e5 values at sigma 0.003)
        assert n_excl <= n // 1000, "%d pixels where float32 and float64 take different signs of (render - photo)" % n_excl
    gmax = float(np.abs(y["grad64"]).max())
    map_err = float(np.abs(y["map32"].astype(np.float64) - y["map64"]).max())
    err = lc.grad_err(y["grad32"], y)
    print("%s %dx%d %s %s: map err %.3g  grad err / max|g| %.3g  (max|g| %.3g, %d of %d pixels excluded)" % (family, h, w, weights, mode, map_err,
                                                                                                           err / gmax if gmax else np.inf, gmax, n_excl, n))
    assert np.isfinite(y["grad64"]).all() and np.isfinite(y["grad32"]).all()
    assert gmax > 0.0
    assert err <= BOUND * gmax, (err / gmax, BOUND)
