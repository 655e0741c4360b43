"""The numpy restatement of mask lifting (tests/lift_ref.py; include/brush_hip_lift.h) without a GPU: the properties
the GPU suite relies on when it holds the kernels to it, on the weights of the float64 renderer (tests/feature_ref.py::render's
`vis`) rounded to f32, and the two-object scene lifted end to end by the restatement alone."""
import numpy as np
import pytest

import lift_ref as lr


def _weights(model="pinhole", mip=False, smooth=False):
    _, _, w, h, out = lr.reference(model, mip, smooth)
    return out["vis"].numpy().astype(np.float32), out, w, h


def _xy_labels(w, h, L):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx + 3 * yy) % L).astype(np.uint8)


def test_votes_partition_the_unlabelled_votes():
    w32, out, w, h = _weights()
    one, wmax, count = lr.votes_from_weights(w32, None, 1)
    assert one.shape == (300, 1) and int((one > 0).sum()) > 100
    for L in (2, 5, 17, 256):
        votes, m, c = lr.votes_from_weights(w32, _xy_labels(w, h, L), L)
        assert np.array_equal(votes.sum(axis=1), one[:, 0]), L
        assert np.array_equal(m, wmax) and np.array_equal(c, count)
    assert np.array_equal(count, out["vis"].numpy().astype(bool).reshape(300, -1).sum(axis=1))
    assert int(count.sum()) == int(out["n_terms"].sum())


def test_an_ignored_pixel_removes_exactly_its_terms():
    w32, _, w, h = _weights()
    L = 5
    lab = _xy_labels(w, h, L)
    votes, wmax, count = lr.votes_from_weights(w32, lab, L)
    holes = lab.copy()
    holes[10, 20], holes[30, 41], holes[7, 7] = 255, L, 200   # 255, the first value that is no label, something between
    got, m, c = lr.votes_from_weights(w32, holes, L)
    want = votes.copy()
    for y, x in ((10, 20), (30, 41), (7, 7)):
        want[:, lab[y, x]] -= lr.quantise(w32[:, y, x])
    assert np.array_equal(got, want) and not np.array_equal(got, votes)
    # the two statistics describe the render, not the labelling
    assert np.array_equal(m, wmax) and np.array_equal(c, count)


@pytest.mark.parametrize("smooth", [False, True], ids=["hard", "smooth"])
def test_votes_add_up_to_the_alpha_channel(smooth):
    """All votes of a frame are its alpha channel: votes.sum() / 2^24 = the sum over pixels of alpha to within n_terms 2^-25 per
    pixel.  Pixel by pixel a term can be off by more than that half unit of the vote grid, because the float64 weight is rounded
    twice: to f32 (at most 2^-25 in [1/2, 1), where f32 values lie ON the grid and the second rounding is exact; at most 2^-26
    below 1/2) and then to the grid (at most 2^-25): 1.5 * 2^-25 per term at worst, which is the per-pixel bound."""
    w32, out, w, h = _weights(smooth=smooth)
    alpha, n_terms = out["alpha"].numpy(), out["n_terms"].numpy()
    votes, _, _ = lr.votes_from_weights(w32, None, 1)
    assert abs(votes.sum() / lr.VOTE_ONE - alpha.sum()) <= float(n_terms.sum()) * 2.0 ** -25
    per_pixel = lr.quantise(w32).sum(axis=0).astype(np.float64) / lr.VOTE_ONE
    err = np.abs(per_pixel - alpha)
    bound = n_terms * 1.5 * 2.0 ** -25
    assert (err <= bound + 1e-15).all(), float((err - bound).max())


def test_assign():
    votes = np.array([[5, 5, 1], [0, 0, 0], [1, 7, 7], [lr.VOTE_ONE, 0, 0], [0, 3, lr.VOTE_ONE - 4], [2, 1, 0]], np.int64)
    lab, share = lr.assign(votes)
    assert lab.tolist() == [0, 255, 1, 0, 2, 0], "ties go to the lowest label, a row of zeros is unassigned"
    assert share.dtype == np.float32 and share[1] == 0.0 and share[0] == np.float32(5.0 / 11.0) and share[3] == 1.0
    # min_weight on the row's total, in raw units: rint(min_weight * 2^24)
    lab, share = lr.assign(votes, min_weight=1.0)
    assert lab.tolist() == [255, 255, 255, 0, 255, 255] and share.tolist() == [0, 0, 0, 1, 0, 0]
    lab, _ = lr.assign(votes, min_weight=float(np.float32(1.0 - 2.0 ** -24)))
    assert lab.tolist() == [255, 255, 255, 0, 2, 255]
    assert lr.min_total(0.0) == 0 and lr.min_total(-1.0) == 0 and lr.min_total(0.5) == 1 << 23 and lr.min_total(2.0 ** -25) == 0 and lr.min_total(3 * 2.0 ** -25) == 2


def test_select():
    votes = np.array([[6, 2], [2, 6], [4, 4], [0, 0], [0, 9]], np.int64)
    wmax = np.array([0.9, 0.2, 0.5, 0.0, 0.7], np.float32)
    count = np.array([10, 3, 5, 0, 1])
    sel = lambda **kw: lr.select(votes, wmax, count, **kw).tolist()
    assert sel(label=0) == [1, 0, 1, 0, 0]                      # >= min_share: the tie at one half passes
    assert sel(label=1, min_share=0.75) == [0, 1, 0, 0, 1]
    assert sel(label=1, min_share=0.0) == [1, 1, 1, 0, 1]       # a splat without a vote is never selected by a label
    assert sel() == [1, 1, 1, 0, 1]                             # any label: it got a vote
    assert sel(min_weight=9 / lr.VOTE_ONE) == [0, 0, 0, 0, 1]
    assert sel(min_max_weight=0.5) == [1, 0, 1, 0, 1]
    assert sel(min_pixels=4) == [1, 0, 1, 0, 0]
    assert sel(label=0, min_max_weight=0.6, min_pixels=4) == [1, 0, 0, 0, 0]   # ANDed
    assert sel(label=0, invert=True) == [0, 1, 0, 1, 1]
    # the statistics alone
    assert lr.select(None, wmax, count, min_pixels=4, n=5).tolist() == [1, 0, 1, 0, 0]
    assert lr.select(None, None, None, n=3).tolist() == [1, 1, 1] and lr.select(None, None, None, invert=True, n=3).tolist() == [0, 0, 0]
    # a test whose table is missing is refused, not skipped
    for kw in (dict(votes=None, label=0), dict(votes=None, min_weight=0.5), dict(votes=votes, max_weight=None, min_max_weight=0.5),
               dict(votes=votes, pixel_count=None, min_pixels=1)):
        args = dict(votes=votes, max_weight=wmax, pixel_count=count, n=5)
        args.update(kw)
        with pytest.raises(ValueError):
            lr.select(**args)


def test_two_objects_are_lifted_end_to_end():
    """Two separated clusters, label maps from each cluster's own alpha, three views: every splat that gathered a summed weight of at
    least 1 gets its cluster's label."""
    sc, cams, w, h, member = lr.two_cluster_case()
    n = member.size
    total = np.zeros((n, 2), np.int64)
    for cp in cams:
        alphas = [lr.render_f64(lr.subset(sc, member == k), cp, w, h)["alpha"].numpy() for k in (0, 1)]
        lab = lr.cluster_labels(*alphas)
        assert (lab == 0).sum() > 40 and (lab == 1).sum() > 40 and (lab == 255).sum() > 1000
        vis = lr.render_f64(sc, cp, w, h)["vis"].numpy().astype(np.float32)
        votes, _, _ = lr.votes_from_weights(vis, lab, 2)
        total += votes
    got, share = lr.assign(total, min_weight=1.0)
    strong = total.sum(axis=1) >= lr.VOTE_ONE
    assert int(strong[member == 0].sum()) >= 10 and int(strong[member == 1].sum()) >= 10
    assert np.array_equal(got[strong], member[strong].astype(np.uint8))
    assert (got[~strong] == 255).all() and (share[strong] > 0.99).all()
    keep = lr.select(total, label=1, min_weight=1.0)
    assert np.array_equal(keep.astype(bool), strong & (member == 1))
