"""LOD decimation on the MI355X (brush-train/src/lod.rs; include/brush_hip.h "LOD decimation"):
  * bh_pup_accumulate bit for bit against the numpy f32 restatement (tests/test_lod_abi.py), dense and row-list mode;
  * bh_pup_scores against the numpy log_det_6x6: same -inf / NaN pattern, finite scores within the final logs' rounding;
  * bh_decimate_to_count bit for bit against Python's stable sort with the reference's comparator;
  * compute_pup_scores end to end against the CPU oracle's forward / loss / backward / fold and the numpy accumulate, and the
    fused per-view call against the composed operators;
  * the scores carry meaning: keeping the top half preserves a held-out view far better than keeping the bottom half;
  * a full-size run (1 M splats, 1080p)."""
import math
import time

import numpy as np
import pytest
import torch

import util
from test_lod_abi import PLANE, accumulate_f32, log_det_6x6_f32, reference_order

pytestmark = pytest.mark.gpu

# Hessian tolerances, from the gradient tolerances of tests/test_gpu_backward.py (GRAD_TOL = 1e-4 of a tensor's largest gradient)
# carried through the product j_i j_k: a product of two components each within 1e-4 of their scale is within ~2e-4 of the
# product's scale, and the sum over views keeps the bound relative to sqrt(H_ii H_kk) (Cauchy-Schwarz).  With a margin of 2.5 for the
# per-view scales differing from the summed ones: per element 5e-4 sqrt(H_ii H_kk), per plane 1e-3 of the plane's largest entry,
# which is also the per-element floor.
H_ELEM = 5e-4
H_PLANE = 1e-3
# Scores: log det H = log det C + sum ln H_ii with C = D^-1/2 H D^-1/2 (unit diagonal), and the per-element bound makes every entry
# of C's perturbation E at most H_ELEM, so log det moves by |tr(C^-1 E)| <= 6 H_ELEM / lambda_min(C) to first order (the sum of the
# ln H_ii moves by 6 x H_ELEM at most).  Per row: SCORE_TOL + 12 H_ELEM / lambda_min(C), on the rows whose bound means something
# (lambda_min(C) >= LAMBDA_MIN: <= 1.25).  A sum of 10 rank-1 terms in 6 dimensions is rarely better conditioned than that: on this
# test's scene and views the oracle finds 11.5 % (8.9 % with min_scale) of the visible splats qualifying, against 0 % under the
# unscaled criterion (smallest pivot^2 >= 0.05 x the largest diagonal entry).  At least MIN_QUALIFYING of them must, so the check
# cannot pass on an empty set.
SCORE_TOL = 0.05
LAMBDA_MIN = 0.005
MIN_QUALIFYING = 0.05


def _ctx():
    import brush_amd as ba
    return ba.get_context()


def _nan_equal_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def _nasty_rows(rng, n):
    """random J rows with +-0, denormals, 1e+-18 magnitudes and NaN mixed in"""
    v = rng.normal(size=(n, 10)).astype(np.float32)
    kind = rng.integers(0, 10, size=(n, 10))
    v[kind == 0] = 0.0
    v[kind == 1] = -0.0
    v[kind == 2] = (rng.uniform(1, 8, size=(kind == 2).sum()) * 1e-40).astype(np.float32)   # denormal
    v[kind == 3] = (rng.normal(size=(kind == 3).sum()) * 1e18).astype(np.float32)
    v[kind == 4] = (rng.normal(size=(kind == 4).sum()) * 1e-18).astype(np.float32)
    v[rng.integers(0, n, size=max(1, n // 500)), rng.integers(0, 10, size=max(1, n // 500))] = np.nan
    v[rng.integers(0, n, size=n // 10)] = 0.0      # whole zero rows (skipped)
    neg = rng.integers(0, n, size=n // 10)
    v[neg] = -0.0                                   # whole -0 rows
    return v


def test_pup_accumulate_is_bit_identical_to_the_f32_restatement():
    from brush_amd import host
    ctx = _ctx()
    rng = np.random.default_rng(0x21)
    n = 70_001
    want = np.zeros((21, n), np.float32)
    got = torch.zeros((21, n), dtype=torch.float32, device="cuda")
    for _ in range(5):
        vt = _nasty_rows(rng, n)
        accumulate_f32(want, vt)
        host.pup_accumulate(torch.from_numpy(vt).cuda(), got, ctx=ctx)
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    assert _nan_equal_bits(g, want)
    assert not np.signbit(g[g == 0]).any()   # never -0

    # row-list mode == dense mode when the unlisted rows are zero (the fused path's situation)
    dense = torch.zeros((21, n), dtype=torch.float32, device="cuda")
    listed = torch.zeros((21, n), dtype=torch.float32, device="cuda")
    for _ in range(5):
        vt = _nasty_rows(rng, n)
        rows = rng.permutation(n)[: n // 3].astype(np.int32)
        mask = np.zeros(n, bool)
        mask[rows] = True
        vt[~mask] = 0.0
        vt_d = torch.from_numpy(vt).cuda()
        host.pup_accumulate(vt_d, dense, ctx=ctx)
        host.pup_accumulate(vt_d, listed, rows=torch.from_numpy(rows).cuda(), ctx=ctx)
    torch.cuda.synchronize()
    assert _nan_equal_bits(dense.cpu().numpy(), listed.cpu().numpy())


def test_pup_scores_match_the_numpy_log_det():
    from brush_amd import host
    rng = np.random.default_rng(0x1D)
    groups = []
    groups.append(np.zeros((21, 200), np.float32))                       # zero rows
    for rank in range(1, 6):                                              # rank 1..5
        h = np.zeros((21, 300), np.float32)
        for _ in range(rank):
            accumulate_f32(h, rng.normal(size=(300, 10)).astype(np.float32))
        groups.append(h)
    ind = np.zeros((21, 300), np.float32)                                 # indefinite
    for (i, k), e in PLANE.items():
        ind[e] = rng.normal(size=300) if i != k else rng.normal(size=300) * 2.0
    groups.append(ind)
    nanrows = np.zeros((21, 100), np.float32)                             # NaN somewhere
    for _ in range(8):
        accumulate_f32(nanrows, rng.normal(size=(100, 10)).astype(np.float32))
    nanrows[rng.integers(0, 21, size=100), np.arange(100)] = np.nan
    groups.append(nanrows)
    spd = np.zeros((21, 5000), np.float32)                                # random SPD, row scales over many decades
    row_scale = np.exp(rng.uniform(-8, 8, size=(5000, 1))).astype(np.float32)
    for _ in range(12):
        accumulate_f32(spd, rng.normal(size=(5000, 10)).astype(np.float32) * row_scale)
    groups.append(spd)
    h = np.ascontiguousarray(np.concatenate(groups, axis=1))
    want = log_det_6x6_f32(h)
    got = host.pup_scores(torch.from_numpy(h).cuda(), ctx=_ctx()).cpu().numpy()
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    assert np.isfinite(got[fin]).all()
    assert fin.sum() > 4000 and np.isneginf(want).sum() > 200 and np.isnan(want).sum() > 50
    err = np.abs(got[fin].astype(np.float64) - want[fin]) / np.maximum(1.0, np.abs(want[fin].astype(np.float64)))
    assert err.max() <= 1e-5, err.max()


def _tie_scores(rng, n):
    s = rng.integers(-6, 6, size=n).astype(np.float32) * np.float32(0.5)
    kind = rng.integers(0, 12, size=n)
    s[kind == 0] = 0.0
    s[kind == 1] = -0.0
    s[kind == 2] = -np.inf
    s[kind == 3] = np.inf
    s[kind == 4] = np.nan
    s[kind == 5] = rng.normal(size=(kind == 5).sum()).astype(np.float32)
    run = rng.integers(0, max(1, n - 64))
    s[run: run + 64] = -np.inf                     # a run of -inf
    return s


@pytest.mark.parametrize("n", [1, 5, 4097, 1_000_003])
def test_decimate_to_count_is_the_reference_stable_sort(n):
    import brush_amd as ba
    ctx = _ctx()
    rng = np.random.default_rng(n)
    scores = _tie_scores(rng, n)
    order = np.asarray(reference_order(scores), np.int64)
    s_dev = torch.from_numpy(scores).cuda()
    for deg in (0, 3):
        c = (deg + 1) ** 2
        tr = torch.from_numpy(rng.normal(size=(n, 10)).astype(np.float32)).cuda()
        sh = torch.from_numpy(rng.normal(size=(n, c, 3)).astype(np.float32)).cuda()
        op = torch.from_numpy(rng.normal(size=n).astype(np.float32)).cuda()
        ms = torch.from_numpy(rng.uniform(0, 1e-2, size=n).astype(np.float32)).cuda()
        for with_ms in (False, True):
            splats = ba.Splats(tr, sh, op, device="cuda", min_scale=ms if with_ms else None)
            for target in sorted(t for t in {1, n // 2, n - 1, n, n + 7} if t >= 1):
                out, keep = ba.decimate_to_count(splats, s_dev, target, ctx=ctx, return_indices=True)
                k = min(target, n)
                want = torch.from_numpy(order[:k] if target < n else np.arange(n)).cuda()
                assert out.num_splats() == k
                assert torch.equal(keep.long(), want), (n, target)
                assert torch.equal(out.transforms, tr[want]) and torch.equal(out.sh_coeffs, sh[want]) and torch.equal(out.raw_opacities, op[want])
                if with_ms:
                    assert torch.equal(out.min_scale, ms[want])
                else:
                    assert out.min_scale is None
                if target >= n:
                    assert out is splats   # lod.rs:15-17: returned unchanged


# ---- end to end against the oracle --------------------------------------------------------------------------------------------
def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return (aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
            aw * bw - ax * bx - ay * by - az * bz)


def _turned_cameras(k, yaw0, spread, cp, model="pinhole", dist=(), move=0.02, pitch=0.03):
    """k cameras near the origin, turned by small yaw / pitch angles: every splat of synth's frustum scene is in front of all of
    them.  (A splat's H has full rank only if it received a gradient in >= 6 views with independent J, so the views see the same
    splats; `move` spreads the camera centres, which decorrelates the views' J.)"""
    cams = []
    for v in range(k):
        yaw = yaw0 + spread * (v / max(k - 1, 1) - 0.5)
        q = _qmul(util.quat_from_axis_angle((0, 1, 0), yaw), util.quat_from_axis_angle((1, 0, 0), pitch * math.sin(2.7 * v)))
        pos = (move * math.sin(1.3 * v), move * math.cos(1.9 * v) if move > 0.05 else 0.0, move * math.sin(0.7 * v) if move > 0.05 else 0.0)
        cams.append(dict(pos=pos, rot_xyzw=q, fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=(0.5, 0.5), model=model, dist=dist))
    return cams


def _frustum_scene(n, seed, w, h, sh_degree=1):
    from brush_amd import synth
    cp = synth.default_camera_params(w, h)
    return synth.make_scene(n, seed, sh_degree=sh_degree, log_scale_range=(math.log(0.02), math.log(0.2)),
                            tan_half_fov=(math.tan(cp["fov_x"] / 2), math.tan(cp["fov_y"] / 2))), cp


def _packed_like_loader(img, mask):
    """view_to_packed_data (brush-dataset/src/scene.rs:97-136) on the host: RGB -> a = 255; RGBA premultiplied in byte space
    ((c a + 127) / 255) unless the alpha is a mask"""
    img = np.asarray(img, np.uint8)
    if img.shape[2] == 3:
        img = np.concatenate([img, np.full(img.shape[:2] + (1,), 255, np.uint8)], axis=2)
    elif not mask:
        a = img[..., 3:4].astype(np.uint32)
        rgb = (img[..., :3].astype(np.uint32) * a + 127) // 255
        img = np.concatenate([rgb.astype(np.uint8), img[..., 3:4]], axis=2)
    return util.packed_from_rgba(img)


def _views(w, h, seed, cp):
    rng = np.random.default_rng(seed)
    cams = _turned_cameras(9, 0.0, 0.3, cp, move=0.5, pitch=0.15) + _turned_cameras(1, 0.05, 0.0, cp, model="kb4", dist=util.REF_LENSES["kb4"][1])
    views = []
    for v, cp in enumerate(cams):
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([128 + 100 * np.sin(xx * 0.05 + v), 128 + 100 * np.cos(yy * 0.07 - v), 128 + 60 * np.sin((xx + yy) * 0.03)], -1)
        img = np.clip(base + rng.normal(0, 10, size=base.shape), 0, 255).astype(np.uint8)
        mask = False
        if v == 3:   # one RGBA view (premultiplied by the loader)
            img = np.concatenate([img, rng.integers(0, 256, size=(h, w, 1)).astype(np.uint8)], axis=2)
        views.append((img, cp, mask))
    return views


def _oracle_hessian(scene, views, w, h, min_scale=None):
    from oracle import bo
    n = scene["transforms"].shape[0]
    hess = np.zeros((21, n), np.float32)
    t, o = scene["transforms"], scene["raw_opac"]
    rt, ro = (t, o) if min_scale is None else bo.fold_min_scale(t, o, min_scale)
    for img, cp, mask in views:
        gt = _packed_like_loader(img, mask)
        ref = bo.Render().forward(util.oracle_camera(bo, cp, w, h), rt, scene["sh"], ro, bg=(0.0, 0.0, 0.0), flags=bo.FLAG_BWD_INFO)
        pred = ref.image()[..., :3].transpose(2, 0, 1)
        dl = np.full((3, h, w), 1.0 / (3 * h * w), np.float32)
        dpred = bo.image_loss_backward(pred, gt, dl, 1.0, 0.0)
        v_out = np.zeros((h, w, 4), np.float32)
        v_out[..., :3] = dpred.transpose(1, 2, 0)
        ref.backward(v_out)
        vt = ref.get("v_transforms").reshape(n, 10)
        if min_scale is not None:
            vt, _ = bo.fold_min_scale_backward(t, o, min_scale, vt, ref.get("v_raw_opac").reshape(n))
        accumulate_f32(hess, vt)
    return hess


def _lambda_min_scaled(hess):
    """smallest eigenvalue of every row's H scaled to unit diagonal (D^-1/2 H D^-1/2; 0 where a diagonal entry is 0).  The scaling
    makes the measure blind to the units of J's components (a mean gradient and a log-scale gradient differ by orders of magnitude)
    and changes log det only by sum ln H_ii."""
    from test_lod_abi import planes_to64
    m = planes_to64(hess)
    d = np.diagonal(m, axis1=1, axis2=2)
    ok = (d > 0).all(axis=1)
    out = np.zeros(m.shape[0])
    s = 1.0 / np.sqrt(d[ok])
    c = m[ok] * s[:, :, None] * s[:, None, :]
    out[ok] = np.linalg.eigvalsh(c)[:, 0]
    return out


def _check_hessian(got, want, what):
    got = got.astype(np.float64)
    want = want.astype(np.float64)
    diag = [want[PLANE[(i, i)]] for i in range(6)]
    for (i, k), e in PLANE.items():
        d = np.abs(got[e] - want[e])
        floor = H_PLANE * np.abs(want[e]).max()
        assert d.max() <= max(floor, 1e-30), (what, (i, k), d.max(), floor)
        tol = H_ELEM * np.sqrt(np.maximum(diag[i] * diag[k], 0.0)) + floor
        assert (d <= tol).all(), (what, (i, k), float((d / np.maximum(tol, 1e-30)).max()))


@pytest.mark.parametrize("with_min_scale", [False, True])
def test_compute_pup_scores_against_the_oracle(with_min_scale):
    import brush_amd as ba
    w, h = 192, 128
    scene, cp = _frustum_scene(4000, 0x5C, w, h)
    views = _views(w, h, 0xA1, cp)
    ms = np.random.default_rng(3).uniform(0.0, 0.03, size=4000).astype(np.float32) if with_min_scale else None
    splats = ba.Splats(scene["transforms"], scene["sh"], scene["raw_opac"], device="cuda", min_scale=ms)
    hip_views = [(img, util.hip_camera(ba, cp), mask) for img, cp, mask in views]
    scores, hess = ba.compute_pup_scores(splats, hip_views, return_hessian=True)
    got_h, got_s = hess.cpu().numpy(), scores.cpu().numpy()
    want_h = _oracle_hessian(scene, views, w, h, ms)
    _check_hessian(got_h, want_h, "hessian")
    zero = (want_h == 0).all(axis=0)
    assert np.isneginf(got_s[zero]).all()
    visible = ~zero
    assert visible.sum() > 1000
    lam = _lambda_min_scaled(want_h)
    well = visible & (lam >= LAMBDA_MIN)
    assert well.sum() >= MIN_QUALIFYING * visible.sum(), (well.sum(), visible.sum())
    want_s = log_det_6x6_f32(want_h)
    assert np.isfinite(got_s[well]).all() and np.isfinite(want_s[well]).all()
    err = np.abs(got_s[well].astype(np.float64) - want_s[well])
    tol = SCORE_TOL + 12.0 * H_ELEM / lam[well]
    assert (err <= tol).all(), float((err / tol).max())


def test_fused_view_matches_the_composed_operators():
    import brush_amd as ba
    from brush_amd import host
    ctx = _ctx()
    w, h = 192, 128
    scene, cp = _frustum_scene(4000, 0x77, w, h, sh_degree=2)
    views = _views(w, h, 0xB2, cp)
    splats = ba.Splats(scene["transforms"], scene["sh"], scene["raw_opac"], device="cuda")
    fused = torch.zeros((21, 4000), dtype=torch.float32, device="cuda")
    composed = torch.zeros_like(fused)
    for img, cp, mask in views:
        cam = util.hip_camera(ba, cp)
        gt = torch.from_numpy(_packed_like_loader(img, mask).view(np.int32)).cuda()
        host.pup_accumulate_view(splats, cam, gt, fused, ctx=ctx)
        node = ba.render_splats_diff(splats, cam, (w, h), (0.0, 0.0, 0.0), ctx=ctx)
        _, v_out = ba.image_loss_value_and_grad(node.img, gt, l1_weight=1.0, ssim_weight=0.0, ctx=ctx)
        g = node.backward(v_out)
        host.pup_accumulate(g["v_transforms"], composed, ctx=ctx)
    torch.cuda.synchronize()
    _check_hessian(fused.cpu().numpy(), composed.cpu().numpy(), "fused vs composed")


# ---- the scores carry meaning ----------------------------------------------------------------------------------------------------
def _psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 10.0 * math.log10(1.0 / max(mse, 1e-12))


def _render_rgb(ba, splats, cp, w, h, ctx):
    img, _ = ba.render_splats(splats, util.hip_camera(ba, cp), (w, h), (0.0, 0.0, 0.0), pass_=ba.RasterPass.Backward, ctx=ctx)
    return img[..., :3].clamp(0, 1).cpu().numpy()


def test_pup_scores_keep_what_matters():
    """The views look into synth's frustum scene from slightly turned cameras, as scripts/lod_probe.py does: an orbit around an
    opaque ball leaves most splats with a rank-deficient H (-inf), and the two halves then differ by index order only."""
    import brush_amd as ba
    ctx = _ctx()
    w, h = 1920, 1080
    scene, cp = _frustum_scene(64_000, 0x64, w, h)
    teacher = ba.Splats(scene["transforms"], scene["sh"], scene["raw_opac"], device="cuda")
    train = _turned_cameras(12, 0.0, 0.3, cp)
    held = _turned_cameras(4, 0.3 / 22, 0.3 * 0.75, cp)   # between the training views
    views = []
    for cp in train:
        rgb = _render_rgb(ba, teacher, cp, w, h, ctx)
        views.append(((rgb * 255.0 + 0.5).astype(np.uint8), util.hip_camera(ba, cp)))
    scores = ba.compute_pup_scores(teacher, views, ctx=ctx)
    n = teacher.num_splats()
    k = ba.lod_target_count(n, 50)
    top = ba.decimate_to_count(teacher, scores, k, ctx=ctx)
    bottom = ba.decimate_to_count(teacher, -scores.nan_to_num(nan=-np.inf), k, ctx=ctx)   # (a -inf score becomes +inf: kept first)
    perm = torch.from_numpy(np.random.default_rng(1).permutation(n)[:k]).cuda()
    rand = ba.Splats(teacher.transforms[perm], teacher.sh_coeffs[perm], teacher.raw_opacities[perm], device="cuda")
    p = {"top": [], "bottom": [], "random": []}
    for cp in held:
        gt = (_render_rgb(ba, teacher, cp, w, h, ctx) * 255.0 + 0.5).astype(np.uint8).astype(np.float32) / 255.0
        for name, s in (("top", top), ("bottom", bottom), ("random", rand)):
            p[name].append(_psnr(_render_rgb(ba, s, cp, w, h, ctx), gt))
    mean = {kk: float(np.mean(v)) for kk, v in p.items()}
    print("held-out PSNR at keep 50 %%: top %.2f dB, bottom %.2f dB, random %.2f dB" % (mean["top"], mean["bottom"], mean["random"]))
    assert mean["top"] >= mean["bottom"] + 3.0, mean


# ---- full size -------------------------------------------------------------------------------------------------------------------
def test_full_size_scores_and_decimation():
    import brush_amd as ba
    from brush_amd import synth
    ctx = _ctx()
    sc, w, h = synth.config_scene("1m_1080p", sh_degree=3)
    splats = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device="cuda")
    cp = synth.default_camera_params(w, h)
    rng = np.random.default_rng(4)
    views = []
    for v in range(4):
        c = dict(cp)
        c["rot_xyzw"] = util.quat_from_axis_angle((0, 1, 0), 0.04 * (v - 1.5))
        views.append((rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8), util.hip_camera(ba, c)))
    t0 = time.time()
    scores, hess = ba.compute_pup_scores(splats, views, ctx=ctx, return_hessian=True)
    n = splats.num_splats()
    k = ba.lod_target_count(n, 50)
    out, keep = ba.decimate_to_count(splats, scores, k, ctx=ctx, return_indices=True)
    torch.cuda.synchronize()
    elapsed = time.time() - t0
    assert not torch.isnan(hess).any()
    assert out.num_splats() == k == 500_000
    want = np.asarray(reference_order(scores.cpu().numpy())[:k], np.int64)
    assert np.array_equal(keep.cpu().numpy().astype(np.int64), want)
    print("1 M / 1080p, 4 views: scores + decimation %.2f s (first call, allocations included)" % elapsed)
    assert elapsed < 60.0
