"""bh_knn_log_scales / to_init_splats / load_init_splats on the MI355X against tests/knn_ref.py (compute_knn_scales,
brush-train/src/splat_init.rs:179-216): nearest-neighbour distances bit-exact against an f32 brute force, log-scales within 2 ulp
of ln in float64, the search's work bounded, the edge cases of the contract, the PLY path of the training stream
(train_stream.rs:100-123) and the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest
import torch

import knn_ref
from test_knn_init_abi import build_knn_cpp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ba():
    import __graft_entry__ as g
    g.build()
    import brush_amd
    torch.cuda.set_device(0)
    return brush_amd


def _run(ba, pos):
    """-> (log_scales [N] f32, nn [N,2] f32, pairs_tested, transforms after) for means pos [N,3] (other columns seeded)."""
    n = pos.shape[0]
    rng = np.random.default_rng(n)
    tr = rng.normal(size=(n, 10)).astype(np.float32)
    tr[:, :3] = pos
    sp = ba.Splats(tr, np.zeros((n, 1, 3), np.float32), np.zeros(n, np.float32), device="cuda:0")
    ls, nn, st = ba.knn_log_scales(sp, return_distances=True, return_stats=True)
    out = sp.transforms.cpu().numpy()
    assert np.array_equal(ls.cpu().numpy(), out[:, 7:10])
    assert np.array_equal(out[:, 7], out[:, 8]) and np.array_equal(out[:, 7], out[:, 9])
    other = [0, 1, 2, 3, 4, 5, 6]
    assert out[:, other].tobytes() == tr[:, other].tobytes(), "columns other than 7..9 changed"
    return out[:, 7].copy(), nn.cpu().numpy(), st["pairs_tested"], out


def _check_exact(pos, ls, nn, queries=None):
    """nn_dist bit-exact against the f32 brute force and log-scales within 2 ulp of ln in float64, at the rows `queries` (all)."""
    q = np.arange(pos.shape[0]) if queries is None else np.asarray(queries)
    want_nn = knn_ref.nn2_brute(pos, q)
    got_nn = nn[q]
    bad = np.nonzero((got_nn.view(np.uint32) != want_nn.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, "nn_dist differs at %d rows, first %s: got %s want %s" % (bad.size, q[bad[:4]], got_nn[bad[:4]], want_nn[bad[:4]])
    if pos.shape[0] < 3:
        want_ls = np.zeros(q.size, np.float32)
    else:
        upper = np.float32(knn_ref.median_size(pos) * np.float32(0.1))
        want_ls = np.log(knn_ref.clamped_dist(want_nn, upper).astype(np.float64)).astype(np.float32)
    u = knn_ref.ulp_diff(ls[q], want_ls)
    assert u.max(initial=0) <= 2, "log-scale %d ulp from ln (row %d: %r vs %r)" % (u.max(), q[u.argmax()], ls[q][u.argmax()], want_ls[u.argmax()])


@pytest.mark.parametrize("kind", knn_ref.KINDS)
def test_exact_against_the_brute_force(ba, kind):
    pos = knn_ref.cloud(kind, 20000, seed=1)
    ls, nn, pairs, _ = _run(ba, pos)
    _check_exact(pos, ls, nn)
    fin = knn_ref.finite_rows(pos)
    upper = np.float32(knn_ref.median_size(pos) * np.float32(0.1))
    assert np.all(np.isinf(nn[~fin]))
    assert np.all(ls[~fin] == ls.max()) if (~fin).any() else True
    if kind == "tiny":
        assert knn_ref.median_size(pos) == np.float32(0.01)
        assert knn_ref.ulp_diff(ls, np.full_like(ls, np.float32(np.log(np.float64(np.float32(1e-3)))))).max() <= 2
    if kind == "tripled":
        assert (nn[:, 0] == 0.0).sum() >= 19999   # all but the one unrepeated filler point
    assert pairs < 20000 * 20000
    assert upper > 0


def _candidates(pos_dev, q_idx, k=8, chunk=32):
    """the k smallest f32 (dx*dx + dy*dy) + dz*dz per query (itself excluded), elementwise in torch on the GPU -> ids [Q, k]"""
    out = []
    px, py, pz = pos_dev[:, 0], pos_dev[:, 1], pos_dev[:, 2]
    for a in range(0, len(q_idx), chunk):
        qi = torch.as_tensor(q_idx[a:a + chunk], device=pos_dev.device, dtype=torch.int64)
        q = pos_dev[qi]
        dx = q[:, 0:1] - px[None, :]
        dy = q[:, 1:2] - py[None, :]
        dz = q[:, 2:3] - pz[None, :]
        s = (dx * dx + dy * dy) + dz * dz
        s[torch.arange(qi.numel(), device=s.device), qi] = float("inf")
        out.append(torch.topk(s, k, dim=1, largest=False).indices.cpu().numpy())
        del dx, dy, dz, s
    return np.concatenate(out)


@pytest.mark.parametrize("kind", ["uniform", "surface", "outliers"])
def test_exact_at_scale(ba, kind):
    n = 2_000_000
    pos = knn_ref.cloud(kind, n, seed=2)
    ls, nn, pairs, _ = _run(ba, pos)
    rng = np.random.default_rng(3)
    q = np.sort(rng.choice(n, 4096, replace=False))
    cand = _candidates(torch.from_numpy(pos).cuda(), q)
    s = knn_ref.sq_dist_f32(pos[q][:, None, :], pos[cand])   # host recompute in the reference's order
    two = np.sort(s, axis=1)[:, :2]
    want = np.sqrt(two).astype(np.float32)
    bad = np.nonzero(nn[q].view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, "nn_dist differs at %d of 4096 sampled rows: %s vs %s" % (bad.size, nn[q][bad[:4]], want[bad[:4]])
    upper = np.float32(knn_ref.median_size(pos) * np.float32(0.1))
    want_ls = np.log(knn_ref.clamped_dist(want, upper).astype(np.float64)).astype(np.float32)
    assert knn_ref.ulp_diff(ls[q], want_ls).max() <= 2
    assert pairs / n <= 4096


@pytest.mark.parametrize("kind", ["uniform", "surface", "outliers"])
def test_work_is_bounded(ba, kind):
    """A brute force is 10^6 distance evaluations per point at 1 M points; a quadratic fallback or a broken prune shows here."""
    n = 1_000_000
    pos = knn_ref.cloud(kind, n, seed=4)
    _, _, pairs, _ = _run(ba, pos)
    print("%s: pairs_tested / N = %.1f" % (kind, pairs / n))
    assert 32 <= pairs / n <= 4096


def test_edge_cases(ba):
    for n in range(0, 3):
        pos = knn_ref.cloud("uniform", 3, seed=9)[:n]
        ls, nn, pairs, _ = _run(ba, pos)
        assert np.array_equal(ls, np.zeros(n, np.float32))
        if n == 2:
            d = np.sqrt(knn_ref.sq_dist_f32(pos[0], pos[1]))
            assert np.array_equal(nn, np.array([[d, np.inf], [d, np.inf]], np.float32))
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32)
    ls, nn, _, _ = _run(ba, pos)
    _check_exact(pos, ls, nn)
    same = np.full((777, 3), 3.5, np.float32)
    ls, nn, _, _ = _run(ba, same)
    assert np.all(nn == 0.0)
    assert np.all(ls == ls[0]) and knn_ref.ulp_diff(ls[:1], np.float32(np.log(np.float64(np.float32(1e-3))))).max() <= 2
    bad = np.full((300, 3), np.nan, np.float32)
    bad[::3, 0] = np.inf
    bad[1::3, 2] = -np.inf
    ls, nn, pairs, _ = _run(ba, bad)
    assert pairs == 0 and np.all(np.isinf(nn))
    assert knn_ref.ulp_diff(ls, np.full(300, np.float32(np.log(np.float64(np.float32(0.2)))))).max() <= 2   # unit-box fallback: upper clamp 0.2
    one_finite = bad.copy()
    one_finite[5] = (0.1, 0.2, 0.3)
    ls, nn, _, _ = _run(ba, one_finite)
    assert np.all(np.isinf(nn))


def test_transform_inputs_are_not_modified(ba):
    pos = knn_ref.cloud("surface", 5000, seed=6)
    t = torch.from_numpy(pos).cuda()
    before = t.clone()
    ls, nn = ba.knn_log_scales(t, return_distances=True)
    assert torch.equal(t, before)
    ls2 = ba.knn_log_scales(torch.cat([t, torch.zeros((5000, 7), device=t.device)], 1))
    assert torch.equal(ls, ls2)
    _check_exact(pos, ls[:, 0].cpu().numpy(), nn.cpu().numpy())


def test_deterministic(ba):
    pos = knn_ref.cloud("outliers", 300000, seed=8)
    a = _run(ba, pos)
    b = _run(ba, pos)
    assert a[3].tobytes() == b[3].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def test_to_init_splats_defaults(ba):
    pos = knn_ref.cloud("uniform", 4000, seed=10)
    sp = ba.to_init_splats(pos, device="cuda:0")
    tr = sp.transforms.cpu().numpy()
    assert np.array_equal(tr[:, :3], pos)
    assert np.array_equal(tr[:, 3:7], np.tile(np.array([1, 0, 0, 0], np.float32), (4000, 1)))
    assert np.array_equal(sp.sh_coeffs.cpu().numpy(), np.full((4000, 1, 3), 0.5, np.float32))
    assert np.array_equal(sp.raw_opacities.cpu().numpy(), np.zeros(4000, np.float32))
    assert np.array_equal(tr[:, 7], ba.knn_log_scales(torch.from_numpy(pos).cuda())[:, 0].cpu().numpy())
    given = np.full((4000, 3), -3.0, np.float32)
    sp2 = ba.to_init_splats(pos, log_scales=given, device="cuda:0")
    assert np.array_equal(sp2.transforms.cpu().numpy()[:, 7:10], given)


def test_load_init_splats_from_a_points_only_ply(ba):
    n = 30000
    pos = knn_ref.cloud("surface", n, seed=11)
    rgb = np.random.default_rng(11).integers(0, 256, (n, 3)).astype(np.uint8)
    data = knn_ref.points_ply(pos, rgb)
    sp, meta = ba.load_init_splats(data, device="cuda:0")
    plain, _ = ba.load_splat_from_ply(data, device="cuda:0")
    tr, tp = sp.transforms.cpu().numpy(), plain.transforms.cpu().numpy()
    assert np.all(tp[:, 7:10] == -4.0)   # into_splats is unchanged
    want = ba.knn_log_scales(plain.transforms[:, :3].contiguous())[:, 0].cpu().numpy()
    assert np.array_equal(tr[:, 7], want) and np.array_equal(tr[:, 9], want)
    assert tr[:, :7].tobytes() == tp[:, :7].tobytes()
    assert sp.sh_coeffs.cpu().numpy().tobytes() == plain.sh_coeffs.cpu().numpy().tobytes()
    assert sp.raw_opacities.cpu().numpy().tobytes() == plain.raw_opacities.cpu().numpy().tobytes()
    _check_exact(pos, tr[:, 7], ba.knn_log_scales(torch.from_numpy(pos).cuda(), return_distances=True)[1].cpu().numpy(),
                 np.arange(0, n, 7))
    # max_splats: the kNN runs over the kept rows only
    sub, meta = ba.load_init_splats(data, max_splats=10000, device="cuda:0")
    kept = sub.transforms.cpu().numpy()
    assert meta.total_splats == kept.shape[0] == 10000
    assert np.array_equal(kept[:, :3], pos[::3][:10000])
    _check_exact(kept[:, :3].copy(), kept[:, 7], ba.knn_log_scales(sub.transforms[:, :3].contiguous(), return_distances=True)[1].cpu().numpy())


def test_load_init_splats_keeps_file_scales(ba):
    from oracle import ply
    rng = np.random.default_rng(12)
    tr = rng.normal(size=(5000, 10)).astype(np.float32)
    data = ply.splat_to_ply(tr, rng.normal(size=(5000, 4, 3)).astype(np.float32), rng.normal(size=5000).astype(np.float32))
    sp, _ = ba.load_init_splats(data, device="cuda:0")
    plain, _ = ba.load_splat_from_ply(data, device="cuda:0")
    for a, b in ((sp.transforms, plain.transforms), (sp.sh_coeffs, plain.sh_coeffs), (sp.raw_opacities, plain.raw_opacities)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    comp = ply.make_compressed_ply(1000, 1, seed=5)
    sc, _ = ba.load_init_splats(comp, device="cuda:0")
    pc, _ = ba.load_splat_from_ply(comp, device="cuda:0")
    assert sc.transforms.cpu().numpy().tobytes() == pc.transforms.cpu().numpy().tobytes()


def test_cpp_knn_program_passes_on_the_gpu(tmp_path):
    exe = build_knn_cpp(tmp_path)
    p = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    for line in ("ok knn_log_scales", "ok to_init_splats", "ok load_init_splats", "all C++ kNN checks passed"):
        assert line in p.stdout
