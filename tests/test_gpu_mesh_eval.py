"""GPU (-m gpu): mesh evaluation (moda_amd/mesh_eval.py, csrc/pointset_kernels.hip) against the float64 oracle
tests/pointset_numpy.py.  Every bar is derived, with u = 2^-24 (fp32 unit round-off):

  nearest   dist2 is three differences, three squares (one as a product, two inside FMAs) and two sums: at most 5 roundings
            on the path of any term, so |dist2 - d64[idx]| <= 5 u d64[idx]; the kernel's choice minimises ITS distances,
            so in float64 it is a minimum up to (1 + 10 u); idx is compared exactly wherever the runner-up is further than
            that, and at most 0.1 % of the queries may be left out on that ground.
  chamfer   gradient terms 2 g (x - y): two roundings per component, then a sum of k terms: (4 + k_max) u sum|terms|.
  icp       fp32 coordinates of size 0.3 round at about 2e-8; 1e-5 leaves more than 100x for accumulated rounding while one
            wrong correspondence costs about the point spacing, 1e-2.
  eval_mesh F-scores are counts: they may differ from the oracle's only through points within 5 u (relative) of a threshold,
            which are counted in float64; cd to 1e-5 relative."""
import ctypes

import numpy as np
import pytest
import torch

import pointset_numpy as psn
from helpers import golden

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import moda_amd
    from moda_amd import mesh as M, mesh_eval as ME, _lib
    from gpu_helpers import T, DEV

U = 2.0 ** -24


def cloud(seed, *shape):
    return np.random.default_rng(seed).uniform(-1, 1, shape + (3,)).astype(np.float32)


def raw_nn(x, y, with_keys):
    """moda_nn_fwd on (B,N,3) / (B,M,3) device tensors, with or without the split workspace."""
    B, N, Mm = x.shape[0], x.shape[1], y.shape[1]
    d = torch.empty((B, N), dtype=torch.float32, device=DEV)
    i = torch.empty((B, N), dtype=torch.int32, device=DEV)
    keys = torch.empty((B, N), dtype=torch.int64, device=DEV) if with_keys else None
    _lib.call("moda_nn_fwd", _lib.ptr(x), _lib.ptr(y), B, N, Mm, _lib.ptr(d), _lib.ptr(i), _lib.ptr(keys), _lib.stream())
    return d, i


def check_nearest(x, y, d, i):
    d, i = d.cpu().numpy().astype(np.float64), i.cpu().numpy().astype(np.int64)
    assert i.min() >= 0 and i.max() < len(y)
    dmin, imin, second = psn.nearest(x, y, with_second=True)
    d_at = ((x.astype(np.float64) - y.astype(np.float64)[i]) ** 2).sum(1)
    e1 = np.abs(d - d_at) / np.maximum(d_at, 1e-300)
    print("N", len(x), "M", len(y), "max |dist2 - d64[idx]| / d64[idx] in u:", e1.max() / U,
          "max d64[idx] / min d64 - 1 in u:", (d_at / np.maximum(dmin, 1e-300) - 1).max() / U)
    assert (np.abs(d - d_at) <= 5 * U * d_at).all()
    assert (d_at <= (1 + 10 * U) * dmin).all()
    clear = second > (1 + 10 * U) * dmin
    left_out = int((~clear).sum())
    print("   queries left out of the exact index comparison:", left_out)
    assert left_out <= 1e-3 * len(x)
    assert np.array_equal(i[clear], imin[clear])


@pytest.mark.parametrize("N,Mm", [(1, 1), (257, 1), (1, 5003), (4096, 5003), (37, 70001)])
def test_nearest_matches_oracle(N, Mm):
    x, y = cloud(100 + N % 7, N), cloud(200 + Mm % 7, Mm)
    d, i = ME.nearest(T(x), T(y))
    assert d.shape == (N,) and i.shape == (N,) and d.dtype == torch.float32 and i.dtype == torch.int32
    check_nearest(x, y, d, i)
    d2, i2 = raw_nn(T(x)[None], T(y)[None], with_keys=False)                  # the unsplit route gives the same bits
    assert torch.equal(d2[0], d) and torch.equal(i2[0], i)


def test_nearest_batched():
    x, y = cloud(7, 3, 1300), cloud(8, 3, 2500)
    d, i = ME.nearest(T(x), T(y))
    assert d.shape == (3, 1300) and i.shape == (3, 1300)
    for b in range(3):
        check_nearest(x[b], y[b], d[b], i[b])


@pytest.mark.parametrize("N,K,copies", [(500, 700, 3), (300, 23333, 3)])
def test_tie_rule_lowest_index(N, K, copies):
    """Every target appears `copies` times, K apart: identical coordinates give bit-identical distances, and the lowest copy
    must be returned, on the split route (copies in different ranges) and on the unsplit one."""
    P = cloud(31, K)
    y = np.tile(P, (copies, 1))
    rng = np.random.default_rng(32)
    sel = rng.integers(0, K, N)
    x = (P[sel] + rng.uniform(-1e-4, 1e-4, (N, 3))).astype(np.float32)
    x[:20] = P[sel[:20]]                                                     # distance exactly 0 as well
    splits, rg = ME.nn_plan(1, N, len(y))
    if K > 1024:
        assert splits > 1 and K >= rg, (splits, rg)                          # copies j, j + K, j + 2K lie in different ranges
    _, want = psn.nearest(x, y)
    assert (want < K).all()
    for with_keys in (True, False):
        d, i = raw_nn(T(x)[None], T(y)[None], with_keys)
        assert np.array_equal(i[0].cpu().numpy(), want), with_keys
    d, i = ME.nearest(T(x), T(y))
    assert np.array_equal(i.cpu().numpy(), want) and (d[:20] == 0).all()


def test_bit_identical_runs():
    x, y = cloud(41, 1, 1500), cloud(42, 1, 70001)
    assert ME.nn_plan(1, 1500, 70001)[0] > 1
    a, b = ME.nearest(T(x), T(y)), ME.nearest(T(x), T(y))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    xt = T(cloud(43, 1, 1500))
    s1, s2 = ME.icp_moments(T(x), T(y), a[1], xt), ME.icp_moments(T(x), T(y), a[1], xt)
    assert torch.equal(s1, s2)


def test_icp_moments_match_oracle():
    x, y, xt = cloud(51, 2, 5000), cloud(52, 2, 777), cloud(53, 2, 5000)
    idx = torch.from_numpy(np.random.default_rng(54).integers(0, 777, (2, 5000)).astype(np.int32)).to(DEV)
    s = ME.icp_moments(T(x), T(y), idx, T(xt)).cpu().numpy()
    for b in range(2):
        p, q, r = x[b].astype(np.float64), y[b].astype(np.float64)[idx[b].cpu().numpy()], xt[b].astype(np.float64)
        want = np.concatenate([p.sum(0), q.sum(0), (p.T @ q).reshape(-1), [(p * p).sum()], [((r - q) ** 2).sum()]])
        scale = np.concatenate([np.abs(p).sum(0), np.abs(q).sum(0), (np.abs(p).T @ np.abs(q)).reshape(-1), [(p * p).sum()],
                                [((r - q) ** 2).sum()]])
        assert (np.abs(s[b] - want) <= 5000 * 2.0 ** -53 * scale).all()      # float64 sums of 5000 exact terms


def test_chamfer_forward_and_backward():
    x, y = cloud(61, 2, 700), cloud(62, 2, 900)
    xt, yt = T(x).requires_grad_(True), T(y).requires_grad_(True)
    cham = moda_amd.chamfer_3DDist()
    d1, d2, i1, i2 = cham(xt, yt)
    n1, n2 = ME.nearest(T(x), T(y)), ME.nearest(T(y), T(x))
    assert torch.equal(d1, n1[0]) and torch.equal(i1, n1[1]) and torch.equal(d2, n2[0]) and torch.equal(i2, n2[1])
    assert i1.dtype == torch.int32 and i2.dtype == torch.int32 and d1.shape == (2, 700) and d2.shape == (2, 900)
    rng = np.random.default_rng(63)
    g1, g2 = rng.standard_normal((2, 700)).astype(np.float32), rng.standard_normal((2, 900)).astype(np.float32)
    ((T(g1) * d1).sum() + (T(g2) * d2).sum()).backward()
    for b in range(2):
        _, _, o1, o2 = psn.chamfer(x[b], y[b])
        assert np.array_equal(o1, i1[b].cpu().numpy()) and np.array_equal(o2, i2[b].cpu().numpy())
        gx, gy, ax, ay, cx, cy = psn.chamfer_grad(x[b], y[b], o1, o2, g1[b], g2[b])
        k_max = int(max(cx.max(), cy.max()))
        ex = np.abs(xt.grad[b].cpu().numpy() - gx) / np.maximum(ax, 1e-300)
        ey = np.abs(yt.grad[b].cpu().numpy() - gy) / np.maximum(ay, 1e-300)
        print("batch", b, "k_max", k_max, "max err / sum|terms| in u:", ex.max() / U, ey.max() / U)
        assert (np.abs(xt.grad[b].cpu().numpy() - gx) <= (4 + k_max) * U * ax).all()
        assert (np.abs(yt.grad[b].cpu().numpy() - gy) <= (4 + k_max) * U * ay).all()
    with torch.no_grad():
        e = cham(T(x), T(y))
    assert torch.equal(e[0], d1) and not e[0].requires_grad


def test_chamfer_bwd_skips_bad_indices():
    x, y = T(cloud(71, 1, 8)), T(cloud(72, 1, 5))
    idx = torch.tensor([[0, -1, 5, 4, 2 ** 30, -2 ** 31, 1, 7]], dtype=torch.int32, device=DEV)
    g = torch.ones((1, 8), device=DEV)
    gx, gy = torch.zeros_like(x), torch.zeros_like(y)
    _lib.call("moda_chamfer_bwd", _lib.ptr(x), _lib.ptr(y), _lib.ptr(idx), _lib.ptr(g), 1, 8, 5, _lib.ptr(gx), _lib.ptr(gy),
              _lib.stream())
    touched = (gx[0] != 0).any(1).cpu().numpy()
    assert touched.tolist() == [True, False, False, True, False, False, True, False]
    assert torch.allclose(gx.sum(1), -gy.sum(1), atol=1e-6)


def test_fscore_matches_reference_fixture():
    g = golden("g28_fscore")
    for name in g["cases"].tolist():
        d1, d2 = T(g[f"{name}_dist1"]), T(g[f"{name}_dist2"])
        for k, thr in enumerate(g[f"{name}_thresholds"].tolist()):
            f, p1, p2 = moda_amd.fscore(d1, d2, threshold=thr)
            assert np.array_equal(f.cpu().numpy(), g[f"{name}_fscore"][k])
            assert np.array_equal(p1.cpu().numpy(), g[f"{name}_precision_1"][k])
            assert np.array_equal(p2.cpu().numpy(), g[f"{name}_precision_2"][k])
    assert np.array_equal(moda_amd.fscore(T(g["a_dist1"]), T(g["a_dist2"]))[0].cpu().numpy(), g["default_threshold_fscore"])


@pytest.mark.parametrize("seed,degrees", [(0, 5.0), (1, 10.0), (2, 15.0), (3, 10.0)])
def test_icp_recovers_known_motion(seed, degrees):
    X, Y, subset, R, T_ = psn.icp_case(seed, degrees)
    sol = moda_amd.iterative_closest_point(T(X)[None], T(Y)[None])
    bbox = float((Y.max(0) - Y.min(0)).max())
    _, idx = ME.nearest(sol.Xt[0], T(Y))
    Rg, Tg = sol.RTs.R[0].cpu().numpy().astype(np.float64), sol.RTs.T[0].cpu().numpy().astype(np.float64)
    print(seed, degrees, "iterations", len(sol.t_history), "rmse", float(sol.rmse[0]), "max |dR|", np.abs(Rg - R).max(),
          "max |dT|", np.abs(Tg - T_).max(), "wrong correspondences", int((idx.cpu().numpy() != subset).sum()))
    assert sol.converged is True and len(sol.t_history) < 100
    assert np.array_equal(idx.cpu().numpy(), subset)
    assert float(sol.rmse[0]) <= 1e-5 * bbox
    assert np.abs(Rg - R).max() <= 1e-5 and np.abs(Tg - T_).max() <= 1e-5 and float(sol.RTs.s[0]) == 1.0
    assert sol.Xt.shape == (1, 1500, 3) and sol.RTs.R.shape == (1, 3, 3) and sol.RTs.T.shape == (1, 3)
    assert np.abs(sol.Xt[0].cpu().numpy() - Y[subset]).max() <= 1e-5 * bbox


def test_icp_scale_iteration_limit_and_batch():
    X, Y, subset, R, T_ = psn.icp_case(3, 5.0, scale=1.1)
    sol = moda_amd.iterative_closest_point(T(X)[None], T(Y)[None], estimate_scale=True)
    _, idx = ME.nearest(sol.Xt[0], T(Y))
    print("scale", float(sol.RTs.s[0]), "iterations", len(sol.t_history))
    assert sol.converged and np.array_equal(idx.cpu().numpy(), subset) and abs(float(sol.RTs.s[0]) - 1.1) <= 1e-5
    one = moda_amd.iterative_closest_point(T(X)[None], T(Y)[None], max_iterations=1)
    assert one.converged is False and len(one.t_history) == 1
    X, Y, subset, R, T_ = psn.icp_case(0, 10.0)
    a = moda_amd.iterative_closest_point(T(X)[None], T(Y)[None])
    b = moda_amd.iterative_closest_point(T(np.stack([X, X])), T(np.stack([Y, Y])))
    assert a.converged and b.converged and len(a.t_history) == len(b.t_history)
    for k in range(2):
        assert torch.equal(b.Xt[k], a.Xt[0]) and torch.equal(b.rmse[k], a.rmse[0])
        assert torch.equal(b.RTs.R[k], a.RTs.R[0]) and torch.equal(b.RTs.T[k], a.RTs.T[0]) and torch.equal(b.RTs.s[k], a.RTs.s[0])
    # init_transform: starting from the answer converges at once to the same transform
    c = moda_amd.iterative_closest_point(T(X)[None], T(Y)[None], init_transform=a.RTs)
    assert c.converged and len(c.t_history) <= 2 and torch.allclose(c.RTs.R, a.RTs.R, atol=1e-6)


def _sphere(shape, r, offset):
    ax = [np.arange(n, dtype=np.float64) - (n - 1) / 2 + o for n, o in zip(shape, offset)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    return (r - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32)


def test_eval_mesh_matches_oracle():
    shape = (40, 40, 40)
    gt = M.TriMesh(*M.marching_cubes(T(_sphere(shape, 14.0, (0.137, 0.071, -0.053))), 0.0))
    pred = M.TriMesh(*M.marching_cubes(T(_sphere(shape, 14.0 * 1.02, (0.537, -0.229, 0.047))), 0.0))
    out = moda_amd.eval_mesh(pred, gt)
    want = psn.eval_mesh(pred.vertices_t.cpu().numpy(), gt.vertices_t.cpu().numpy())
    print("V", len(pred.vertices), "G", len(gt.vertices), "iterations", len(out["icp"].t_history), "/", len(want["icp"].t_history),
          "cd", out["cd"], want["cd"], "f", [(out[k], want[k]) for k in ("f001", "f002", "f005")])
    assert abs(out["bbox_max"] - want["bbox_max"]) <= 4 * U * want["bbox_max"]
    assert abs(out["cd"] - want["cd"]) <= 1e-5 * want["cd"]
    G, V = len(want["d_gt"]), len(want["d_back"])
    for key in ("f001", "f002", "f005"):
        thr = want["thresholds"][key]
        n1 = int((np.abs(want["d_gt"] - thr) <= 5 * U * thr).sum())
        n2 = int((np.abs(want["d_back"] - thr) <= 5 * U * thr).sum())
        print("  ", key, "points within 5 u of the threshold:", n1, n2)
        # |df/dp1|, |df/dp2| <= 2 for f = 2 p1 p2 / (p1 + p2); f itself is formed in fp32 from fp32 precisions
        assert abs(out[key] - want[key]) <= 2 * (n1 / G + n2 / V) + 8 * U
    assert any(0 < want[k] < 1 for k in ("f001", "f002", "f005"))            # a threshold cuts through the distances
    assert out["raw_cd"].shape == (G,) and out["raw_cd_back"].shape == (V,) and out["verts"].shape == (V, 3)
    assert out["raw_cd"].is_cuda and out["icp"].converged == want["icp"].converged
    same = moda_amd.eval_mesh(pred.vertices, gt.vertices_t)                  # numpy float64 and tensor inputs
    assert same["cd"] == out["cd"] and same["f002"] == out["f002"]


def test_refusals():
    x, y = T(cloud(81, 10)), T(cloud(82, 12))
    for bad in (float("nan"), float("inf"), -float("inf")):
        xb, yb = x.clone(), y.clone()
        xb[3, 1] = bad
        yb[5, 2] = bad
        for a, b in ((xb, y), (x, yb)):
            with pytest.raises(ValueError, match="non-finite"):
                ME.nearest(a, b)
            with pytest.raises(ValueError, match="non-finite"):
                moda_amd.chamfer_3DDist()(a[None], b[None])
            with pytest.raises(ValueError, match="non-finite"):
                moda_amd.iterative_closest_point(a[None], b[None])
            with pytest.raises(ValueError, match="non-finite"):
                moda_amd.eval_mesh(a, b)
    with pytest.raises(ValueError, match="empty"):
        ME.nearest(x, y[:0])
    with pytest.raises(ValueError):
        ME.nearest(x, y[None])
    with pytest.raises(ValueError):
        ME.nearest(x[:, :2], y[:, :2])
    with pytest.raises(ValueError):
        moda_amd.iterative_closest_point(x, y)                               # unbatched
    with pytest.raises(ValueError, match="padded"):
        moda_amd.iterative_closest_point(object(), object())
    d, i = ME.nearest(x[:0], y)
    assert d.shape == (0,) and i.shape == (0,)
    lib = _lib.load()
    assert lib.moda_nn_fwd(None, None, 1, 10, 0, None, None, None, None) == -2
    assert lib.moda_nn_fwd(None, None, 0, 10, 10, None, None, None, None) == -2
    assert lib.moda_nn_fwd(None, None, 2, 2 ** 30, 10, None, None, None, None) == -2
    assert lib.moda_nn_fwd(None, None, 2, 10, 2 ** 30, None, None, None, None) == -2
    assert lib.moda_chamfer_bwd(None, None, None, None, 2, 2 ** 30, 10, None, None, None) == -2
    assert lib.moda_chamfer_bwd(None, None, None, None, 1, 10, 0, None, None, None) == -2
    assert lib.moda_icp_moments(None, None, None, None, 2, 10, 2 ** 30, None, None, None) == -2
    assert lib.moda_icp_moments(None, None, None, None, 1, 10, 0, None, None, None) == -2
    assert lib.moda_nn_fwd(None, None, 1, 10, 10, None, None, None, None) == -1     # valid shape, null pointers: MODA_EINVAL
