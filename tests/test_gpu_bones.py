"""GPU (-m gpu): k-means, surface sampling and reinit_bones (moda_amd/bones.py, feeders.reinit_bones, csrc/bones_kernels.hip)
against the float64 oracle tests/bones_numpy.py.  Every bar is derived, with u = 2^-24 (fp32 unit round-off, half an ulp):

  assign    as test_gpu_mesh_eval's `nearest`: d = fma(dz, dz, fma(dy, dy, dx * dx)) carries at most 5 roundings on the path of any
            term, and the kernel minimises ITS distances, so in float64 its choice is a minimum up to (1 + 10 u); the index is
            compared exactly wherever the runner-up is further than that, and at most 0.1 % of the points may be left out.
  centres   float64 sums of n exact terms (relative error n 2^-53, far below fp32) divided once and rounded once to fp32: within
            one fp32 ulp of the float64 mean over the kernel's own assignment; counts are integers: exact.
  trajectory  test_bones_oracle.py asserts on the CPU that no point of any iteration is within 1e-5 (relative) of changing
            cluster and no stopping test within 1e-3 of tol, while one ulp in a centre moves a distance ratio by about 4e-7: the
            kernel must take the oracle's branches, so iteration count and assignment are equal and centres within one ulp.
  sampler   areas of the test meshes are exact in fp32 (dyadic, planar), so the CDFs agree to float64 rounding and the face is
            compared exactly (margins asserted on the CPU).  Point: s = sqrtf(u1) is within 1 ulp = 2 u (the bound HIP documents
            for sqrtf); w0 = 1 - s: 3 u absolute; w1 = s (1 - u2): 4 u; w2 = s u2: 3 u; p = fma(w2, c, fma(w1, b, w0 a)) adds one
            rounding per step on partial sums bounded by |a| + |b| + |c|: |p - p64| <= 8 u (|a| + |b| + |c|) per coordinate.
            Barycentrics recovered from p move by that bound over the face's smallest altitude.
  areas     (random mesh) each cross component is a difference of two rounded products of rounded differences: at most 4 u
            relative on each product, so 8 u |e1| |e2| covers the component, the squares, the sum and the square root.
  reinit    bone_transform (render_kernels.hip) forms c' = R c + 2 t: R's entries carry about 5 roundings, each product one
            more, the sum three: 16 u |c| with |R c|_1 <= sqrt 3 |c|, and t = d (x) r^-1 about 6 roundings, 12 u |t|.  The head's
            quaternion is unit to about 4 u, so R R^T deviates from 1 by 8 u.  Forward after inverse: 2 (16 u c* + 12 u |t|) + 8 u |c|
            with c* = max(|c|, |b|) and |t| <= |c| + |b|: under 64 u (max|c| + max|b|)."""
import types

import numpy as np
import pytest
import torch

import bones_numpy as bn
import pointset_numpy as psn
from test_bones_oracle import TRAJECTORIES, trajectory_case, sampler_meshes, sampler_u

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import moda_amd
    from moda_amd import bones as B, feeders as FD, mesh as M
    from gpu_helpers import T, DEV, make_models

U = 2.0 ** -24


def cloud(seed, n):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 3)).astype(np.float32)


def ti(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def np_(t):
    return t.detach().cpu().numpy()


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def check_assignment(X, C, a):
    """`a` (N,) against the centres C the step started from, as test_gpu_mesh_eval.check_nearest."""
    assert a.min() >= 0 and a.max() < len(C)
    dmin, imin, second = psn.nearest(X, C, with_second=True)
    d_at = ((X.astype(np.float64) - C.astype(np.float64)[a]) ** 2).sum(1)
    print("N", len(X), "K", len(C), "max d64[assign] / min d64 - 1 in u:", (d_at / np.maximum(dmin, 1e-300) - 1).max() / U)
    assert (d_at <= (1 + 10 * U) * dmin).all()
    clear = second > (1 + 10 * U) * dmin
    left_out = int((~clear).sum())
    print("   points left out of the exact comparison:", left_out)
    assert left_out <= 1e-3 * len(X)
    assert np.array_equal(a[clear], imin[clear])


def check_update(X, a, K, centers, counts):
    """centres against the float64 mean over the kernel's own assignment (every cluster non-empty), counts exactly."""
    want_n = np.bincount(a, minlength=K)
    assert np.array_equal(counts, want_n) and want_n.min() > 0
    X64 = X.astype(np.float64)
    want = np.stack([X64[a == k].sum(0) / want_n[k] for k in range(K)])
    err = np.abs(centers.astype(np.float64) - want) / ulp32(want)
    print("   max |centre - float64 mean| in fp32 ulps:", err.max())
    assert (err <= 1.0).all()


# (263000, 5) is added to the issue's shapes: 70001 points make 274 workgroups, under MODA_KMEANS_MAX_BLOCKS = 1024; this one
# makes the grid stride (1028 blocks' worth of points on 1024)
@pytest.mark.parametrize("N,K", [(1, 1), (64, 64), (257, 3), (1500, 25), (70001, 25), (263000, 5)])
def test_one_step_matches_oracle(N, K):
    X = cloud(300 + N % 11, N)
    init = np.random.default_rng(400 + N % 13).permutation(N)[:K]
    res = moda_amd.kmeans(T(X), K, init=ti(init), tol=0.0, iter_limit=1)
    a, c = res
    assert a.dtype == torch.int64 and a.shape == (N,) and c.dtype == torch.float32 and c.shape == (K, 3) and a.is_cuda and c.is_cuda
    assert res.iterations == 1 and len(res) == 2
    a = np_(a)
    check_assignment(X, X[init], a)
    check_update(X, a, K, np_(c), np_(res.counts))
    if N > 1:
        d = np_(c).astype(np.float64) - X[init].astype(np.float64)
        assert abs(res.shift - np.sqrt((d * d).sum(1)).sum()) <= 1e-12 * max(res.shift, 1.0)


@pytest.mark.parametrize("N,seed,iterations", TRAJECTORIES)
def test_trajectory_matches_oracle(N, seed, iterations):
    X, init = trajectory_case(N, seed)
    want = bn.kmeans(X, init, tol=1e-4, iter_limit=100)
    res = moda_amd.kmeans(T(X), 25, init=ti(init), tol=1e-4, iter_limit=100)
    print("N", N, "iterations", res.iterations, "oracle", want.iterations, "shift", res.shift, "oracle", want.shifts[-1])
    assert res.iterations == want.iterations == iterations
    assert np.array_equal(np_(res[0]), want.assign)
    err = np.abs(np_(res[1]).astype(np.float64) - want.centers.astype(np.float64)) / ulp32(want.centers)
    print("   max centre difference in fp32 ulps:", err.max())
    assert (err <= 1.0).all()
    assert np.array_equal(np_(res.counts), want.counts)


def test_runs_are_bit_identical():
    X = T(cloud(41, 70001))
    init = ti(np.random.default_rng(42).permutation(70001)[:25])
    r1 = moda_amd.kmeans(X, 25, init=init, iter_limit=100)
    r2 = moda_amd.kmeans(X, 25, init=init, iter_limit=100)
    assert r1.iterations == r2.iterations and r1.shift == r2.shift
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1]) and torch.equal(r1.counts, r2.counts)
    s1 = moda_amd.kmeans(X, 25, seed=7, iter_limit=3)                       # the seeded start is reproducible too
    s2 = moda_amd.kmeans(X, 25, seed=7, iter_limit=3)
    assert torch.equal(s1[0], s2[0]) and torch.equal(s1[1], s2[1]) and s1.iterations == 3


def test_identical_points_and_duplicate_init():
    """All centres equal: every distance ties and cluster 0 takes everything; the empty clusters take the points the rule names."""
    N, K, seed = 1000, 3, 12345
    P = np.tile(np.asarray([[0.25, -0.5, 0.75]], np.float32), (N, 1))
    res = moda_amd.kmeans(T(P), K, init=ti(np.asarray([0, 1, 2])), seed=seed, iter_limit=100)
    assert res.iterations == 1 and res.shift == 0.0                         # nothing moves: the first stopping test passes
    assert int(res[0].abs().max()) == 0 and np_(res.counts).tolist() == [N, 0, 0]
    assert np.array_equal(np_(res[1]), P[:3])
    X = cloud(43, N)
    r1 = moda_amd.kmeans(T(X), K, init=ti(np.asarray([5, 5, 5])), seed=seed, tol=0.0, iter_limit=1)
    assert int(r1[0].abs().max()) == 0 and np_(r1.counts).tolist() == [N, 0, 0]
    c1 = np_(r1[1])
    for k in (1, 2):
        p = bn.empty_point(seed, 0, k, K, N)
        assert p == B.empty_cluster_point(seed, 0, k, K, N) and np.array_equal(c1[k], X[p]), k
    assert (np.abs(c1[0] - X.astype(np.float64).mean(0)) <= ulp32(X.astype(np.float64).mean(0))).all()
    assert not np.array_equal(c1[1], c1[2])
    r2 = moda_amd.kmeans(T(X), K, init=ti(np.asarray([5, 5, 5])), seed=seed, tol=0.0, iter_limit=2)
    assert r2.iterations == 2
    check_assignment(X, c1, np_(r2[0]))                                     # the second step starts from the first one's centres
    want = bn.update_step(X, np_(r2[0]), c1, seed, 1)
    assert np.array_equal(np_(r2.counts), want[1])
    assert (np.abs(np_(r2[1]).astype(np.float64) - want[0]) <= ulp32(want[0])).all()


def test_iteration_limit_and_steps_past_convergence():
    N, seed, iterations = TRAJECTORIES[0]
    X, init = trajectory_case(N, seed)
    one = moda_amd.kmeans(T(X), 25, init=ti(init), iter_limit=1)
    assert one.iterations == 1
    # iterations are enqueued 16 at a time: the free run enqueues 32 for 21, the limited one exactly 21
    free = moda_amd.kmeans(T(X), 25, init=ti(init), tol=1e-4, iter_limit=100)
    exact = moda_amd.kmeans(T(X), 25, init=ti(init), tol=1e-4, iter_limit=iterations)
    assert free.iterations == exact.iterations == iterations and iterations % 16 != 0
    assert torch.equal(free[0], exact[0]) and torch.equal(free[1], exact[1]) and free.shift == exact.shift
    unlimited = moda_amd.kmeans(T(X), 25, init=ti(init), tol=1e-4, iter_limit=0)
    assert unlimited.iterations == iterations and torch.equal(unlimited[1], free[1])


# ---- sampler ------------------------------------------------------------------------------------------------------------
def point_bound(verts, faces, face):
    tri = np.abs(verts.astype(np.float64)[faces[face]])                     # (S, 3 corners, 3)
    return 8 * U * tri.sum(1)


def check_on_face(verts, faces, face, pts, bound):
    v = verts.astype(np.float64)
    a, b, c = (v[faces[face][:, i]] for i in range(3))
    e1, e2, d = b - a, c - a, pts - a
    g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    r1, r2 = (d * e1).sum(1), (d * e2).sum(1)
    det = g11 * g22 - g12 * g12
    w1, w2 = (g22 * r1 - g12 * r2) / det, (g11 * r2 - g12 * r1) / det
    w0 = 1 - w1 - w2
    off = np.abs(d - w1[:, None] * e1 - w2[:, None] * e2).max(1)            # distance from the face's plane, per coordinate
    longest = np.sqrt(np.maximum(np.maximum(g11, g22), ((c - b) ** 2).sum(1)))
    altitude = np.sqrt(det) / longest
    slack = np.sqrt(3) * bound.max(1) / altitude
    print("   max off-plane / bound:", (off / bound.max(1)).max(), "min barycentric / slack:", (np.minimum(np.minimum(w0, w1), w2) / slack).min())
    assert (off <= np.sqrt(3) * bound.max(1)).all()
    assert (w0 >= -slack).all() and (w1 >= -slack).all() and (w2 >= -slack).all()


@pytest.mark.parametrize("name", ["one", "two", "strip"])
def test_sampler_matches_oracle(name):
    verts, faces = sampler_meshes()[name]
    u = sampler_u(1000)
    pts, face, areas, cdf = moda_amd.sample_surface(T(verts), ti(faces), T(u))
    assert pts.shape == (1000, 3) and pts.dtype == torch.float32 and face.dtype == torch.int32 and cdf.dtype == torch.float64
    want_areas, want_cdf = bn.face_cdf(verts, faces)
    assert np.array_equal(np_(areas), want_areas)                           # exact by construction of the meshes
    assert np.array_equal(np_(cdf), want_cdf)                               # dyadic: every partial sum is exact in any order
    want_face, want_pts, _, _ = bn.sample(verts, faces, u)
    face = np_(face).astype(np.int64)
    assert np.array_equal(face, want_face)
    bound = point_bound(verts, faces, face)
    err = np.abs(np_(pts).astype(np.float64) - want_pts)
    print(name, "max |p - p64| / bound:", (err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all()
    check_on_face(verts, faces, face, np_(pts).astype(np.float64), bound)
    out = moda_amd.sample_points_from_meshes(T(verts), ti(faces), u=T(u))
    assert torch.equal(out, pts)


def test_sampler_random_mesh():
    """Areas that are not exact: the areas and the CDF within their bounds, the face exactly the one the kernel's own CDF names."""
    rng = np.random.default_rng(9)
    V, F, S = 700, 5000, 4000
    verts = rng.uniform(-1, 1, (V, 3)).astype(np.float32)
    faces = rng.integers(0, V, (F, 3)).astype(np.int32)
    faces[::97, 1] = faces[::97, 0]                                         # some faces of area exactly 0
    u = sampler_u(S, 10)
    pts, face, areas, cdf = moda_amd.sample_surface(T(verts), ti(faces), T(u))
    areas, cdf, face = np_(areas), np_(cdf), np_(face).astype(np.int64)
    v = verts.astype(np.float64)
    e1, e2 = v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]
    lim = 8 * U * np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)
    err = np.abs(areas - bn.face_areas(verts, faces))
    print("max area error / bound:", (err[lim > 0] / lim[lim > 0]).max())
    assert (err <= lim).all() and (areas[::97] == 0).all()
    ref = np.cumsum(areas.astype(np.float64))
    assert (np.abs(cdf - ref) <= F * 2.0 ** -53 * ref).all()
    t = u[:, 0].astype(np.float64) * cdf[-1]
    below = np.where(face > 0, cdf[np.maximum(face - 1, 0)], 0.0)
    assert (cdf[face] > t).all() and (below <= t).all() and (areas[face] > 0).all()
    bound = point_bound(verts, faces, face)
    s = np.sqrt(u[:, 1].astype(np.float64))
    w = np.stack([1 - s, s * (1 - u[:, 2].astype(np.float64)), s * u[:, 2].astype(np.float64)], 1)
    want = (w[:, :, None] * v[faces[face]]).sum(1)
    assert (np.abs(np_(pts) - want) <= bound).all()


def test_sampler_statistics_batches_and_meshes():
    verts, faces = sampler_meshes()["two"]
    S = 200000
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    u = torch.rand((S, 3), generator=g, device=DEV)
    _, face, _, _ = moda_amd.sample_surface(T(verts), ti(faces), u)
    share = float((face == 1).double().mean())
    sigma = np.sqrt(0.75 * 0.25 / S)
    print("share of the larger face:", share, "sigma", sigma)
    assert abs(share - 0.75) <= 5 * sigma
    # batched input equals the per-item calls bit for bit
    (v0, f0), (v1, f1) = bn.strip_mesh(2051, 5), bn.strip_mesh(2051, 6)
    vb, fb = T(np.stack([v0, v1])), ti(np.stack([f0, f1]))
    ub = T(np.stack([sampler_u(777, 1), sampler_u(777, 2)]))
    out = moda_amd.sample_points_from_meshes(vb, fb, u=ub)
    assert out.shape == (2, 777, 3)
    for b in range(2):
        assert torch.equal(out[b], moda_amd.sample_points_from_meshes(vb[b], fb[b], u=ub[b]))
    # a TriMesh, the default uniforms, a generator
    mesh = M.TriMesh(T(v0), ti(f0))
    ga, gb = torch.Generator(device=DEV), torch.Generator(device=DEV)
    ga.manual_seed(3)
    gb.manual_seed(3)
    p1 = moda_amd.sample_points_from_meshes(mesh, num_samples=1000, generator=ga)
    p2 = moda_amd.sample_points_from_meshes(T(v0), ti(f0).long(), 1000, generator=gb)
    assert p1.shape == (1000, 3) and torch.equal(p1, p2)
    assert moda_amd.sample_points_from_meshes(mesh).shape == (10000, 3)
    assert float(p1[:, 2].abs().max()) == 0 and float(p1[:, 1].min()) >= 0 and float(p1[:, 1].max()) <= 1


# ---- reinit_bones -------------------------------------------------------------------------------------------------------
def small_model(K, extra_bones=3):
    models, _ = make_models(17, K, with_skin=True, perturb_bones=True)
    model = types.SimpleNamespace(device=DEV)
    model.pose_code = FD.FrameCode(6, 128, np.asarray([0, 50])).to(DEV)
    head = FD.DQ_RTHead(use_quat=True, in_channels_xyz=128, in_channels_dir=0, out_channels=7 * K, raw_feat=True).to(DEV).eval()
    with torch.no_grad():
        head.rgb[0].bias.copy_(torch.tensor([0, 0, 0, 1, 0, 0, 0.0], device=DEV).repeat(K))
    model.nerf_body_rts = torch.nn.Sequential(model.pose_code, head)
    model.rest_pose_code = models["rest_pose_code"]
    model.bones = torch.nn.Parameter(torch.cat([models["bones_rst"], models["bones_rst"][:extra_bones] + 5.0]).clone())
    model.nerf_models = {}
    model.num_bones = 0
    model.latest_vars = {"obj_bound": np.asarray([0.2, 0.15, 0.25], np.float32)}
    return model, head


def pinned_reinit(mesh, K, init, seed):
    """reinit_bones on a fresh small model with k-means' random start replaced by `init` (reinit_bones passes no start) and the
    torch seed fixed for the head's xavier draw.  -> model, head, the head's state and the bones before the call."""
    torch.manual_seed(seed)                                                 # the head's other layers are drawn here
    model, head = small_model(K)
    before = {k: v.clone() for k, v in head.state_dict().items()}
    bones_before = model.bones.detach().clone()
    orig = B.kmeans
    torch.manual_seed(seed + 1)
    try:
        B.kmeans = lambda **kw: orig(**{**kw, "init": ti(init)})
        moda_amd.reinit_bones(model, mesh, K, True)
    finally:
        B.kmeans = orig
    return model, head, before, bones_before


def test_reinit_bones():
    """The head has exactly 7 K output rows (correct_bones needs head and bones to agree), so 'rows beyond the first 7 K' is
    checked where rows beyond exist: the bones past K, and every other parameter of the head."""
    K = 25
    X, init = trajectory_case(1500, 0)
    known = moda_amd.kmeans(T(X), K, init=ti(init), iter_limit=100)[1]
    mesh = M.TriMesh(T(X), torch.zeros((0, 3), dtype=torch.int32, device=DEV))           # device vertices
    model, head, before, bones_before = pinned_reinit(mesh, K, init, 0)
    assert model.num_bones == K and model.nerf_models["bones"] is model.bones
    after = head.state_dict()
    w = after["rgb.0.weight"]
    assert w.shape[0] == 7 * K and bool((w != before["rgb.0.weight"]).any(dim=1).all())
    assert float(w.abs().max()) <= 0.5 * np.sqrt(6.0 / (w.shape[1] + 7 * K)) + 1e-7       # xavier_uniform_, gain 0.5
    assert float(after["rgb.0.bias"].abs().max()) == 0
    for k in before:
        if not k.startswith("rgb.0."):
            assert torch.equal(before[k], after[k]), k
    assert torch.equal(model.bones[K:], bones_before[K:]) and not torch.equal(model.bones[:K], bones_before[:K])
    back, _ = FD.correct_bones(model, model.bones[:K].detach(), inverse=False)
    err = np.abs(np_(back)[:, :3].astype(np.float64) - np_(known).astype(np.float64)).max()
    tol = 64 * U * (float(known.abs().max()) + float(model.bones[:K, :3].detach().abs().max()))
    print("round trip error", err, "bound", tol)
    assert err <= tol
    rest = np.tile(np.asarray([1, 0, 0, 0, 0, 0, 0], np.float32), (K, 1))              # orientation 1, log-scale 0
    assert np.abs(np_(back)[:, 3:] - rest).max() <= 64 * U
    # anything with .vertices (host, float64) gives the same bones
    model2, _, _, _ = pinned_reinit(types.SimpleNamespace(vertices=X.astype(np.float64)), K, init, 0)
    assert torch.equal(model2.bones, model.bones)


def test_reinit_bones_small_mesh_and_refusal():
    K = 25
    model, _ = small_model(K)
    few = types.SimpleNamespace(vertices=cloud(3, 99).astype(np.float64))
    moda_amd.reinit_bones(model, few, K, True)
    back, _ = FD.correct_bones(model, model.bones[:K].detach(), inverse=False)
    bound = model.latest_vars["obj_bound"].astype(np.float64)
    c = np_(back)[:, :3].astype(np.float64)
    slack = 64 * U * (np.abs(c).max() + float(model.bones[:K, :3].detach().abs().max()))
    assert (np.abs(c) <= bound[None] + slack).all() and np.unique(c, axis=0).shape[0] == K
    with pytest.raises(NotImplementedError):
        moda_amd.reinit_bones(model, few, K, False)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals():
    X = T(cloud(1, 100))
    bad = X.clone()
    bad[17, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        moda_amd.kmeans(bad, 5)
    bad[17, 1] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        moda_amd.kmeans(bad, 5)
    with pytest.raises(ValueError):
        moda_amd.kmeans(X[:4], 5)
    with pytest.raises(ValueError):
        moda_amd.kmeans(T(cloud(1, 100)), 65)
    with pytest.raises(ValueError):
        moda_amd.kmeans(X.reshape(50, 6), 5)
    with pytest.raises(ValueError):
        moda_amd.kmeans(X, 5, init=ti(np.asarray([0, 1, 2, 3, 100])))
    with pytest.raises(ValueError):
        moda_amd.kmeans(X, 5, tol=0.0)
    with pytest.raises(NotImplementedError, match="distance"):
        moda_amd.kmeans(X, 5, distance="cosine")
    with pytest.raises(NotImplementedError, match="cluster_centers"):
        moda_amd.kmeans(X, 5, cluster_centers=X[:5])
    a, c = moda_amd.kmeans(X.cpu(), 5, device=DEV, iter_limit=2)            # a host tensor is moved, as the package does
    assert a.is_cuda and c.is_cuda
    verts, faces = sampler_meshes()["two"]
    v, f = T(verts), ti(faces)
    with pytest.raises(NotImplementedError, match="return_normals"):
        moda_amd.sample_points_from_meshes(v, f, 10, return_normals=True)
    with pytest.raises(NotImplementedError, match="grad"):
        moda_amd.sample_points_from_meshes(v.clone().requires_grad_(True), f, 10)
    with pytest.raises(ValueError, match="area"):
        moda_amd.sample_points_from_meshes(v * 0, f, 10)
    vn = v.clone()
    vn[2, 0] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        moda_amd.sample_points_from_meshes(vn, f, 10)
    with pytest.raises(ValueError, match="no faces"):
        moda_amd.sample_points_from_meshes(v, f[:0], 10)
    fb = f.clone()
    fb[1, 2] = 6
    with pytest.raises(ValueError, match="outside"):
        moda_amd.sample_points_from_meshes(v, fb, 10)
    fb[1, 2] = -1
    with pytest.raises(ValueError, match="outside"):
        moda_amd.sample_points_from_meshes(v, fb, 10)
    with pytest.raises(ValueError, match="u outside"):
        moda_amd.sample_points_from_meshes(v, f, u=torch.ones((4, 3), device=DEV))
