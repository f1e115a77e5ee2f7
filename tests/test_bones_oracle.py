"""CPU (-m "not gpu"): the float64 oracle tests/bones_numpy.py against closed forms, the empty-cluster rule against the
published splitmix64 sequence, the bindings of the new entries, and the margin conditions tests/test_gpu_bones.py relies on."""
import os
import re

import numpy as np
import pytest

import bones_numpy as bn
from moda_amd import _lib, bones as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("moda_kmeans_blocks", "moda_kmeans_steps", "moda_mesh_face_cdf", "moda_mesh_sample")

# the inputs of the GPU tests, shared so that what is asserted here is what runs there
TRAJECTORIES = [(1500, 0, 21), (5003, 3, 30)]                               # N, seed, iterations to converge
SAMPLER_SEED = 77


def trajectory_case(N, seed):
    r = np.random.default_rng(seed)
    X = r.uniform(-1, 1, (N, 3)).astype(np.float32)
    return X, r.permutation(N)[:25]


def sampler_meshes():
    """name -> (verts fp32, faces int32): one triangle, two faces of areas 1 : 3, a strip that crosses a scan tile."""
    one = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
    two = (np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 0.5], [6, 0, 0.5], [0, 1, 0.5]], np.float32),
           np.array([[0, 1, 2], [3, 4, 5]], np.int32))
    return {"one": one, "two": two, "strip": bn.strip_mesh(2048 + 3, 5)}


def sampler_u(S, seed=SAMPLER_SEED):
    return np.random.default_rng(seed).random((S, 3), dtype=np.float32)


def test_two_blobs_converge_in_two_iterations():
    r = np.random.default_rng(1)
    a = (r.uniform(-0.1, 0.1, (300, 3)) + [1, 0, 0]).astype(np.float32)
    b = (r.uniform(-0.1, 0.1, (200, 3)) + [-1, 0, 0]).astype(np.float32)
    X = np.concatenate([a, b])
    res = bn.kmeans(X, [0, 300], tol=1e-4, iter_limit=0)
    assert res.iterations == 2                                              # the first step moves to the means, the second not at all
    assert np.array_equal(res.assign, np.r_[np.zeros(300, int), np.ones(200, int)])
    want = np.stack([a.astype(np.float64).mean(0), b.astype(np.float64).mean(0)])
    assert np.abs(res.centers - want).max() <= 2.0 ** -24 * 1.1 and res.shifts[1] == 0.0
    assert list(res.counts) == [300, 200] and res.margin > 1.0


def test_sampler_closed_forms():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    u = np.array([[0.3, 0.25, 0.5], [0.9, 0.0, 0.7], [0.0, 0.64, 0.25]], np.float32)
    face, pts, w, _ = bn.sample(verts, faces, u)
    assert np.array_equal(face, [0, 0, 0])
    # s = sqrt(u1): (0.5, 0, 0.8); w = (1 - s, s (1 - u2), s u2); on this triangle p = (w1, w2, 0)
    want_w = np.array([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.2, 0.6, 0.2]])
    assert np.abs(w - want_w).max() < 1e-7                                  # u is fp32: 0.64 and 0.7 are not exact
    assert np.abs(pts - np.stack([want_w[:, 1], want_w[:, 2], np.zeros(3)], 1)).max() < 1e-7
    assert bn.face_areas(verts, faces)[0] == 0.5


def test_zero_area_face_is_never_selected():
    verts = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    faces = np.array([[0, 1, 2], [0, 1, 3], [1, 1, 4], [0, 3, 4], [0, 2, 1]], np.int32)     # 0, 2, 4: zero area
    areas, cdf = bn.face_cdf(verts, faces)
    assert list(areas) == [0, 0.5, 0, 0.5, 0]
    u = np.concatenate([np.array([[0.0, 0.5, 0.5], [0.5, 0.5, 0.5], [np.nextafter(np.float32(1), np.float32(0)), 0.5, 0.5],
                                  [np.nextafter(np.float32(0.5), np.float32(0)), 0.1, 0.1]], np.float32), sampler_u(5000, 3)])
    face = bn.sample(verts, faces, u)[0]
    assert set(face.tolist()) == {1, 3} and face[0] == 1 and face[1] == 3 and face[2] == 3 and face[3] == 1


def test_splitmix_rule():
    """The published splitmix64 sequence from state 0 is 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F: the rule's
    argument seed + golden * (iteration * K + k + 1) walks that sequence."""
    golden = 0x9E3779B97F4A7C15
    for fn in (bn.splitmix64, B.splitmix64):
        assert fn(golden) == 0xE220A8397B1DCDAF
        assert fn(2 * golden) == 0x6E789E6AA1B965F4
        assert fn(3 * golden) == 0x06C45D188009454F
    N = 1000003
    for fn in (bn.empty_point, B.empty_cluster_point):
        assert fn(0, 0, 0, 25, N) == 0xE220A8397B1DCDAF % N                  # (seed, iteration, k) = (0, 0, 0)
        assert fn(0, 0, 1, 25, N) == 0x6E789E6AA1B965F4 % N                  # (0, 0, 1)
        assert fn(0, 1, 0, 2, N) == 0x06C45D188009454F % N                   # (0, 1, 0) with K = 2: the third draw
        assert fn(golden, 0, 0, 25, N) == 0x6E789E6AA1B965F4 % N             # the seed shifts the walk
    assert bn.splitmix64(0x9E3779B97F4A7C15 * 7 + (1 << 64)) == bn.splitmix64(0x9E3779B97F4A7C15 * 7)   # mod 2^64


def test_new_entries_are_bound_and_declared():
    hdr = open(os.path.join(ROOT, "include", "moda_hip.h")).read()
    declared = set(re.findall(r"\b(moda_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_ENTRIES:
        assert name in _lib.EXPORTS and name in declared, name
    assert _lib.ABI_VERSION == 11 and _lib.load().moda_abi_version() == 11
    assert int(re.search(r"#define MODA_KMEANS_MAX_K (\d+)", hdr).group(1)) == B.MAX_K == 64
    assert int(re.search(r"#define MODA_MC_SCAN_TILE (\d+)", hdr).group(1)) == B._SCAN_TILE


def test_entries_refuse_bad_arguments_without_a_device():
    """Shape and pointer checks come before any launch, so they can be exercised without a GPU."""
    lib = _lib.load()
    EINVAL, ESHAPE = -1, -2
    assert lib.moda_kmeans_blocks(0) == 0 and lib.moda_kmeans_blocks(1) == 1 and lib.moda_kmeans_blocks(257) == 2
    assert lib.moda_kmeans_blocks(2 ** 31 - 1) == 1024
    null = [None] * 6
    assert lib.moda_kmeans_steps(None, 100, 0, *null, 1e-4, 0, 0, 1, None) == EINVAL
    assert lib.moda_kmeans_steps(None, 100, 65, *null, 1e-4, 0, 0, 1, None) == EINVAL
    assert lib.moda_kmeans_steps(None, 24, 25, *null, 1e-4, 0, 0, 1, None) == ESHAPE
    assert lib.moda_kmeans_steps(None, 100, 25, *null, 1e-4, 0, 0, 1, None) == EINVAL          # null pointers
    assert lib.moda_mesh_face_cdf(None, None, 3, 0, None, None, None, None, None, None) == ESHAPE
    assert lib.moda_mesh_face_cdf(None, None, 3, 1, None, None, None, None, None, None) == EINVAL
    assert lib.moda_mesh_sample(None, None, 3, 1, None, None, None, 5, None, None, None) == EINVAL
    assert lib.moda_mesh_sample(None, None, 3, 1, None, None, None, 0, None, None, None) == 0


def test_python_refusals_that_need_no_device():
    import torch
    X = torch.zeros(10, 3)
    with pytest.raises(NotImplementedError, match="distance"):
        B.kmeans(X, 2, distance="cosine")
    with pytest.raises(NotImplementedError, match="cluster_centers"):
        B.kmeans(X, 2, cluster_centers=torch.zeros(2, 3))
    with pytest.raises(ValueError):
        B.kmeans(torch.zeros(10, 2), 2)
    with pytest.raises(ValueError):
        B.kmeans(X, 11)
    with pytest.raises(ValueError):
        B.kmeans(torch.zeros(100, 3), 65)
    with pytest.raises(NotImplementedError, match="return_normals"):
        B.sample_points_from_meshes(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), 5, return_normals=True)
    with pytest.raises(NotImplementedError, match="grad"):
        B.sample_points_from_meshes(torch.zeros(3, 3, requires_grad=True), torch.zeros(1, 3, dtype=torch.int32), 5)
    with pytest.raises(ValueError, match="no faces"):
        B.sample_points_from_meshes(torch.zeros(3, 3), torch.zeros(0, 3, dtype=torch.int32), 5)


@pytest.mark.parametrize("N,seed,iterations", TRAJECTORIES)
def test_trajectory_margins(N, seed, iterations):
    """What lets the GPU test demand identical assignments: no point of any iteration is closer than 1e-5 (relative, squared
    distances) to changing its cluster -- one fp32 ulp in a centre moves such a ratio by about 4e-7 -- and no iteration's
    stopping test is close: shift^2 stays away from tol by more than 1e-3 of it."""
    X, init = trajectory_case(N, seed)
    res = bn.kmeans(X, init, tol=1e-4, iter_limit=100)
    print("N", N, "seed", seed, "iterations", res.iterations, "min margin", res.margin, "last shifts", res.shifts[-3:])
    assert res.iterations == iterations
    assert res.margin >= 1e-5
    assert all(abs(s * s / 1e-4 - 1) > 1e-3 for s in res.shifts)
    assert res.counts.min() > 0


def test_sampler_margins():
    """Every u0 * total of the GPU sampler tests lies further than 1e-9 * total from every CDF boundary, and the meshes' areas
    are exact in fp32, so the fp32 kernel's CDF agrees with the oracle's to float64 rounding and must pick the same face."""
    for name, (verts, faces) in sampler_meshes().items():
        exact = bn.face_areas(verts, faces)
        areas, cdf = bn.face_cdf(verts, faces)
        assert np.array_equal(areas.astype(np.float64), exact), name
        assert float(cdf[-1]) == float(np.sum(exact)), name                  # dyadic areas: the sum is exact in any order
        for S in (1000,) + ((200000,) if name == "two" else ()):
            gap = bn.sample(verts, faces, sampler_u(S))[3]
            print(name, "S", S, "min gap / total", gap.min())
            assert gap.min() > 1e-9, name
