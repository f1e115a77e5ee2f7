"""Float64 numpy oracle for moda_amd/bones.py (not a test): Lloyd's k-means as moda_amd.kmeans' docstring states it, with the
empty-cluster rule restated, and the surface sampler (face areas, inclusive CDF, the draw).  Inputs are fp32 values widened to
float64, so the oracle sees exactly the numbers the kernels see."""
from collections import namedtuple

import numpy as np

from pointset_numpy import dist2_matrix

KMeans = namedtuple("KMeans", "assign centers iterations margin shifts counts")
_M = (1 << 64) - 1


def splitmix64(z):
    z &= _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


def empty_point(seed, iteration, k, K, N):
    """Index of the point that refills cluster k when it is empty, `iteration` = iterations finished before this one."""
    return splitmix64(seed + 0x9E3779B97F4A7C15 * (iteration * K + k + 1)) % N


def assign_step(X, C):
    """-> nearest centre per point (lowest index among equal distances), and second_nearest_d / nearest_d - 1 per point
    (inf where K == 1 or the nearest distance is 0 with a positive runner-up; 0 where both are 0)."""
    D = dist2_matrix(X, C)
    a = D.argmin(1)
    r = np.arange(len(a))
    d1 = D[r, a].copy()
    if D.shape[1] == 1:
        return a, np.full(len(a), np.inf)
    D[r, a] = np.inf
    d2 = D.min(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.where(d2 > d1, d2 / d1 - 1.0, 0.0)
    return a, m


def update_step(X, a, C_old, seed, iteration):
    """Float64 means over the assignment, rounded to fp32 once; empty clusters by the rule.  -> centres fp32, counts, shift."""
    K, N = len(C_old), len(X)
    X64 = np.asarray(X, np.float64)
    counts = np.bincount(a, minlength=K)
    C = np.empty((K, 3), np.float32)
    for k in range(K):
        if counts[k]:
            C[k] = (X64[a == k].sum(0) / counts[k]).astype(np.float32)
        else:
            C[k] = X[empty_point(seed, iteration, k, K, N)]
    d = C.astype(np.float64) - np.asarray(C_old, np.float64)
    shift = float(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).sum())
    return C, counts, shift


def kmeans(X, init, tol=1e-4, iter_limit=0, seed=0):
    """X (N,3) fp32, init (K,) indices -> KMeans(assign, centers fp32 -- rounded each iteration --, iterations, margin = the
    minimum over all iterations and points of second_nearest_d / nearest_d - 1, the shift of every iteration, last counts)."""
    X = np.asarray(X, np.float32)
    C = X[np.asarray(init)].copy()
    it, margin, shifts = 0, np.inf, []
    while True:
        a, m = assign_step(X, C)
        margin = min(margin, float(m.min()))
        C, counts, shift = update_step(X, a, C, seed, it)
        shifts.append(shift)
        it += 1
        if shift * shift < tol or (iter_limit != 0 and it >= iter_limit):
            return KMeans(a, C, it, margin, shifts, counts)


def face_areas(verts, faces):
    v = np.asarray(verts, np.float64)
    a, b, c = (v[np.asarray(faces)[:, i]] for i in range(3))
    return 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)


def face_cdf(verts, faces):
    """-> areas (float64 arithmetic, rounded to fp32 as the kernel stores them), inclusive CDF float64 of those."""
    areas = face_areas(verts, faces).astype(np.float32)
    return areas, np.cumsum(areas.astype(np.float64))


def sample(verts, faces, u):
    """u (S,3) fp32 in [0,1) -> face (S,) (the first i with cdf[i] > u0 * cdf[-1]), points (S,3) float64, the barycentrics
    (S,3) float64 and the distance of every u0 * total to the nearest CDF boundary, as a fraction of the total."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces)
    u = np.asarray(u, np.float32).astype(np.float64)
    _, cdf = face_cdf(verts, faces)
    t = u[:, 0] * cdf[-1]
    face = np.minimum(np.searchsorted(cdf, t, side="right"), len(cdf) - 1)
    bounds = np.concatenate([[0.0], cdf[:-1]])                       # boundaries a target can cross; u0 < 1 keeps it off cdf[-1]
    gap = np.abs(t[:, None] - bounds[None, :]).min(1) / cdf[-1] if len(t) * len(bounds) <= 2e7 else None
    s = np.sqrt(u[:, 1])
    w = np.stack([1 - s, s * (1 - u[:, 2]), s * u[:, 2]], 1)
    pts = (w[:, :, None] * v[f[face]]).sum(1)
    return face, pts, w, gap


def strip_mesh(n_faces, seed):
    """A planar triangle strip whose areas are exact in fp32: vertices (x_i, 0 or 1, 0) with x steps from {1, 2, 3} / 4, so
    every cross product is a small dyadic number and its norm an exact square root."""
    rng = np.random.default_rng(seed)
    n = n_faces + 2
    x = np.cumsum(rng.integers(1, 4, n)) / 4.0
    verts = np.stack([x, (np.arange(n) % 2).astype(np.float64), np.zeros(n)], 1).astype(np.float32)
    faces = np.stack([np.arange(n_faces), np.arange(n_faces) + 1, np.arange(n_faces) + 2], 1).astype(np.int32)
    return verts, faces
