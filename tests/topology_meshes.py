"""Meshes whose connected parts are known without running a union-find, built in numpy: the inputs of
tests/test_gpu_mesh_topology.py (the kernels' largest_part) and tests/test_mc_oracle.py (the oracle's two labellings).

Each builder returns (nv, faces (F,3) int64, keep (nv,) bool): `keep` marks the part that largest_part must keep (the
part with the most vertices; among equals the one holding the lowest vertex), stated BY CONSTRUCTION.  `expected_faces`
turns it into the face list that must come out: the rows whose first index is kept, in their order, renumbered by the
running count of kept vertices."""
import numpy as np

import mc_numpy as mcn
import raster_numpy as rn

RANDOM_VOLUME = dict(shape=(64, 64, 64), seed=5)
# threshold -> (vertices, parts) of the numpy marching cubes on that volume; 1.5 has a three-way tie for the largest
# part at 34 vertices.  Conditions on the input, asserted by the tests that use it: if a numpy change moves them, the
# seed is to be replaced, not the figures
RANDOM_VOLUME_PARTS = {0.1: (384814, 3986), 1.0: (207171, 22724), 1.5: (97212, 14187), 2.0: (34180, 5535)}
_cache = {}


def random_volume_mesh(threshold):
    """-> (vertices (V,3) float64, faces (F,3) int64) of the numpy marching cubes on the seeded Gaussian volume."""
    if threshold not in _cache:
        vol = np.random.default_rng(RANDOM_VOLUME["seed"]).standard_normal(RANDOM_VOLUME["shape"]).astype(np.float32)
        v, f, _ = mcn.marching_cubes(vol, threshold)
        _cache[threshold] = (v, f)
    return _cache[threshold]


def expected_faces(faces, keep):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    new = np.cumsum(keep) - 1
    rows = keep[faces[:, 0]]
    assert (keep[faces[rows]]).all() and not keep[faces[~rows]].any(), "a face straddles the kept part: the builder is wrong"
    return new[faces[rows]]


def strip_faces(n):
    """The triangle strip (i, i+1, i+2) over n >= 3 vertices: one part, a chain as long as the mesh."""
    i = np.arange(n - 2, dtype=np.int64)
    return np.stack([i, i + 1, i + 2], 1)


def labelling(n, kind, seed=0):
    if kind == "natural":
        return np.arange(n, dtype=np.int64)
    if kind == "reversed":
        return np.arange(n - 1, -1, -1, dtype=np.int64)
    assert kind == "shuffled"
    return np.random.default_rng(seed).permutation(n).astype(np.int64)


def shuffle_rows(faces, seed):
    return faces[np.random.default_rng(seed).permutation(len(faces))]


def strip(n, kind, rows_seed=None):
    """One strip through all n vertices, its vertices renamed by `labelling`; rows shuffled when rows_seed is given."""
    f = labelling(n, kind, seed=n % 1000 + 1)[strip_faces(n)]
    if rows_seed is not None:
        f = shuffle_rows(f, rows_seed)
    return n, f, np.ones(n, bool)


def two_strips(n_even, n_odd, rows_seed=None):
    """A strip through the even vertices 0, 2, .. (n_even of them) and one through the odd vertices 1, 3, .. (n_odd),
    |n_even - n_odd| <= 1; nv = 2 max(n_even, n_odd) (- 1 when the even strip is the longer), so when the odd strip is
    the longer the last even vertex is in no face.  The longer strip is kept; equal lengths: the even one (vertex 0)."""
    assert abs(n_even - n_odd) <= 1 and min(n_even, n_odd) >= 3
    nv = max(2 * n_even - 1, 2 * n_odd)
    f = np.concatenate([2 * strip_faces(n_even), 2 * strip_faces(n_odd) + 1])
    f = shuffle_rows(f, 17 if rows_seed is None else rows_seed)          # the two strips' rows always interleave
    parity = np.arange(nv) % 2
    keep = (parity == 1) if n_odd > n_even else (parity == 0) & (np.arange(nv) < 2 * n_even)
    return nv, f, keep


def hub(nf):
    """nf faces (i, i+1, nv-1): every face's second hook meets the others at the highest vertex.  One part."""
    nv = nf + 2
    i = np.arange(nf, dtype=np.int64)
    return nv, np.stack([i, i + 1, np.full(nf, nv - 1, np.int64)], 1), np.ones(nv, bool)


def scattered(n_unused, seed=3):
    """An icosphere (162 vertices, 320 faces, one part) whose vertices sit at sorted random places among n_unused
    vertices that no face references."""
    v, f = rn.icosphere(2)
    nv = len(v) + n_unused
    pos = np.sort(np.random.default_rng(seed).choice(nv, len(v), replace=False))
    keep = np.zeros(nv, bool)
    keep[pos] = True
    return nv, pos[f], keep


def gapped_strip(nv, rows_seed=5):
    """The kept part: a strip, in both windings, through the vertices with index % 3 != 0.  Every other vertex is alone in
    its part and carries one face (a, a, a), which must be dropped.  Rows shuffled, so kept and dropped faces alternate
    irregularly: the new vertex and face numbers have gaps across every scan-tile boundary."""
    idx = np.nonzero(np.arange(nv) % 3 != 0)[0]
    s = idx[strip_faces(len(idx))]
    lone = np.nonzero(np.arange(nv) % 3 == 0)[0]
    f = np.concatenate([s, s[:, ::-1], np.stack([lone, lone, lone], 1)])
    keep = np.zeros(nv, bool)
    keep[idx] = True
    return nv, shuffle_rows(f, rows_seed), keep


def degenerate_faces():
    """Icospheres P (162 vertices), Q (162) and R (42), then one vertex L that only a face (L, L, L) names.  Q and R are
    joined by nothing but a face (q, q, r), so the kept part is Q + R (204 vertices) only if that face's one real edge
    is hooked; P and Q hold more faces with a repeated index, which change nothing.  Rows shuffled."""
    (vp, fp), (vr, fr) = rn.icosphere(2), rn.icosphere(1)
    nP, nR = len(vp), len(vr)
    q0, r0, lone = nP, 2 * nP, 2 * nP + nR
    nv = lone + 1
    extra = np.asarray([[q0 + 5, q0 + 5, r0 + 7],                          # the bridge
                        [3, 3, 90], [40, 40, 40], [q0 + 9, q0 + 9, q0 + 9], [q0 + 11, q0 + 100, q0 + 100],
                        [r0 + 1, r0 + 1, r0 + 1], [lone, lone, lone]], np.int64)
    f = shuffle_rows(np.concatenate([fp, fp + q0, fr + r0, extra]), 23)
    keep = np.zeros(nv, bool)
    keep[q0:lone] = True
    return nv, f, keep
