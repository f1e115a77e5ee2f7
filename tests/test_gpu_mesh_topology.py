"""GPU (-m gpu): moda_mesh_largest_part (moda_amd/mesh.py largest_part, csrc/mesh_kernels.hip) where the order of the
atomics, the depth of the union-find and the tiling of the scans decide the answer.

The inputs are built in numpy (tests/topology_meshes.py; the random-volume meshes by the numpy marching cubes), never by
the GPU marching cubes, so nothing of the extraction kernels can mask or fake a failure here.  The expected part comes
from the oracle's sequential union-find (mc_numpy.components_seq) up to 300,000 vertices, from its vectorised
`components` on the one random-volume mesh above that (tests/test_mc_oracle.py holds the two equal on these very meshes,
and their part counts to scipy's), and from the construction for the million-element meshes.

Every case asserts the same three things, all exact (the kernels only copy vertices and renumber faces, so there is
no tolerance anywhere in this file): faces array_equal to the expectation, vertices bit for bit input[keep], and two
runs torch.equal.  None of these meshes is meant to hang or fault: they are ordinary meshes with awkward numbering."""
import numpy as np
import pytest
import torch

import mc_numpy as mcn
import topology_meshes as tm

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from moda_amd import mesh as M
    from gpu_helpers import T, DEV

MILLION = 1000000


def vertex_values(nv, seed=1):
    """fp32 coordinates with every row distinct from its neighbours; a few special bit patterns ride along, since a copy
    must carry them unchanged."""
    v = np.random.default_rng(seed).standard_normal((nv, 3)).astype(np.float32)
    special = np.asarray([-0.0, np.inf, -np.inf, 1e-45, 3.4e38], np.float32)
    v.reshape(-1)[:min(len(special), v.size)] = special[:v.size]
    return v


def run(nv, faces, keep, name):
    """largest_part twice on the device; -> the kept vertex count.  faces (F,3) int64, keep (nv,) bool."""
    verts = vertex_values(nv)
    want_f = tm.expected_faces(faces, keep)
    tv = T(verts)
    tf = torch.as_tensor(np.ascontiguousarray(faces), dtype=torch.int32, device=DEV).reshape(-1, 3)
    a = M.largest_part(M.TriMesh(tv, tf))
    b = M.largest_part(M.TriMesh(tv, tf))
    assert torch.equal(tv, T(verts)) and torch.equal(tf.cpu(), torch.as_tensor(faces, dtype=torch.int32).reshape(-1, 3))
    got_v, got_f = a.vertices_t.cpu().numpy(), a.faces_t.cpu().numpy()
    print(f"{name}: nv {nv} nf {len(faces)} -> kept {len(got_v)} vertices, {len(got_f)} faces "
          f"(expected {int(keep.sum())}, {len(want_f)})")
    assert got_v.dtype == np.float32 and got_f.dtype == np.int32
    assert got_f.shape == want_f.shape and np.array_equal(got_f, want_f), name
    assert got_v.shape == (int(keep.sum()), 3) and np.array_equal(got_v.view(np.int32), verts[keep].view(np.int32)), name
    assert torch.equal(a.vertices_t, b.vertices_t) and torch.equal(a.faces_t, b.faces_t), name
    return len(got_v)


# ---- many parts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", sorted(tm.RANDOM_VOLUME_PARTS))
def test_many_parts_of_a_random_volume(threshold):
    v, f = tm.random_volume_mesh(threshold)
    nv = len(v)
    comp = mcn.components_seq if nv <= 300000 else mcn.components              # host time: the Python loop only where it is short
    lab = comp(nv, f)
    roots, sizes = np.unique(lab, return_counts=True)
    assert (nv, len(roots)) == tm.RANDOM_VOLUME_PARTS[threshold]              # a condition on the input
    top = np.sort(sizes)[::-1]
    if threshold == 1.5:
        assert top[0] == top[1] == top[2] == 34 and top[3] < 34                # three parts tie for the largest
    else:
        assert top[0] > top[1]
    best = roots[sizes == top[0]].min()                                        # among equals, the part with the lowest vertex
    keep = lab == best
    kv, kf = mcn.largest_part(v, f, components=comp)
    assert np.array_equal(kv, v[keep]) and np.array_equal(kf, tm.expected_faces(f, keep))
    assert run(nv, f, keep, f"random volume, threshold {threshold}") == top[0]
    # the same parts under another vertex numbering: the tie rule follows the numbers, not the geometry
    perm = np.random.default_rng(7).permutation(nv)
    lab_p = np.empty(nv, np.int64)
    lab_p[perm] = lab                                                           # vertex i is now called perm[i]
    low = np.full(nv, nv, np.int64)
    np.minimum.at(low, lab_p, np.arange(nv))                                   # lowest new name per old part
    cand = roots[sizes == top[0]]
    keep_p = lab_p == cand[np.argmin(low[cand])]
    assert run(nv, perm[f], keep_p, f"random volume, threshold {threshold}, vertices renamed") == top[0]


# ---- chains -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_seed", [None, 9])
@pytest.mark.parametrize("kind", ["natural", "reversed", "shuffled"])
def test_strip_of_a_million_is_kept_whole(kind, rows_seed):
    nv, f, keep = tm.strip(MILLION, kind, rows_seed)
    assert keep.all() and np.array_equal(tm.expected_faces(f, keep), f)        # expected: the input unchanged
    assert run(nv, f, keep, f"strip {kind}, rows {'shuffled' if rows_seed else 'in order'}") == nv


@pytest.mark.parametrize("n_even,n_odd", [(MILLION // 2, MILLION // 2), (MILLION // 2 + 1, MILLION // 2),
                                          (MILLION // 2, MILLION // 2 + 1)])
def test_two_interleaved_strips_keep_the_longer_or_vertex_zero(n_even, n_odd):
    nv, f, keep = tm.two_strips(n_even, n_odd)
    parity = 1 if n_odd > n_even else 0
    assert keep[parity] and np.array_equal(np.nonzero(keep)[0], np.arange(parity, 2 * max(n_even, n_odd), 2))
    assert run(nv, f, keep, f"two strips {n_even} + {n_odd}") == max(n_even, n_odd)


# ---- contention ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_seed", [None, 4])
def test_hub_is_one_part(rows_seed):
    nv, f, keep = tm.hub(MILLION)
    if rows_seed is not None:
        f = tm.shuffle_rows(f, rows_seed)
    assert run(nv, f, keep, "hub") == nv


# ---- vertices that no face references, faces that repeat an index ---------------------------------------------------
def test_unreferenced_vertices():
    nv, f, keep = tm.scattered(100000)
    assert keep.sum() == 162
    assert run(nv, f, keep, "icosphere among unused vertices") == 162


@pytest.mark.parametrize("nv", [1, 5, 4097])
def test_no_faces_keeps_vertex_zero(nv):
    none = np.zeros((0, 3), int)
    assert np.array_equal(mcn.components_seq(nv, none), np.arange(nv))
    kv, kf = mcn.largest_part(np.arange(3.0 * nv).reshape(nv, 3), none, components=mcn.components_seq)
    assert len(kv) == 1 and kv[0, 0] == 0 and kf.shape == (0, 3)
    assert run(nv, none, np.arange(nv) == 0, f"no faces, nv {nv}") == 1


def test_faces_with_repeated_indices():
    nv, f, keep = tm.degenerate_faces()
    lab = mcn.components_seq(nv, f)
    assert np.array_equal(lab == 162, keep) and keep.sum() == 204
    assert ((f[:, 0] == f[:, 1]) & (f[:, 1] != f[:, 2])).sum() == 2 and ((f[:, 0] == f[:, 1]) & (f[:, 1] == f[:, 2])).sum() == 4
    assert run(nv, f, keep, "repeated indices") == 204


# ---- sizes that straddle the scan tile (2048) and the tile-sum scan's chunk (1024 tiles) ---------------------------
@pytest.mark.parametrize("nv", [2047, 2048, 2049, 2097151, 2097153])
def test_gapped_strip_across_scan_tiles(nv):
    nv, f, keep = tm.gapped_strip(nv)
    if nv > 2097152:
        assert len(f) > 2097152                                                # the second chunk for the faces too
    assert run(nv, f, keep, "gapped strip") == nv - (nv + 2) // 3
