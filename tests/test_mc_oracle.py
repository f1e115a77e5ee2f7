"""CPU: the oracle's two connected-part labellings (tests/mc_numpy.py) against each other, against the parts that
tests/topology_meshes.py states by construction and, where scipy is installed, against its connected_components.

`components` (vectorised min-propagation with pointer jumping) and `components_seq` (a sequential union-find with path
halving) share no step, and neither shares one with the kernels' concurrent hooks.  tests/test_gpu_mesh_topology.py takes
its expectations from them (up to about 300,000 vertices) and from the constructions (above that); this file is what
vouches for both.  Every comparison is exact: labels are integers."""
import time

import numpy as np
import pytest

import mc_numpy as mcn
import topology_meshes as tm


def both(nv, faces):
    t0 = time.perf_counter()
    a = mcn.components(nv, faces)
    t1 = time.perf_counter()
    b = mcn.components_seq(nv, faces)
    t2 = time.perf_counter()
    print(f"nv {nv} nf {len(faces)}: components {t1 - t0:.2f} s, components_seq {t2 - t1:.2f} s")
    assert a.shape == b.shape == (nv,) and np.array_equal(a, b)
    # a label is the lowest vertex of its part: a fixed point that no member undercuts
    assert np.array_equal(b[b], b) and (b <= np.arange(nv)).all()
    return b


def check_largest(nv, faces, keep):
    """largest_part with either labelling gives the constructed answer."""
    verts = np.arange(3 * nv, dtype=np.float64).reshape(nv, 3)
    for comp in (mcn.components, mcn.components_seq):
        kv, kf = mcn.largest_part(verts, faces, components=comp)
        assert np.array_equal(kv, verts[keep]) and np.array_equal(kf, tm.expected_faces(faces, keep))


@pytest.mark.parametrize("threshold", sorted(tm.RANDOM_VOLUME_PARTS))
def test_random_volume_parts(threshold):
    v, f = tm.random_volume_mesh(threshold)
    lab = both(len(v), f)
    roots, sizes = np.unique(lab, return_counts=True)
    assert (len(v), len(roots)) == tm.RANDOM_VOLUME_PARTS[threshold]
    top = np.sort(sizes)[::-1]
    if threshold == 0.1:
        assert len(f) == 777063 and (top[0], top[1]) == (356188, 78)
    if threshold == 1.5:
        assert top[0] == top[1] == top[2] == 34 and top[3] < 34            # the three-way tie
        kv, kf = mcn.largest_part(v, f, components=mcn.components_seq)
        first = roots[sizes == 34].min()
        assert len(kv) == 34 and np.array_equal(kv, v[lab == first])


@pytest.mark.parametrize("threshold", sorted(tm.RANDOM_VOLUME_PARTS))
def test_random_volume_part_count_against_scipy(threshold):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    v, f = tm.random_volume_mesh(threshold)
    roots = np.unique(mcn.components_seq(len(v), f))
    he = mcn.edges_of(f)
    n, _ = connected_components(sp.coo_matrix((np.ones(len(he)), (he[:, 0], he[:, 1])), shape=(len(v), len(v))), directed=False)
    assert n == len(roots)


@pytest.mark.parametrize("kind", ["natural", "reversed", "shuffled"])
def test_strip_of_20000_is_one_part(kind):
    nv, f, keep = tm.strip(20000, kind)
    assert (both(nv, f) == 0).all()
    check_largest(nv, f, keep)


@pytest.mark.parametrize("n_even,n_odd", [(500, 500), (501, 500), (500, 501)])
def test_two_interleaved_strips(n_even, n_odd):
    nv, f, keep = tm.two_strips(n_even, n_odd)
    lab = both(nv, f)
    ev, od = np.arange(0, 2 * n_even, 2), np.arange(1, 2 * n_odd, 2)
    assert (lab[ev] == 0).all() and (lab[od] == 1).all() and keep.sum() == max(n_even, n_odd)
    check_largest(nv, f, keep)


def test_unreferenced_vertices_and_no_faces():
    nv, f, keep = tm.scattered(100000)
    lab = both(nv, f)
    assert np.array_equal(lab[~keep], np.nonzero(~keep)[0]) and (lab[keep] == np.nonzero(keep)[0][0]).all()
    check_largest(nv, f, keep)
    for nv in (1, 5, 4097):
        none = np.zeros((0, 3), int)
        assert np.array_equal(both(nv, none), np.arange(nv))
        check_largest(nv, none, np.arange(nv) == 0)                        # every part has one vertex: the lowest is kept


def test_repeated_indices_and_hub_and_gaps():
    nv, f, keep = tm.degenerate_faces()
    lab = both(nv, f)
    assert keep.sum() == 204 and len(np.unique(lab)) == 3 and np.array_equal(lab == 162, keep)
    check_largest(nv, f, keep)
    nv, f, keep = tm.hub(20000)
    assert (both(nv, f) == 0).all()
    check_largest(nv, f, keep)
    for nv in (2047, 2048, 2049):
        nv, f, keep = tm.gapped_strip(nv)
        lab = both(nv, f)
        assert (lab[keep] == 1).all() and np.array_equal(lab[~keep], np.nonzero(~keep)[0])
        check_largest(nv, f, keep)
