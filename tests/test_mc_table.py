"""CPU: the generated marching-cubes table (moda_amd/mc_table.py) and the float64 oracle built on it (tests/mc_numpy.py).

The committed table in mesh_kernels.hip must be the generator's output, each case must use exactly its crossing edges,
and the meshes it gives must be closed and consistently oriented away from the lattice border, with the Euler
characteristic of a sphere (2) and of a torus (0).  PyMCubes / trimesh are not available to compare against, so the
table's ambiguity rule is checked by these properties, not against PyMCubes' own table."""
import os
import re

import numpy as np
import pytest

import mc_numpy as mcn
from moda_amd import mc_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_table_is_the_generator_output():
    src = open(os.path.join(ROOT, "moda_amd", "csrc", "mesh_kernels.hip")).read()
    m = re.search(re.escape(mc_table.BEGIN) + r".*?" + re.escape(mc_table.END) + r"\n", src, re.S)
    assert m is not None, "marker comments not found in mesh_kernels.hip"
    assert m.group(0) == mc_table.table_text()


def test_every_case_uses_exactly_its_crossing_edges():
    ntri, tris = mc_table.generate()
    assert ntri[0] == 0 and ntri[255] == 0
    for case in range(256):
        occ = [(case >> c) & 1 for c in range(8)]
        cross = {e for e, (_, _, c0, c1) in enumerate(mc_table.EDGES) if occ[c0] != occ[c1]}
        used = set(tris[case, :ntri[case]].reshape(-1).tolist())
        assert used == cross, case
        assert (tris[case, ntri[case]:] == -1).all()
        for t in tris[case, :ntri[case]]:
            assert len(set(t.tolist())) == 3, case


def _check_closed_oriented(vol, thr, verts_faces=None):
    """Every mesh edge away from the lattice border is used by exactly two faces, in opposite directions; edges used
    otherwise lie in a border plane of the lattice (both their vertices sit on lattice edges inside that plane)."""
    verts, faces, _ = verts_faces if verts_faces is not None else mcn.marching_cubes(vol, thr)
    occ = mcn.occupancy(vol, thr)
    pts = np.argwhere(mcn.crossing_edges(occ))                     # vertex -> (i, j, k, axis) of its edge
    g = np.asarray(occ.shape)
    he = mcn.edges_of(faces)
    key = np.sort(he, 1)
    uniq, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    fwd = np.zeros(len(uniq), np.int64)
    np.add.at(fwd, inv, (he[:, 0] < he[:, 1]).astype(np.int64))
    good = (cnt == 2) & (fwd == 1)
    bad = uniq[~good]
    for a, b in bad:
        on_plane = False
        for ax in range(3):
            for side in (0, g[ax] - 1):
                pa, pb = pts[a], pts[b]
                if pa[3] != ax and pb[3] != ax and pa[ax] == side and pb[ax] == side:
                    on_plane = True
        assert on_plane, (a, b, pts[a], pts[b])
    assert (cnt <= 2).all()
    return len(bad)


@pytest.mark.parametrize("thr", [-0.5, 0.0, 0.3, 0.8])
def test_random_fields_give_closed_oriented_meshes(thr):
    rng = np.random.default_rng(7)
    vol = rng.standard_normal((9, 11, 13)).astype(np.float32)
    verts, faces, n_occ = mcn.marching_cubes(vol, thr)
    assert len(faces) > 50 and n_occ == int((vol > np.float32(thr)).sum())
    _check_closed_oriented(vol, thr, (verts, faces, n_occ))


def _sdf_grid(n, f):
    x = np.arange(n, dtype=np.float64) - (n - 1) / 2 + 0.137
    X, Y, Z = np.meshgrid(x, x + 0.071, x - 0.053, indexing="ij")
    return f(X, Y, Z).astype(np.float32)


def _signed_volume(verts, faces):
    v = verts[faces]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6)


def test_sphere_and_torus_euler_characteristic():
    sphere = _sdf_grid(48, lambda X, Y, Z: 17.0 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2))
    v, f, _ = mcn.marching_cubes(sphere, 0.0)
    assert _check_closed_oriented(sphere, 0.0, (v, f, 0)) == 0
    assert mcn.euler_characteristic(len(v), f) == 2
    assert _signed_volume(v, f) > 0                                  # normals point from occupied to empty
    torus = _sdf_grid(48, lambda X, Y, Z: 6.0 - np.sqrt((np.sqrt(X ** 2 + Y ** 2) - 14.0) ** 2 + Z ** 2))
    v, f, _ = mcn.marching_cubes(torus, 0.0)
    assert _check_closed_oriented(torus, 0.0, (v, f, 0)) == 0
    assert mcn.euler_characteristic(len(v), f) == 0
    assert _signed_volume(v, f) > 0


def test_oracle_largest_part_keeps_the_bigger_sphere():
    def two(X, Y, Z):
        return np.maximum(9.0 - np.sqrt((X + 10) ** 2 + Y ** 2 + Z ** 2), 4.5 - np.sqrt((X - 12) ** 2 + Y ** 2 + Z ** 2))
    vol = _sdf_grid(40, two)
    v, f, _ = mcn.marching_cubes(vol, 0.0)
    lab = mcn.components(len(v), f)
    assert len(np.unique(lab)) == 2
    kv, kf = mcn.largest_part(v, f)
    assert (kv[:, 0] < 20).all() and len(kv) > len(v) / 2
    assert kf.max() == len(kv) - 1 and mcn.euler_characteristic(len(kv), kf) == 2
