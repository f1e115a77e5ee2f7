"""Float64 numpy restatement of marching cubes as moda_amd/csrc/mesh_kernels.hip specifies it (the test oracle).

It shares only the generated case table (moda_amd/mc_table.py) with the kernels: vertex numbering comes from a cumulative
sum over a dense (g0, g1, g2, 3) edge array and faces from a per-slot gather, not from the kernels' scans and per-point
offsets.  Conventions: a corner is occupied iff its value is finite and > threshold (with `vis`: the value is -1 where
vis < 0.5); one vertex per crossing lattice edge, numbered in C order of the edge's lower point, then axis; faces by cell
in C order, then in table order; a vertex sits at t = (thr - v_a) / (v_b - v_a) along its edge, or at the finite end
when the other end is not finite."""
import numpy as np

from moda_amd import mc_table

_NTRI, _TRIS = mc_table.generate()
_EDGE_AXIS = np.asarray([e[0] for e in mc_table.EDGES])
_EDGE_OFF = np.asarray([e[1] for e in mc_table.EDGES])


def values(vol, vis=None):
    v = np.asarray(vol, np.float32)
    if vis is not None:
        v = np.where(np.asarray(vis, np.float32) < 0.5, np.float32(-1), v)
    return v


def occupancy(vol, threshold, vis=None):
    v = values(vol, vis).astype(np.float64)
    thr = np.float64(np.float32(threshold))
    return np.isfinite(v) & (v > thr)


def crossing_edges(occ):
    """(g0, g1, g2, 3) bool: the +axis edge from each lattice point crosses the surface."""
    cross = np.zeros(occ.shape + (3,), bool)
    cross[:-1, :, :, 0] = occ[:-1] != occ[1:]
    cross[:, :-1, :, 1] = occ[:, :-1] != occ[:, 1:]
    cross[:, :, :-1, 2] = occ[:, :, :-1] != occ[:, :, 1:]
    return cross


def marching_cubes(vol, threshold, vis=None, scale=(1.0, 1.0, 1.0), shift=(0.0, 0.0, 0.0)):
    """-> (vertices (V,3) float64, faces (F,3) int64, occupied count)."""
    v = values(vol, vis).astype(np.float64)
    thr = np.float64(np.float32(threshold))
    occ = np.isfinite(v) & (v > thr)
    g = np.asarray(occ.shape)
    cross = crossing_edges(occ)
    eid = np.full(cross.shape, -1, np.int64)
    eid[cross] = np.arange(int(cross.sum()))                        # C order over (i, j, k, axis)
    pts = np.argwhere(cross)                                        # same order
    verts = pts[:, :3].astype(np.float64)
    if len(pts):
        a = v[pts[:, 0], pts[:, 1], pts[:, 2]]
        nb = pts[:, :3].copy()
        nb[np.arange(len(pts)), pts[:, 3]] += 1
        b = v[nb[:, 0], nb[:, 1], nb[:, 2]]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            t = (thr - a) / (b - a)
        t = np.where(~np.isfinite(a), 1.0, np.where(~np.isfinite(b), 0.0, t))
        verts[np.arange(len(pts)), pts[:, 3]] += t
    verts = verts * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    # cells: case index from the 8 corners, C order over (g0-1, g1-1, g2-1)
    o = occ.astype(np.int64)
    case = np.zeros(tuple(g - 1), np.int64)
    for c, (dx, dy, dz) in enumerate(mc_table.CORNERS):
        case |= o[dx:dx + g[0] - 1, dy:dy + g[1] - 1, dz:dz + g[2] - 1] << c
    case = case.reshape(-1)
    ntri = _NTRI[case]
    start = np.concatenate([[0], np.cumsum(ntri)[:-1]])
    faces = np.zeros((int(ntri.sum()), 3), np.int64)
    for s in range(_TRIS.shape[1]):
        sel = np.nonzero(ntri > s)[0]
        for k in range(3):
            e = _TRIS[case[sel], s, k]
            p = np.stack(np.unravel_index(sel, tuple(g - 1)), 1) + _EDGE_OFF[e]
            faces[start[sel] + s, k] = eid[p[:, 0], p[:, 1], p[:, 2], _EDGE_AXIS[e]]
    assert (faces >= 0).all()
    return verts, faces, int(occ.sum())


def edges_of(faces):
    """Directed half-edges (3F, 2)."""
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def euler_characteristic(nv, faces):
    he = edges_of(faces)
    und = np.unique(np.sort(he, 1), axis=0)
    return nv - len(und) + len(faces)


def components(nv, faces):
    """Vertex labels: the lowest vertex index of each face-connected part (numpy union-find by repeated min-propagation)."""
    lab = np.arange(nv)
    he = edges_of(faces)
    while True:
        m = np.minimum(lab[he[:, 0]], lab[he[:, 1]])
        new = lab.copy()
        np.minimum.at(new, he[:, 0], m)
        np.minimum.at(new, he[:, 1], m)
        new = new[new]                                              # pointer jumping
        if np.array_equal(new, lab):
            return lab
        lab = new


def components_seq(nv, faces):
    """The same labels by a sequential union-find: one Python loop over the edges (f0, f1), (f1, f2) of each face, finds with
    path halving, the larger root hooked under the smaller, so a root is the lowest vertex of its part.  Neither the
    kernels' concurrent hooks nor `components`' min-propagation: its time does not depend on how the vertices are numbered
    (about 1 s per 300,000 faces), which `components`' does (a chain with shuffled labels takes it O(nv) sweeps)."""
    parent = list(range(nv))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    for a, b in np.concatenate([f[:, [0, 1]], f[:, [1, 2]]]).tolist():
        ra, rb = find(a), find(b)
        if ra < rb:
            parent[rb] = ra
        elif rb < ra:
            parent[ra] = rb
    return np.asarray([find(x) for x in range(nv)], np.int64).reshape(nv)


def largest_part(verts, faces, components=components):
    """Keep the part with the most vertices (ties: the part holding the lowest vertex index), order kept, faces remapped.
    `components`: the labelling to use, `components` or `components_seq`."""
    nv = len(verts)
    if nv == 0:
        return verts, faces
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    lab = components(nv, faces)
    cnt = np.bincount(lab, minlength=nv)
    best = int(np.argmax(cnt))                                      # first maximum = lowest label = lowest vertex index
    keep = lab == best
    new = np.cumsum(keep) - 1
    fk = keep[np.asarray(faces)[:, 0]]
    return verts[keep], new[np.asarray(faces)[fk]]
