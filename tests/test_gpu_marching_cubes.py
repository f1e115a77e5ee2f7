"""GPU (-m gpu): mesh extraction (moda_amd/mesh.py, csrc/mesh_kernels.hip) against the float64 oracle tests/mc_numpy.py.

What is pinned to the reference: the input volume (the G13 fixture and model of tests/test_gpu_mesh_queries.py), the vertex
set (one vertex per crossing lattice edge, which does not depend on the case table) and the index-to-world mapping of
train_utils.py:1442.  mcubes and trimesh are not available, so no golden mesh of the reference itself exists here: face
topology is checked against the oracle built on the generated table, and by closedness, orientation and Euler
characteristic.  Vertex bounds come from fp32 rounding: t correctly rounded in fp32 carries <= 3 ulp relative error, p + t
adds half an ulp at magnitude g, so lattice-index vertices are within 2 ulp_fp32(g); with the world affine,
2 ulp_fp32(g) |scale| + 2 ulp_fp32(max |out|) per coordinate.  (The kernel forms t and p + t in double and rounds once to
fp32, which stays inside these bounds.)"""
import ctypes
import types

import numpy as np
import pytest
import torch

import mc_numpy as mcn
from helpers import golden

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import moda_amd
    from moda_amd import mesh as M, mesh_queries as MQ, _lib
    from gpu_helpers import T, DEV


def ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def lattice_bound(shape):
    return 2 * ulp(max(shape))


def world_bound(shape, scale, out):
    return 2 * ulp(max(shape)) * np.abs(np.asarray(scale, np.float64)) + 2 * ulp(np.abs(out).max() if len(out) else 0.0)


def sdf(shape, f, offset=(0.137, 0.071, -0.053)):
    ax = [np.arange(n, dtype=np.float64) - (n - 1) / 2 + o for n, o in zip(shape, offset)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    return f(X, Y, Z).astype(np.float32)


def sphere(shape, r=None):
    r = r if r is not None else 0.35 * min(shape)
    return sdf(shape, lambda X, Y, Z: r - np.sqrt(X ** 2 + Y ** 2 + Z ** 2))


def field(kind, shape, seed=3):
    if kind == "random":
        return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    return sphere(shape)


def gpu_mc(vol, thr, vis=None):
    v, f = M.marching_cubes(T(vol), thr, None if vis is None else T(vis))
    return v.cpu().numpy().astype(np.float64), f.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 5, 4), (17, 17, 17), (64, 64, 64)])
@pytest.mark.parametrize("kind", ["random", "sphere"])
@pytest.mark.parametrize("with_vis", [False, True])
def test_matches_oracle(shape, kind, with_vis):
    vol = field(kind, shape)
    vis = np.random.default_rng(11).random(shape).astype(np.float32) * 0.6 + 0.1 if with_vis else None
    for thr in ([0.0, 0.4] if kind == "random" else [0.0]):
        v, f = gpu_mc(vol, thr, vis)
        rv, rf, _ = mcn.marching_cubes(vol, thr, vis)
        assert f.shape == rf.shape and np.array_equal(f, rf), (shape, kind, thr)
        assert v.shape == rv.shape
        if len(v):
            err = np.abs(v - rv).max()
            print(shape, kind, with_vis, thr, "V", len(v), "F", len(f), "max |dv|", err, "bound", lattice_bound(shape))
            assert err <= lattice_bound(shape), err


@pytest.mark.parametrize("shape", [(17, 17, 17), (64, 64, 64)])
@pytest.mark.parametrize("with_vis", [False, True])
@pytest.mark.parametrize("thr", [0.0, 1.0])
def test_integer_volume_exact_ties(shape, with_vis, thr):
    """Values in {-2, .., 2}: a fifth of the corners that `vis` leaves EQUAL the threshold.  Occupancy is the strict >, so such a corner is empty
    and a crossing edge that ends on it has t exactly 0 or 1: its vertex sits on the lattice point, where up to six edges
    put one each, and triangles between them have no area.  Faces are the oracle's exactly; vertices within lattice_bound."""
    vol = np.random.default_rng(21).integers(-2, 3, shape).astype(np.float32)
    vis = np.random.default_rng(11).random(shape).astype(np.float32) * 0.6 + 0.1 if with_vis else None
    rv, rf, _ = mcn.marching_cubes(vol, thr, vis)
    # conditions on the input, on the oracle alone
    assert (mcn.values(vol, vis) == thr).mean() > 0.05
    on_lattice = (rv == np.round(rv)).all(1)
    assert on_lattice.mean() > 0.05 and not on_lattice.all()
    assert len(np.unique(rv, axis=0)) < len(rv)                                 # coincident vertices
    tri = rv[rf]
    flat = (np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) == 0).all(1)
    assert flat.any() and not flat.all()                                        # triangles without area
    v, f = gpu_mc(vol, thr, vis)
    assert f.shape == rf.shape and np.array_equal(f, rf), (shape, with_vis, thr)
    assert v.shape == rv.shape
    err = np.abs(v - rv).max()
    print(shape, with_vis, thr, "V", len(v), "F", len(f), "on lattice", int(on_lattice.sum()), "flat", int(flat.sum()),
          "max |dv|", err, "bound", lattice_bound(shape))
    assert err <= lattice_bound(shape), err
    assert np.array_equal(v[on_lattice], rv[on_lattice])                        # t = 0 and t = 1 are exact in any precision


def test_world_affine_matches_oracle():
    shape, b = (33, 33, 33), np.asarray([0.31, 0.27, 0.45])
    vol = sphere(shape)
    scale, shift = 2 * b / shape[0], -b
    v, f, n_occ = M._run_mc(T(vol), 0.0, None, scale=scale, shift=shift)
    rv, rf, r_occ = mcn.marching_cubes(vol, 0.0, scale=scale, shift=shift)
    v = v.cpu().numpy().astype(np.float64)
    assert np.array_equal(f.cpu().numpy(), rf) and n_occ == r_occ
    assert (np.abs(v - rv) <= world_bound(shape, scale, rv)).all()


def _check_closed(faces):
    he = mcn.edges_of(faces)
    key = np.sort(he, 1)
    uniq, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    fwd = np.zeros(len(uniq), np.int64)
    np.add.at(fwd, inv.reshape(-1), (he[:, 0] < he[:, 1]).astype(np.int64))
    assert (cnt == 2).all() and (fwd == 1).all()


def test_sphere_256_closed_oriented():
    shape = (256, 256, 256)
    vol = sphere(shape, r=97.3)
    v, f = gpu_mc(vol, 0.0)
    # the vertex set is the set of crossing edges, in C order of (lower point, axis)
    pts = np.argwhere(mcn.crossing_edges(mcn.occupancy(vol, 0.0)))
    assert len(v) == len(pts) and len(pts) > 100000
    lower = pts[:, :3].astype(np.float64)
    on_axis = np.zeros_like(lower, bool)
    on_axis[np.arange(len(pts)), pts[:, 3]] = True
    assert np.array_equal(np.where(on_axis, 0.0, v), np.where(on_axis, 0.0, lower))
    d = v[on_axis] - lower[on_axis]
    assert (d >= 0).all() and (d <= 1).all()
    assert f.min() >= 0 and f.max() < len(v)
    _check_closed(f)
    assert mcn.euler_characteristic(len(v), f) == 2
    tri = v[f]
    vol6 = np.einsum("ij,ij->i", tri[:, 0], np.cross(tri[:, 1], tri[:, 2])).sum()
    assert vol6 > 0


def test_bit_identical_runs_and_degenerate_volumes():
    vol = field("random", (64, 64, 64), seed=5)
    a, b = M.marching_cubes(T(vol), 0.1), M.marching_cubes(T(vol), 0.1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    la, lb = M.largest_part(M.TriMesh(*a)), M.largest_part(M.TriMesh(*b))
    assert torch.equal(la.vertices_t, lb.vertices_t) and torch.equal(la.faces_t, lb.faces_t)
    for fill in (-1.0, 1.0):
        v, f = M.marching_cubes(torch.full((20, 21, 22), fill, device=DEV), 0.0)
        assert v.shape == (0, 3) and f.shape == (0, 3)
        assert len(M.largest_part(M.TriMesh(v, f)).vertices) == 0


def test_non_finite_values():
    vol = field("random", (17, 19, 18), seed=9)
    rng = np.random.default_rng(2)
    for val in (np.nan, np.inf, -np.inf):
        idx = rng.integers(0, vol.size, 300)
        vol.reshape(-1)[idx] = val
    v, f = gpu_mc(vol, 0.0)
    rv, rf, _ = mcn.marching_cubes(vol, 0.0)
    assert len(v) > 0 and np.isfinite(v).all() and f.min() >= 0 and f.max() < len(v)
    assert np.array_equal(f, rf) and np.abs(v - rv).max() <= lattice_bound(vol.shape)


def test_index_limit_refused_before_launch():
    big = torch.zeros(1, device=DEV).expand(1024, 1024, 683)     # 3 * g0 g1 g2 >= 2^31, nothing allocated
    with pytest.raises(ValueError, match="int32"):
        M.marching_cubes(big, 0.0)
    with pytest.raises(ValueError):
        M.marching_cubes(torch.zeros(1, 5, 5, device=DEV), 0.0)
    lib = _lib.load()
    assert lib.moda_mc_count(None, None, 1024, 1024, 683, 0.0, *([None] * 7), None) == -2
    assert lib.moda_mc_count(None, None, 1, 5, 5, 0.0, *([None] * 7), None) == -2


def test_largest_part_two_spheres():
    shape = (72, 64, 64)

    def two(X, Y, Z):
        return np.maximum(13.0 - np.sqrt((X + 15) ** 2 + Y ** 2 + Z ** 2), 7.5 - np.sqrt((X - 20) ** 2 + Y ** 2 + Z ** 2))
    vol = sdf(shape, two)
    v, f = M.marching_cubes(T(vol), 0.0)
    rv, rf, _ = mcn.marching_cubes(vol, 0.0)
    lab = mcn.components(len(rv), rf)
    sizes = sorted(np.bincount(lab)[np.unique(lab)])
    assert len(sizes) == 2 and 2.5 < sizes[1] / sizes[0] < 3.5, sizes
    part = M.largest_part(M.TriMesh(v, f))
    kv, kf = mcn.largest_part(rv, rf)
    pv, pf = part.vertices, part.faces
    assert np.array_equal(pf, kf) and pv.shape == kv.shape
    assert np.abs(pv - kv).max() <= lattice_bound(shape)
    assert pf.min() >= 0 and pf.max() == len(pv) - 1 and (pv[:, 0] < 36).all()


# ---- extract_mesh end to end on the G13 mock model ----------------------------------------------------------------
def _model(tmp_path, **opt_over):
    from test_gpu_mesh_queries import build_model
    model, models, emb = build_model()
    opts = dict(flowbw=False, lbs=False, neudbs=True, nerf_skin=True, nerf_dis=False, num_bones=25, queryfw=False,
                symm_shape=False, full_mesh=False, nerf_vis=True, use_cc=True, ce_color=True, checkpoint_dir=str(tmp_path),
                logname="log")
    opts.update(opt_over)
    (tmp_path / "log").mkdir(exist_ok=True)
    model.opts = types.SimpleNamespace(**opts)
    model.nerf_coarse, model.nerf_vis = models["coarse"], models["nerf_vis"]
    model.near_far = torch.zeros(1)
    model.latest_vars = {"obj_bound": np.asarray([0.2, 0.15, 0.25], np.float32), "idk": np.ones(4)}
    return model


def _expected(model, grid, thr, embedid=None):
    o = model.opts
    use_vis = not o.full_mesh and model.latest_vars["idk"].sum() > 0
    pw = None
    if embedid is not None and not o.queryfw:
        def pw(q):
            return MQ.warp_bw(o, model, {}, q, embedid)[0]
    vol, vis = MQ.query_volume(model.nerf_coarse, model.embedding_xyz, model.latest_vars["obj_bound"], grid,
                               nerf_vis=model.nerf_vis if use_vis else None, point_warp=pw, symm_shape=o.symm_shape,
                               precision="fp32")
    vol, vis = vol.cpu().numpy(), None if vis is None else vis.cpu().numpy()
    b = np.asarray(model.latest_vars["obj_bound"], np.float64)
    scale = 2 * b / grid
    v, f, _ = mcn.marching_cubes(vol, thr, vis, scale=scale, shift=-b)
    if o.use_cc and len(v):
        v, f = mcn.largest_part(v, f)
    return v, f, scale, vol


@pytest.mark.parametrize("over", [dict(), dict(use_cc=False), dict(full_mesh=True), dict(symm_shape=True),
                                  dict(embed=3)])
def test_extract_mesh_matches_oracle(tmp_path, over):
    over = dict(over)
    embedid = over.pop("embed", None)
    model = _model(tmp_path, **over)
    grid = 24
    _, _, _, vol = _expected(model, grid, 0.0, embedid)
    thr = float(np.median(vol))                                      # a mesh of about half the lattice
    ev, ef, scale, _ = _expected(model, grid, thr, embedid)
    out = M.extract_mesh(model, 1024, grid, threshold=thr, embedid=embedid)
    mesh = out["mesh"]
    assert len(ev) > 0 and np.array_equal(mesh.faces, ef)
    assert (np.abs(mesh.vertices - ev) <= world_bound((grid,) * 3, scale, ev)).all()
    assert mesh.vertices.dtype == np.float64 and mesh.faces.dtype == np.int64 and mesh.bounds.shape == (2, 3)
    c = mesh.visual.vertex_colors
    assert c.shape == (len(ev), 4) and c.dtype == np.uint8 and (c[:, 3] == 255).all()
    assert np.allclose(model.vis_min[0], mesh.vertices.min(0)) and "fraction occupied" in (tmp_path / "log" / "loss_log.txt").read_text()
    if embedid is not None:
        assert "bones" in out
    # queryfw: the rest mesh forward-warped to frame 3
    model.opts.queryfw = True
    fw = M.extract_mesh(model, 1024, grid, threshold=thr, embedid=3, mesh_dict_in={"mesh": mesh})["mesh"]
    want, _ = MQ.warp_fw(model.opts, model, {}, mesh.vertices, 3)
    assert np.array_equal(fw.vertices, want.astype(np.float64)) and np.array_equal(fw.faces, mesh.faces)
    assert np.array_equal(mesh.vertices, M.TriMesh(mesh.vertices_t, mesh.faces_t).vertices)   # the input mesh is untouched


def test_extract_mesh_refuses_unported_branches(tmp_path):
    model = _model(tmp_path, nerf_vis=False)
    with pytest.raises(NotImplementedError, match="nerf_vis"):
        M.extract_mesh(model, 1024, 16, threshold=0.0)
    model = _model(tmp_path, ce_color=False, full_mesh=True)
    _, _, _, vol = _expected(model, 16, 0.0)
    with pytest.raises(NotImplementedError, match="get_vertex_colors"):
        M.extract_mesh(model, 1024, 16, threshold=float(np.median(vol)))


def test_g13_fixture_volume(tmp_path, capsys):
    g = golden("g13_grid")["vol_sigma"].astype(np.float32)
    assert g.max() <= -0.002
    model = _model(tmp_path, full_mesh=True)
    out = M.extract_mesh(model, 1024, g.shape[0])                     # default threshold -0.002: the empty mesh
    assert len(out["mesh"].vertices) == 0 and len(out["mesh"].faces) == 0
    printed = capsys.readouterr().out
    assert "fraction occupied:" in printed and "tensor(0.," in printed, printed
    v, f = gpu_mc(g, -0.002)
    assert len(v) == 0 and len(f) == 0
    s = np.sort(g.reshape(-1))
    thr = float((s[107] + s[108]) / 2)                               # the median, which equals no fixture value
    assert np.float32(thr) not in s
    v, f = gpu_mc(g, thr)
    rv, rf, _ = mcn.marching_cubes(g, thr)
    assert len(v) > 0 and np.array_equal(f, rf) and np.abs(v - rv).max() <= lattice_bound(g.shape)


def test_extreme_finite_magnitudes():
    """Values near FLT_MAX: b - a overflows in fp32, the vertex still sits at the true fraction of its edge."""
    vol = np.clip(field("random", (9, 10, 11), seed=4), -1.1, 1.1) * np.float32(3e38)     # finite, |b - a| up to 6.6e38
    assert np.isfinite(vol).all()
    v, f = gpu_mc(vol, 0.0)
    rv, rf, _ = mcn.marching_cubes(vol, 0.0)
    assert len(v) > 0 and np.isfinite(v).all() and np.array_equal(f, rf)
    assert np.abs(v - rv).max() <= lattice_bound(vol.shape)


def test_largest_part_tie_keeps_lowest_vertex():
    """Two mirror-image spheres: equal vertex counts, so the part holding vertex 0 (the one at low x) is kept."""
    shape = (64, 40, 40)

    def two(X, Y, Z):
        return np.maximum(8.0 - np.sqrt((X + 14) ** 2 + Y ** 2 + Z ** 2), 8.0 - np.sqrt((X - 14) ** 2 + Y ** 2 + Z ** 2))
    vol = sdf(shape, two, offset=(0.0, 0.071, -0.053))               # exactly mirror-symmetric in x
    v, f = M.marching_cubes(T(vol), 0.0)
    rv, rf, _ = mcn.marching_cubes(vol, 0.0)
    lab = mcn.components(len(rv), rf)
    roots, sizes = np.unique(lab, return_counts=True)
    assert len(roots) == 2 and sizes[0] == sizes[1]
    part = M.largest_part(M.TriMesh(v, f))
    kv, kf = mcn.largest_part(rv, rf)
    assert np.array_equal(part.faces, kf) and np.abs(part.vertices - kv).max() <= lattice_bound(shape)
    assert len(kv) == sizes[0] and (kv[:, 0] < 32).all() and np.array_equal(kv[0], rv[0])


def test_largest_part_refuses_out_of_range_faces():
    verts = torch.zeros((4, 3), device=DEV)
    for bad in ([[0, 1, 4]], [[0, -1, 2]]):
        faces = torch.tensor([[0, 1, 2], [1, 2, 3]] + bad, dtype=torch.int32, device=DEV)
        with pytest.raises(ValueError, match="outside"):
            M.largest_part(M.TriMesh(verts, faces))
    ok = M.largest_part(M.TriMesh(verts, torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32, device=DEV)))
    assert len(ok.vertices) == 4 and len(ok.faces) == 2
