"""GPU (-m gpu): the camera tools (moda_amd/cams.py, csrc/cams_kernels.hip) against the float64 restatement tests/cams_numpy.py,
itself pinned to the reference by tests/test_cams_oracle.py where the reference can be run."""
import importlib
import os

import numpy as np
import pytest
import torch

import cams_numpy as cn
from test_cams_oracle import G, HULL, fill_patterns, hull

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import moda_amd
    from gpu_helpers import DEV
    CM = importlib.import_module("moda_amd.cams")


def np_(t):
    return t.detach().cpu().numpy()


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def rotations(rng, n, max_deg=None):
    q, r = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.linalg.det(q)[:, None]
    if max_deg is None:
        return q
    ax = rng.standard_normal((n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = np.deg2rad(rng.uniform(0, max_deg, n))
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    return np.eye(3)[None] + np.sin(ang)[:, None, None] * K + (1 - np.cos(ang))[:, None, None] * np.matmul(K, K)


def cams(R, t, krow=(0, 0, 0, 1)):
    out = np.tile(np.eye(4), (len(R), 1, 1))
    out[:, :3, :3], out[:, :3, 3], out[:, 3] = R, t, krow
    return out.astype(np.float32)


# ---- fill_invalid_rotations / save_cams ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [p[0] for p in fill_patterns()])
def test_fill_and_save_cams_are_exact(pattern):
    """Rotations and src are copies, the scaled translations one fp32 product: everything bit for bit, the table's duplicated
    last rows included, its translation and K row untouched."""
    _, valid, off = next(p for p in fill_patterns() if p[0] == pattern)
    nv, N = len(off) - 1, int(off[-1])
    rng = np.random.default_rng(11)
    rtk = rng.standard_normal((N, 4, 4)).astype(np.float32)
    got, src = CM.fill_invalid_rotations(dev(rtk), dev(valid), off)
    want, want_src = cn.fill_invalid_rotations(rtk, valid, off)
    assert np.array_equal(np_(src), want_src) and np.array_equal(bits(np_(got)), bits(want))
    data_offset = [int(o) + v for v, o in enumerate(off)]
    M = data_offset[-1]
    for unc_filter in (True, False):
        state = moda_amd.FrameState(M, DEV)
        tab_rtk, tab_raw = rng.standard_normal((M, 4, 4)).astype(np.float32), rng.standard_normal((M, 3, 4)).astype(np.float32)
        state.rtk.copy_(dev(tab_rtk))
        state.rt_raw.copy_(dev(tab_raw))
        init = CM.save_cams(dev(rtk), dev(valid), data_offset, 0.37, state, unc_filter=unc_filter)
        w_rtk, w_src, w_nv, w_rows, w_tab, w_raw = cn.save_cams(rtk, valid, data_offset, 0.37, tab_rtk, tab_raw, unc_filter)
        assert np.array_equal(bits(np_(init.rtk)), bits(w_rtk)) and np.array_equal(np_(init.src), w_src)
        assert np.array_equal(np_(init.n_valid), w_nv) and np.array_equal(np_(init.rows), w_rows)
        assert np.array_equal(bits(np_(state.rtk)), bits(w_tab)) and np.array_equal(bits(np_(state.rt_raw)), bits(w_raw))
        assert np.array_equal(bits(np_(state.rtk)[:, :3, 3]), bits(tab_rtk[:, :3, 3])) and np.array_equal(bits(np_(state.rtk)[:, 3]), bits(tab_rtk[:, 3]))
        last = np.asarray(data_offset[1:]) - 1
        assert np.array_equal(bits(np_(state.rt_raw)[last]), bits(np_(state.rt_raw)[last - 1]))
        if not unc_filter:
            assert np.array_equal(np_(init.src), np.arange(N))


def test_save_round_trips_through_load_root(tmp_path):
    rng = np.random.default_rng(5)
    rtk = cams(rotations(rng, 7), rng.standard_normal((7, 3)), (10, 10, 5, 5))
    valid = np.asarray([1, 0, 1, 1, 0, 0, 1], bool)
    state = moda_amd.FrameState(9, DEV)
    init = CM.save_cams(dev(rtk), dev(valid), [0, 5, 9], 2.0, state)
    paths = init.save(str(tmp_path), ["a", "b"])
    assert len(paths) == 9 and os.path.basename(paths[4]) == "a-00004.txt"
    back = CM.load_root('%s/a-' % tmp_path, 0)
    want = np_(init.rtk).astype(np.float64)
    assert np.array_equal(back[:4], want[:4]) and np.array_equal(back[4], want[3])
    assert np.array_equal(CM.load_root('%s/b-' % tmp_path, 0)[:3], want[4:])


# ---- align_sim3 ---------------------------------------------------------------------------------------------------------------
def sim3_inputs(n, kind, seed=0, max_deg=8.0):
    rng = np.random.default_rng(1000 * n + seed)
    Ra, delta, noise = rotations(rng, n), rotations(rng, 1)[0], rotations(rng, n, max_deg)
    a = cams(Ra, rng.standard_normal((n, 3)) + [0, 0, 3])
    b = cams(np.matmul(np.matmul(Ra, noise), delta.T), 0.4 * (rng.standard_normal((n, 3)) + [0, 0, 3]), (3, 4, 5, 6))
    err = rng.uniform(0.1, 1.0, n).astype(np.float32)
    inl = {"none": None, "all": np.ones(n, bool), "allfalse": np.zeros(n, bool), "some": rng.uniform(size=n) < 0.4}[kind]
    if kind == "some":
        inl[n // 2] = True
    return a, b, inl, err


def check_sim3(a, b, inl, err):
    """Against the float64 restatement fed the same fp32 inputs: 1e-6 on the rotation entries (the mean and the aligned cameras)
    and the scale, 1e-4 degrees on the errors and their statistics."""
    ta, tb = dev(a), dev(b)
    keep_a, keep_b = ta.clone(), tb.clone()
    ti = None if inl is None else dev(inl)
    out, fit = CM.align_sim3(ta, tb, ti, None if inl is None else dev(err))
    want = cn.align_sim3(a, b, inl, err)
    assert torch.equal(ta, keep_a) and torch.equal(tb, keep_b) and (inl is None or np.array_equal(np_(ti), inl))
    o = np_(out).astype(np.float64)
    d_rot = max(np.abs(np_(fit.rotation) - want["rotation"]).max(), np.abs(o[:, :3, :3] - want["b"][:, :3, :3]).max())
    d_scale = abs(float(np_(fit.scale)) - want["scale"])
    d_t = np.abs(o[:, :3, 3] - want["b"][:, :3, 3]).max()
    d_err = np.abs(np_(fit.so3_err).astype(np.float64) - want["so3_err"]).max()
    d_stats = np.nanmax(np.abs(np_(fit.stats) - want["stats"]))
    print(len(a), "rot", d_rot, "scale", d_scale, "t", d_t, "err", d_err, "stats", d_stats, "status", np_(fit.status))
    assert d_rot < 1e-6 and d_scale < 1e-6 and d_t < 1e-6 and d_err < 1e-4 and d_stats < 1e-4
    assert np.array_equal(np.isnan(np_(fit.stats)), np.isnan(want["stats"]))
    assert np.array_equal(np_(fit.inlier_used), want["used"]) and np.array_equal(bits(o[:, 3]), bits(b[:, 3]))
    st = np_(fit.status)
    assert st[0] == want["zero_norm"] and st[1] == int(want["fallback"]) and st[2] == int(want["used"].sum())
    return fit, want


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("kind", ["none", "allfalse", "some", "all"])
def test_align_sim3_against_float64(n, kind):
    a, b, inl, err = sim3_inputs(n, kind)
    fit, want = check_sim3(a, b, inl, err)
    if kind == "allfalse":
        assert np.nonzero(np_(fit.inlier_used))[0].tolist() == [int(np.argmin(err))]


def test_align_sim3_wide_spread_and_zero_translation():
    a, b, inl, err = sim3_inputs(257, "none", seed=3, max_deg=120.0)
    dso3 = np.matmul(b[:, :3, :3].astype(np.float64).transpose(0, 2, 1), a[:, :3, :3].astype(np.float64))
    lam = cn.mean_rotation(dso3)[1]
    assert lam[-1] - lam[-2] > 0.1 * len(a)                                  # the mean is well defined
    fit, _ = check_sim3(a, b, inl, err)
    assert abs(float(np_(fit.eig)[0]) - lam[-1]) < 1e-9 * len(a)
    a, b, inl, err = sim3_inputs(65, "some")
    b[[3, 40], :3, 3] = 0                                                   # one of them an inlier or not: the count is over all frames
    inl[3] = False
    _, fit = CM.align_sim3(dev(a), dev(b), dev(inl), dev(err))
    assert np_(fit.status)[0] == 2


# ---- visual_hull_align --------------------------------------------------------------------------------------------------------
def run_hull(scene, G_=64, masks=None, dtype=torch.float32):
    p = "hull/%s/" % scene
    m = G[p + "masks"] if masks is None else masks
    return CM.visual_hull_align(dev(G[p + "rtk"]), dev(G[p + "kaug"]), dev(m, dtype), grid_size=G_, return_scores=True)


@pytest.mark.parametrize("scene", HULL)
def test_hull_against_float64_on_the_golden_scenes(scene):
    p = "hull/%s/" % scene
    want = hull(scene)
    V = G[p + "masks"].shape[0]
    out, status, scores = run_hull(scene, dtype=torch.uint8 if scene == "v7" else (torch.bool if scene == "v3" else torch.float32))
    band = np.abs(want["scores"] - 0.8 * V) < 1e-4
    sel = np_(scores).astype(np.float64) > 0.8 * V
    d = np.abs(np_(out).astype(np.float64)[:, :3, 3] - want["rtk"][:, :3, 3]).max() / float(want["bound"])
    print(scene, "score difference", np.abs(np_(scores) - want["scores"]).max(), "translations / bound", d, "status", np_(status))
    assert band.sum() <= 4 and np.array_equal(sel[~band], want["selected"][~band])
    assert d < 1e-5
    assert np_(status).tolist() == [0, 0, int(want["selected"].sum()), 0] and out.shape == (V, 4, 4)
    assert np.array_equal(bits(np_(out)[:, :3, :3]), bits(G[p + "rtk"][:V, :3, :3])) and np.array_equal(bits(np_(out)[:, 3]), bits(G[p + "rtk"][:V, 3]))


@pytest.mark.parametrize("G_", [20, 8])
def test_hull_on_other_lattices(G_):
    p = "hull/v12/"
    want = cn.visual_hull_align(G[p + "rtk"], G[p + "kaug"], G[p + "masks"], G_)
    out, status, scores = run_hull("v12", G_)
    assert scores.shape == (G_ ** 3,) and np.abs(np_(scores) - want["scores"]).max() < 1e-5
    assert np_(status).tolist() == [0, int(want["empty"]), int(want["selected"].sum()), 0]
    assert np.abs(np_(out).astype(np.float64)[:, :3, 3] - want["rtk"][:, :3, 3]).max() < 1e-5 * float(want["bound"])


def test_hull_empty_selection_same_bits_and_graph_replay():
    p = "hull/v10/"
    out, status, _ = run_hull("v10", masks=np.zeros_like(G[p + "masks"]))
    assert np_(status).tolist() == [0, 1, 0, 0] and np.array_equal(bits(np_(out)), bits(G[p + "rtk"]))
    one, two = run_hull("v10"), run_hull("v10")
    assert all(torch.equal(x, y) for x, y in zip(one, two))
    rtk, kaug, m = dev(G[p + "rtk"]), dev(G[p + "kaug"]), dev(np.zeros_like(G[p + "masks"]), torch.float32)
    CM.visual_hull_align(rtk, kaug, m, return_scores=True)                      # the eager warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = CM.visual_hull_align(rtk, kaug, m, return_scores=True)
    m.copy_(dev(G[p + "masks"], torch.float32))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(res, one))


# ---- draw_cams, eval_root, align_sfm_sim3 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 130])
def test_draw_cams_against_numpy(n):
    """Vertices at 1e-6 of the scale -- the reference's `scale`, the median translation norm, of which the glyph radius is 0.02:
    fp32 vertices lie 6e-8 of their own size apart, and they are as large as the translations -- faces and colours exact."""
    rng = np.random.default_rng(n)
    c = cams(rotations(rng, n), rng.standard_normal((n, 3)) * 2 + [0, 0, 4])
    c[n // 2, :3, 3] = 0                                                    # excluded from the median
    for color in ("cool", "gray"):
        mesh = CM.draw_cams(dev(c), color=color)
        v, f, col, scale = cn.draw_cams(c, color)
        assert np.abs(mesh.vertices - v).max() < 1e-6 * scale
        assert np.array_equal(mesh.faces, f) and np.array_equal(mesh.visual.vertex_colors, col)
    m1, m2, lines = CM.draw_cams_pair(dev(c), dev(c[::-1].copy()))
    assert lines.vertices.shape == (8 * n, 3) and lines.faces.max() == 8 * n - 1 and m1.vertices.shape == m2.vertices.shape
    centres = -np.einsum('nji,nj->ni', c[:, :3, :3].astype(np.float64), c[:, :3, 3].astype(np.float64))
    ends = lines.vertices.reshape(n, 2, 4, 3).mean(2)
    assert np.abs(ends[:, 0] - centres).max() < 1e-5 and np.abs(ends[:, 1] - centres[::-1]).max() < 1e-5


def test_eval_root_and_align_sfm_sim3_are_the_chain_of_the_pieces():
    a, b, _, err = sim3_inputs(40, "none")
    aligned, fit, mesh = CM.eval_root(dev(a), dev(b))
    al2, fit2 = CM.align_sim3(dev(a), dev(b))
    both = CM.concatenate([CM.draw_cams(dev(a), color='gray'), CM.draw_cams(al2)])
    assert torch.equal(aligned, al2) and torch.equal(fit.stats, fit2.stats) and torch.equal(mesh.vertices_t, both.vertices_t)
    assert torch.equal(mesh.faces_t, both.faces_t) and np.array_equal(mesh.visual.vertex_colors, both.visual.vertex_colors)
    p = "hull/v12/"
    V = 12
    rng = np.random.default_rng(2)
    pred = dev(cams(rotations(rng, V + 5), rng.standard_normal((V + 5, 3)) + [0, 0, 3]))
    valid = dev(rng.uniform(size=V + 5) < 0.5)
    e = dev(rng.uniform(size=V + 5).astype(np.float32))
    kaug = dev(np.concatenate([np.tile([1., 1, 0, 0], (5, 1)), G[p + "kaug"]]).astype(np.float32))
    masks = torch.zeros((V + 5, 32, 32), device=DEV)
    masks[5:] = dev(G[p + "masks"], torch.float32)
    prior = dev(G[p + "rtk"])
    keep = pred.clone()
    rtk, ok = CM.align_sfm_sim3(pred, valid, e, kaug, masks, [None, prior], [0, 5, V + 5])
    centred = CM.visual_hull_align(prior, kaug[5:], masks[5:])[0]
    want = CM.align_sim3(pred[5:], centred, is_inlier=valid[5:], err_valid=e[5:])[0]
    assert torch.equal(pred, keep) and torch.equal(rtk[:5], pred[:5]) and torch.equal(rtk[5:], want)
    assert torch.equal(ok[:5], valid[:5]) and bool(ok[5:].all())
