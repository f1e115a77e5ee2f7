"""GPU (-m gpu): the mesh rasteriser (moda_amd/mesh_render.py, soft_renderer.py, geom_utils.render_color / render_flow,
csrc/raster_kernels.hip) against the float64 oracle tests/raster_numpy.py and the reference-recorded fixture G29.

What pins what: tests/test_raster_oracle.py pins the oracle's kernel restatement on closed forms and the code around the kernel
on G29, which the reference's own soft_renderer / geom_utils wrote; here the HIP route is held to the oracle and to G29.
render_dp is not in G29 (see gen_golden_raster.py), so its stated properties are tested instead.

Bars, with u = 2^-24:
  face_idx, alpha  EQUAL to the oracle at every pixel whose edge margin exceeds 1e-4 and whose depth margin exceeds 1e-5.
            A barycentric w_k = A x + B y + C is a sum of terms of size about |x| / (height of the face) that cancel.  For
            faces of height >= 0.01 NDC an fp32 evaluation would stay within a few 1e-5, but the foreshortened faces at the
            limb of these spheres are down to 1e-5 NDC high, and an fp32 evaluation of w was measured on the card at up to
            3.7e-3 from the oracle in w_clip (2e-5 relative in zp) at pixels outside the margins.  The kernel therefore forms
            the edge equations and w in float64 from the same fp32 vertices and the same pixel centres as the oracle: its w
            differs from the oracle's by float64 rounding (1e-16 |x| / height, 1e-11 for these faces), so inside / outside and
            the order of depths can differ only inside the margins.  The fp32 steps after it (w -> fp32, the renormalising
            division, three divisions and a sum of positive terms for zp) cost a few u each.  Pixels inside the margins
            are left out, and AT MOST 1 % of the covered pixels of a scene may be (a condition on the scene, asserted; the
            share is printed).
  bary, attributes  |gpu - oracle| <= 1e-4 * max|attr| absolute at the compared pixels (w_clip = w / sum w: a few u, see above).
  zbuf      1e-5 relative.
  observed maxima are printed in units of u."""
import numpy as np
import pytest
import torch

import raster_numpy as rn
from helpers import golden
from test_raster_oracle import REPLICA_SCENES, REPLICA_SIZES, CHUNK_FACES, CHUNK_SEEDS, replica_scene

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import moda_amd
    from moda_amd import mesh as M, mesh_render as R, soft_renderer as sr, geom_utils as G
    from gpu_helpers import T, DEV

U = 2.0 ** -24
EDGE, DEPTH, CAP = 1e-4, 1e-5, 0.01


def I(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.int32, device=DEV)


views = rn.views


def check_against_oracle(verts, faces, S, name, near=1.0, far=100.0, attrs=None):
    """verts (B,V,3) fp32, faces (F,3) or (B,F,3): rasterize (+ interpolate) on the GPU and hold every view to the oracle."""
    B = len(verts)
    fi, bw, zb, al = R.rasterize(T(verts), I(faces), S, near=near, far=far)
    assert fi.shape == (B, S, S) and fi.dtype == torch.int32 and bw.shape == (B, S, S, 3) and zb.shape == al.shape == (B, S, S)
    img = None if attrs is None else R.interpolate(T(attrs), I(faces), fi, bw).cpu().numpy()
    fi, bw, zb, al = fi.cpu().numpy(), bw.cpu().numpy().astype(np.float64), zb.cpu().numpy().astype(np.float64), al.cpu().numpy()
    assert np.isfinite(bw).all() and np.isfinite(zb).all() and set(np.unique(al)) <= {0.0, 1.0}
    for b in range(B):
        f = faces if np.ndim(faces) == 2 else faces[b]
        r = rn.rasterize(verts[b][f], S, near, far)
        ok = (r.edge_margin > EDGE) & (r.depth_margin > DEPTH)
        covered = int(r.alpha.sum())
        left = int((r.alpha & ~ok).sum())
        hit = ok & (r.face_idx >= 0)
        eb = np.abs(bw[b][hit] - r.bary[hit]).max() if hit.any() else 0.0
        ez = (np.abs(zb[b][hit] - r.zbuf[hit]) / r.zbuf[hit]).max() if hit.any() else 0.0
        print(f"{name} view {b} S {S}: covered {covered}, left out {left} ({100.0 * left / max(covered, 1):.3f} %), "
              f"max |bary err| {eb / U:.1f} u, max zbuf rel err {ez / U:.1f} u")
        assert left <= CAP * covered, "the scene itself breaks the 1 % condition: replace the scene"
        assert np.array_equal(fi[b][ok], r.face_idx[ok])
        assert np.array_equal(al[b][ok] > 0, r.alpha[ok])
        assert (fi[b][al[b] == 0] == -1).all() and (zb[b][fi[b] < 0] == 0).all()
        assert eb <= 1e-4 and ez <= 1e-5
        if attrs is not None:
            want = rn.interpolate(attrs[b][f], r)
            ea = np.abs(img[b] - want)[:, ok].max()
            print(f"    max |attr err| {ea / U:.1f} u of max |attr| {np.abs(attrs).max():.3f}")
            assert ea <= 1e-4 * np.abs(attrs).max()
            assert (img[b][:, fi[b] < 0] == 0).all()
    return fi


@pytest.mark.parametrize("sub,S,seeds", [(4, 64, (1, 2, 3)), (4, 257, (4,)), (4, 50, (5,)), (5, 256, (6, 8, 9)), (5, 64, (7,))])
def test_icosphere_matches_oracle(sub, S, seeds):
    v, f = rn.icosphere(sub, 0.9)
    assert len(f) == 20 * 4 ** sub
    vs = views(v, seeds)
    attrs = np.random.default_rng(sub).uniform(-1, 1, (len(seeds), len(v), 5)).astype(np.float32)
    check_against_oracle(vs, f, S, f"icosphere{sub}", attrs=attrs)


def test_sixteen_views_and_per_view_faces():
    v, f = rn.icosphere(3, 0.85)
    vs = views(v, range(20, 36))
    fi = check_against_oracle(vs, f, 64, "icosphere3 x16")
    rng = np.random.default_rng(0)
    fpv = np.stack([f[rng.permutation(len(f))] for _ in range(3)])            # another face order per view
    fi3 = check_against_oracle(vs[:3], fpv, 64, "per-view faces")
    same = (fi[:3] >= 0) == (fi3 >= 0)
    assert same.all()


def test_interpenetrating_spheres_and_off_screen():
    v1, f1 = rn.icosphere(4, 0.6)
    v2, f2 = rn.icosphere(3, 0.5)
    v = np.concatenate([v1 + [-0.25, 0.1, 0.0], v2 + [0.3, -0.1, 0.2]])
    f = np.concatenate([f1, f2 + len(v1)])
    vs = views(v, (8, 9, 10, 11))
    vs[1, :, 0] += 0.9                                                        # partly off-screen
    vs[2, :, 1] -= 3.0                                                        # fully off-screen: background, nothing else
    vs[3, :, 2] += 200.0                                                      # beyond far: alpha without colour
    fi = check_against_oracle(vs, f, 128, "two spheres")
    assert (fi[2] == -1).all() and (fi[3] == -1).all() and (fi[1] >= 0).any()
    _, _, _, al = R.rasterize(T(vs), I(f), 128)
    assert (al[2] == 0).all() and (al[3] > 0).any()


def mc_scene(n=32):
    """The GPU marching-cubes mesh of the synthetic sphere SDF, scaled into the view volume."""
    v, f = M.marching_cubes(T(rn.sphere_volume(n)), 0.0)
    v, f = v.cpu().numpy().astype(np.float64), f.cpu().numpy().astype(np.int64)
    assert len(f) > 3000
    return (v - (n - 1) / 2) / (0.5 * n) * 0.8, f


def test_marching_cubes_mesh_matches_oracle():
    v, f = mc_scene()
    check_against_oracle(views(v, (12, 13)), f, 256, "marching cubes")


def test_one_face_and_one_pixel():
    tri = np.array([[[-0.6, -0.55, 2.0], [0.75, -0.25, 3.0], [-0.25, 0.8, 4.0]]], np.float32)
    f = np.array([[0, 1, 2]])
    for S in (1, 2, 16, 17):
        check_against_oracle(tri, f, S, "one face")
    fi, bw, zb, al = R.rasterize(T(tri), I(f), 1)
    assert int(fi[0, 0, 0]) == 0 and float(al[0, 0, 0]) == 1.0                # the centre (0, 0) lies in the triangle
    # degenerate faces are handled, not trapped: nothing drawn, nothing non-finite; bad vertex indices are skipped
    flat = np.array([[[-0.5, -0.5, 2.0], [0.0, 0.0, 2.0], [0.5, 0.5, 2.0]]], np.float32)
    for verts, faces in ((flat, f), (tri, np.array([[0, 1, 7]])), (tri, np.array([[0, -1, 2]])), (tri[:, [0, 0, 0]], f)):
        fi, bw, zb, al = R.rasterize(T(verts), I(faces), 16)
        assert (fi == -1).all() and (al == 0).all() and (zb == 0).all() and torch.isfinite(bw).all()


def test_tie_rule_depth_range_and_windings():
    S = 32
    a, b = -0.5, 0.5
    quad = np.array([[a, a, 2.0], [b, a, 2.0], [b, b, 2.0], [a, b, 2.0]], np.float32)
    verts = np.concatenate([quad, quad, quad * [1, 1, 0.25], quad * [1, 1, 75.0]])[None].astype(np.float32)     # z = 2, 2, 0.5, 150
    f = np.array([[4, 5, 6], [0, 1, 2], [0, 2, 3], [6, 5, 4], [8, 9, 10], [12, 14, 13]])
    fi, bw, zb, al = R.rasterize(T(verts), I(f), S)
    fi = fi[0].cpu().numpy()
    r = rn.rasterize(verts[0][f], S)
    assert np.array_equal(fi, r.face_idx) and np.array_equal(al[0].cpu().numpy() > 0, r.alpha)
    assert set(np.unique(fi)) == {-1, 0, 2}                                   # equal depth: the lower index; out of range: never
    assert (zb[0].cpu().numpy()[fi >= 0] == 2.0).all()


@pytest.mark.parametrize("C", [1, 3, 16, 17])
def test_channels_equal_three_wide_renders_bit_for_bit(C):
    v, f = rn.icosphere(4, 0.9)
    vs = views(v, (14, 15))
    fi, bw, _, _ = R.rasterize(T(vs), I(f), 96)
    attrs = T(np.random.default_rng(C).standard_normal((2, len(v), C)).astype(np.float32))
    full = R.interpolate(attrs, I(f), fi, bw, background=0.25)
    assert full.shape == (2, C, 96, 96)
    for i in range(0, C, 3):
        chunk = attrs[..., i:i + 3]
        while chunk.shape[-1] < 3:                                            # moda.py:989-991: padded with the first channels
            chunk = torch.cat([chunk, attrs[..., :3 - chunk.shape[-1]]], -1)
        assert chunk.shape[-1] == 3
        part = R.interpolate(chunk.contiguous(), I(f), fi, bw, background=0.25)
        k = min(3, C - i)
        assert torch.equal(part[:, :k], full[:, i:i + k])


def test_binned_equals_unbinned_and_runs_are_identical():
    v, f = rn.icosphere(5, 0.9)
    vs = views(v, (16, 17, 18))
    a = R.rasterize(T(vs), I(f), 257)
    b = R.rasterize(T(vs), I(f), 257)
    c = R.rasterize(T(vs), I(f), 257, binned=False)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


# ---- the order guarantee: the lowest face index wins equal depths, wherever the equal faces sit in the list ----------------------
# tests/test_raster_oracle.py holds the oracle to the same statements on the same face lists (REPLICA_SCENES, CHUNK_FACES).

def _scene(name):
    return mc_scene() if name == "marching cubes" else replica_scene(name)


def _assert_replica(single, got, lowest, what):
    """got = the render of a list in which face i of the single list first appears at index lowest[i]."""
    fi, bw, zb, al = single
    want = torch.where(fi >= 0, torch.as_tensor(lowest, dtype=torch.int32, device=DEV)[fi.clamp(min=0).long()], fi)
    assert torch.equal(got[0], want), what + ": face_idx"
    for x, y, k in zip(single[1:], got[1:], ("bary", "zbuf", "alpha")):
        assert x.dtype == torch.float32 and torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{what}: {k}"


@pytest.mark.parametrize("binned", [True, False])
@pytest.mark.parametrize("S", REPLICA_SIZES)
@pytest.mark.parametrize("name", sorted(REPLICA_SCENES) + ["marching cubes"])
def test_replicated_faces_keep_the_lowest_copy(name, S, binned):
    """Copies of a face have identical records, hence identical zp in every lane; < is strict, so the lowest copy wins and
    every other comparison is the one of the single list: all four outputs are the single render's bit for bit."""
    v, f = _scene(name)
    seeds = REPLICA_SCENES.get(name, (12, 13))
    vs = T(views(v, seeds))
    single = R.rasterize(vs, I(f), S, binned=binned)
    covered = int((single[0] >= 0).sum())
    assert covered > 0.2 * len(seeds) * S * S and len(torch.unique(single[0])) > 30
    for kind, faces, lowest in rn.replicas(f):
        got = R.rasterize(vs, I(faces), S, binned=binned)
        _assert_replica(single, got, lowest, f"{name} S {S} binned {binned} {kind}")
    print(f"{name} S {S} binned {binned}: F {len(f)}, {covered} pixels drawn, each a tie in every replica")


def test_replicated_faces_match_the_oracle_and_per_view_lists():
    S = 64
    for name in sorted(REPLICA_SCENES):
        v, f = replica_scene(name)
        vs = views(v, REPLICA_SCENES[name][:2])
        for kind, faces, lowest in rn.replicas(f):
            fi = R.rasterize(T(vs), I(faces), S)[0].cpu().numpy()
            for b in range(len(vs)):
                # depth_margin is 0 wherever a copy ties: the face index is compared directly, at the pixels that the
                # single list's margins clear
                r1, r = rn.rasterize(vs[b][f], S), rn.rasterize(vs[b][faces], S)
                ok = (r1.edge_margin > EDGE) & (r1.depth_margin > DEPTH)
                assert (r1.alpha & ~ok).sum() <= CAP * r1.alpha.sum()
                assert np.array_equal(fi[b][ok], r.face_idx[ok]), (name, kind, b)
    # another face order per view, and the replicas of each view's own list
    v, f = replica_scene("icosphere4")
    vs = T(views(v, (31, 32, 33)))
    rng = np.random.default_rng(1)
    fpv = np.stack([f[rng.permutation(len(f))] for _ in range(3)])
    single = R.rasterize(vs, I(fpv), 257)
    assert int((single[0] >= 0).sum()) > 0.2 * 3 * 257 * 257
    for kind in range(3):
        per_view = [rn.replicas(x)[kind] for x in fpv]
        assert all(np.array_equal(p[2], per_view[0][2]) for p in per_view)
        got = R.rasterize(vs, I(np.stack([p[1] for p in per_view])), 257)
        _assert_replica(single, got, per_view[0][2], f"per-view faces {per_view[0][0]}")


@pytest.mark.parametrize("F", CHUNK_FACES)
def test_face_counts_around_the_chunk_size(F):
    """The first F faces of icosphere 4's list: the last 256-face chunk holds 255, 256, 1, .. faces."""
    v, f = rn.icosphere(4, 0.9)
    attrs = np.random.default_rng(F).uniform(-1, 1, (len(CHUNK_SEEDS), len(v), 3)).astype(np.float32)
    fi = check_against_oracle(views(v, CHUNK_SEEDS), f[:F], 64, f"icosphere4[:{F}]", attrs=attrs)
    assert (fi >= 0).any() and fi.max() < F
    a = R.rasterize(T(views(v, CHUNK_SEEDS)), I(f[:F]), 64)
    c = R.rasterize(T(views(v, CHUNK_SEEDS)), I(f[:F]), 64, binned=False)
    for x, z in zip(a, c):
        assert torch.equal(x, z)


def rodrigues(a):
    """float64 rotation matrices of axis-angle vectors (n,3): I + sin(t) K + (1 - cos(t)) K^2."""
    a = np.asarray(a, np.float64)
    out = []
    for v in a:
        t = np.linalg.norm(v)
        k = v / t if t > 0 else v
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        out.append(np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K)
    return np.stack(out)


def renderer(S=64):
    return sr.SoftRenderer(image_size=S, sigma_val=1e-12,
                           camera_mode='look_at', perspective=False, aggr_func_rgb='hard',
                           light_mode='vertex', light_intensity_ambient=1., light_intensity_directionals=0.)


def g29_masks(g, name, S):
    fv = g[f"{name}_face_vertices"]
    rs = [rn.rasterize(fv[b], S) for b in range(len(fv))]
    ok = np.stack([(r.edge_margin > EDGE) & (r.depth_margin > DEPTH) for r in rs])
    return ok, np.stack([r.alpha for r in rs])


def test_render_color_matches_g29():
    g = golden("g29_mesh_render")
    S = int(g["image_size"])
    rend = renderer(S)
    assert np.array_equal(np.asarray(rend.transform.transformer._eye, np.float64), g["eye"])
    for name in g["cases"].tolist():
        verts, faces, colors = g[f"{name}_verts"], g[f"{name}_faces"], g[f"{name}_colors"]
        B = len(verts)
        out = G.render_color(rend, T(verts), I(faces)[None].repeat(B, 1, 1), T(colors)).cpu().numpy()
        want = g[f"{name}_rendered"]
        assert out.shape == want.shape == (B, 4, S, S)
        ok, cov = g29_masks(g, name, S)
        assert (cov & ~ok).sum() <= CAP * cov.sum()
        err = np.abs(out - want)[:, :3][np.broadcast_to(ok[:, None], (B, 3, S, S))].max()
        print(name, "max |colour err|", err / U, "u; left out", int((cov & ~ok).sum()), "of", int(cov.sum()))
        assert err <= 1e-4 * np.abs(colors).max()
        assert np.array_equal(out[:, 3][ok], want[:, 3][ok])


def test_render_flow_matches_g29_and_vanishes_on_itself():
    g = golden("g29_mesh_render")
    S = int(g["image_size"])
    rend = renderer(S)
    verts, faces, vn = g["flow_verts"], g["flow_faces"], g["flow_verts_n"]
    B = len(verts)
    fl = G.render_flow(rend, T(verts), I(faces)[None].repeat(B, 1, 1), T(vn)).cpu().numpy()
    want = g["flow_rendered"]
    ok, cov = g29_masks(g, "flow", S)
    assert fl.shape == want.shape == (B, S, S, 3) and (fl[..., 2] == 0).all()
    err = np.abs(fl - want)[ok].max()
    print("max |flow err|", err / U, "u")
    assert err <= 1e-4 * max(np.abs(vn).max(), 1.0)
    assert np.array_equal((fl != 0).any(-1)[ok], (want != 0).any(-1)[ok])
    # a mesh against itself: the rendered NDC position is the pixel centre; the reference's grid is i * 2 / (w - 1) - 1, which
    # differs from the centres by (2 i + 1 - S) / S - (2 i / (S - 1) - 1), at most 1 / S at the border.  With y pre-flipped the
    # rendered y is that of the pixel's row, so the residual is exactly that grid difference: checked to 1e-6
    own = G.render_flow(rend, T(verts), I(faces)[None].repeat(B, 1, 1), T(verts)).cpu().numpy()
    i = np.arange(S, dtype=np.float64)
    d = (2 * i + 1 - S) / S - (2 * i / (S - 1) - 1)
    sil = ok & cov
    assert np.abs(own[..., 0] - d[None, None, :])[sil].max() <= 1e-6
    assert np.abs(own[..., 1] - d[None, :, None])[sil].max() <= 1e-6
    assert (own[~cov & ok] == 0).all()


def test_render_dp_properties():
    v, f = rn.icosphere(4, 1.0)
    rng = np.random.default_rng(3)
    embed = np.abs(rng.standard_normal((len(v), 16))).astype(np.float32) + 0.1
    near_far = T(np.asarray([[4.0, 8.0]], np.float32))
    rend = renderer(256)
    bs = 4
    np.random.seed(11)
    feats, rtk = moda_amd.render_dp(T(v.astype(np.float32) * 0.9), I(f), T(embed), near_far, DEV, rend, bs)
    assert feats.shape == (bs, 16, 112, 112) and rtk.shape == (bs, 4, 4)
    norm = feats.norm(dim=1)
    nz = norm > 0
    assert nz.any() and (norm[nz] - 1).abs().max() <= 1e-5
    # the oracle's cameras: the same draws, the same torch crop, raster_numpy in place of the kernels
    # the expected rtk, built here from the np.random draws replayed in the reference's order (moda.py:952, :958) and a
    # float64 Rodrigues formula: nothing of mesh_render.py goes into it
    np.random.seed(11)
    dep = np.float32(1 + np.random.normal(0, 0.5, bs))
    rot = np.random.normal(0, 6.28, (bs, 3)).astype(np.float32)
    want_rtk = np.zeros((bs, 4, 4))
    want_rtk[:, :3, :3] = rodrigues(rot)
    want_rtk[:, 2, 3] = np.maximum(np.float32(6.0) * dep, np.float32(1.2 * 1 / 3 * 6.0))       # moda.py:954-955, fp32
    want_rtk[:, 3] = [256.0, 256.0, 128.0, 128.0]
    got = rtk.cpu().numpy().astype(np.float64)
    print("render_dp max |rtk - expected|", np.abs(got - want_rtk).max() / U, "u")
    assert np.array_equal(got[:, 3], want_rtk[:, 3]) and np.array_equal(got[:, :3, 3], want_rtk[:, :3, 3])
    # the rotation in fp32: the angle t = |a| carries 2 u t of rounding, the half-angle's sine and cosine u t + 2 u each, and
    # an entry is twice a sum of two products of them: 4 (t + 3) u.  The translation and intrinsics are exact
    t = np.linalg.norm(rot.astype(np.float64), axis=1)
    assert (np.abs(got[:, :3, :3] - want_rtk[:, :3, :3]).max((1, 2)) <= 4 * (t + 3) * U).all()
    np.random.seed(11)
    Rm, Tm, K, rtk_o, d_mean = R.dp_cameras(near_far, DEV, bs)
    assert torch.equal(rtk, rtk_o)
    assert torch.equal(rtk[:, 3], T(np.tile(np.asarray([[256.0, 256.0, 128.0, 128.0]], np.float32), (bs, 1))))
    assert (rtk[:, 2, 3] >= 0.4 * 6.0 - 1e-6).all()
    verts = G.pinhole_cam(G.obj_to_cam((T(v.astype(np.float32) * 0.9) / 3 * d_mean)[None].repeat(bs, 1, 1), Rm, Tm), K)
    eye = torch.Tensor(rend.transform.transformer._eye).to(DEV)
    pre = verts - eye
    pre[:, :, 1] = -1 * pre[:, :, 1]
    pre = (pre - eye).cpu().numpy()
    imgs, oks = [], []
    for b in range(bs):
        img, r = rn.render(pre[b][f], embed[f], 256, background=0.0)
        imgs.append(img[:16])
        oks.append((r.edge_margin > EDGE) & (r.depth_margin > DEPTH))
    full = G.render_color(rend, verts, I(f), T(embed)[None].repeat(bs, 1, 1)).cpu().numpy()
    ok = np.stack(oks)
    err = np.abs(full[:, :16] - np.stack(imgs))[np.broadcast_to(ok[:, None], (bs, 16, 256, 256))].max()
    print("render_dp full-size max |err|", err / U, "u")
    assert err <= 1e-4 * np.abs(embed).max()
    # the crops of the oracle images, with mask_aug's draws replayed from the same state
    state = np.random.get_state()
    np.random.seed(11)
    R.dp_cameras(near_far, DEV, bs)
    want = R.dp_crops(T(np.stack(imgs).astype(np.float32)))
    np.random.set_state(state)
    # away from resampled silhouette pixels: where both are non-zero and the 3 x 3 neighbourhood of the oracle is non-zero
    wz = (want.norm(dim=1, keepdim=True) > 0).float()
    inner = (torch.nn.functional.avg_pool2d(wz, 5, 1, 2) == 1)[:, 0] & (feats.norm(dim=1) > 0)
    rel = ((feats - want).abs().amax(1) / want.abs().amax(1).clamp(min=1e-12))[inner].max()
    print("render_dp crop max rel err away from the silhouette", float(rel), "over", int(inner.sum()), "pixels")
    assert inner.sum() > 1000 and float(rel) <= 1e-3


def test_render_mesh_depth_and_silhouette():
    v, f = rn.icosphere(4, 0.5)
    d, S = 3.0, 128
    rtk = np.eye(4, dtype=np.float32)
    rtk[:3, :3] = rn.rotation(5)
    rtk[:3, 3] = [0.1, -0.05, d]
    rtk[3] = [200.0, 200.0, 64.0, 64.0]
    mesh = M.TriMesh(T(v.astype(np.float32)), I(f))
    colors = np.full((len(v), 4), 255, np.uint8)
    colors[:, 1] = 128
    mesh.visual.vertex_colors = colors
    for smooth in (True, False):
        color, depth, sil = moda_amd.render_mesh(mesh, rtk, S, smooth=smooth)
        assert color.shape == (S, S, 3) and color.dtype == torch.uint8 and depth.shape == (S, S) and depth.dtype == torch.float32
        assert torch.equal(sil, depth > 0) and sil.sum() > 1000
        c = color.cpu().numpy()
        s = sil.cpu().numpy()
        assert (c[0, 0] == 0).all() and (c[~s] == 0).all() and (c[s] > 0).all()
    # closed form: the depth at a pixel is where its ray (u - px) / fx, (v - py) / fy, 1 meets the plane of the face drawn there
    cam = v.astype(np.float32).astype(np.float64) @ rtk[:3, :3].astype(np.float64).T + rtk[:3, 3].astype(np.float64)
    ndc = np.stack([(200.0 * cam[:, 0] / cam[:, 2] + 64.0) * (2.0 / S) - 1, -((200.0 * cam[:, 1] / cam[:, 2] + 64.0) * (2.0 / S) - 1),
                    cam[:, 2]], -1)
    r = rn.rasterize(ndc[f], S, 1e-3, 1000.0)
    ok = (r.edge_margin > EDGE) & (r.depth_margin > DEPTH) & (r.face_idx >= 0)
    rows, cols = np.nonzero(ok)
    tri = cam[f[r.face_idx[ok]]]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    ray = np.stack([(cols + 0.5 - 64.0) / 200.0, (rows + 0.5 - 64.0) / 200.0, np.ones(len(rows))], -1)
    want = (nrm * tri[:, 0]).sum(-1) / (nrm * ray).sum(-1)
    got = depth.cpu().numpy().astype(np.float64)[ok]
    rel = np.abs(got - want) / want
    grazing = np.abs((nrm * ray).sum(-1)) / (np.linalg.norm(nrm, axis=-1) * np.linalg.norm(ray, axis=-1)) < 0.05
    print("render_mesh max depth rel err", rel[~grazing].max() / U, "u over", int((~grazing).sum()), "pixels")
    assert (~grazing).sum() > 1000 and rel[~grazing].max() <= 1e-5
    assert np.array_equal(sil.cpu().numpy()[(r.edge_margin > EDGE)], r.alpha[(r.edge_margin > EDGE)])


def test_refusals():
    moda = dict(image_size=64, sigma_val=1e-12, camera_mode='look_at', perspective=False, aggr_func_rgb='hard',
                light_mode='vertex', light_intensity_ambient=1., light_intensity_directionals=0.)
    for key, value in (("aggr_func_rgb", "softmax"), ("perspective", True), ("light_intensity_directionals", 0.5),
                       ("anti_aliasing", True), ("camera_mode", "look"), ("camera_mode", "projection"), ("sigma_val", 1e-4),
                       ("aggr_func_alpha", "sum"), ("dist_func", "barycentric"), ("fill_back", False)):
        with pytest.raises(NotImplementedError, match=key):
            sr.SoftRenderer(**{**moda, key: value})
    v, f = rn.icosphere(1, 0.5)
    vs = views(v, (1,))
    with pytest.raises(NotImplementedError, match="texture_type"):
        sr.Mesh(T(vs), I(f), texture_type='surface')
    with pytest.raises(NotImplementedError, match="texture_type"):
        G.render_color(renderer(), T(vs), I(f)[None], T(vs), texture_type='surface')
    rend = renderer()
    rend.transform.transformer._eye = [1.0, 0.0, -2.0]
    with pytest.raises(NotImplementedError, match="eye"):
        G.render_color(rend, T(vs), I(f)[None], T(vs))
    x = T(vs).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="gradients"):
        R.rasterize(x, I(f), 16)
    with pytest.raises(NotImplementedError, match="gradients"):
        G.render_color(renderer(), T(vs), I(f)[None], x)
    with pytest.raises(RuntimeError, match="CUDA"):
        R.rasterize(torch.as_tensor(vs), I(f), 16)
    with pytest.raises(RuntimeError, match="CUDA"):
        R.rasterize(T(vs), torch.as_tensor(f), 16)
    bad = vs.copy()
    bad[0, 3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        R.rasterize(T(bad), I(f), 16)
    with pytest.raises(ValueError):
        R.rasterize(T(vs), I(f), 0)
    with pytest.raises(TypeError):
        R.rasterize(T(vs), T(f.astype(np.float32)), 16)
