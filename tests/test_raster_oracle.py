"""CPU (no GPU needed): the float64 oracle tests/raster_numpy.py.

What pins what.  The kernel restatement (coverage rule, depth, tie rule, near / far, alpha before the depth test) is pinned by
the ANALYTIC tests here, whose expected values are closed forms that do not come from raster_numpy.  Everything around the
kernel (eye offset and its second subtraction in look_at, y pre-flip, face-vertex gathering, lighting, channel layout,
render_flow's (w-1) grid and masking, obj_to_cam, pinhole_cam) is pinned by G29, which tests/golden/gen_golden_raster.py
recorded from the reference's own soft_renderer / geom_utils code run on the CPU with raster_numpy standing in for the CUDA
extension only; here a numpy restatement of those wrappers must reproduce the tensors that reached the stand-in bit for
bit, and raster_numpy must reproduce the recorded images from them.  render_dp is not in G29 (the reference's nnutils/moda.py
cannot be imported without torchvision and pytorch3d); the GPU tests check its stated properties instead.
Last, the presence of the rasteriser entries in the header, the binding and the built library, and their shape refusals."""
import os
import re

import numpy as np

import raster_numpy as rn
from helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("moda_raster_fwd", "moda_raster_interp")


def lattice(i, S):
    """NDC coordinate of pixel-corner lattice line i (0 .. S): pixel centres lie half a pixel off every such line."""
    return 2.0 * i / S - 1.0


def test_lattice_triangle_cover_and_identity():
    S = 16
    # right triangle with corners on the lattice points (2,3), (12,3), (2,8), in pixels from the bottom left
    tri = np.array([[lattice(2, S), lattice(3, S), 2.0], [lattice(12, S), lattice(3, S), 2.0], [lattice(2, S), lattice(8, S), 2.0]])
    xs, ys = rn.pixel_centres(S)
    for order in ([0, 1, 2], [2, 1, 0]):                                      # both windings
        r = rn.rasterize(tri[order][None], S)
        # closed form: centre (c + .5, j + .5) in pixels (j counted from the bottom) is inside iff c >= 2, j >= 3 and
        # (c + .5 - 2) / 10 + (j + .5 - 3) / 5 < 1, i.e. c + 2 j < 16.5: no centre lies on an edge
        want = np.zeros((S, S), bool)
        for row in range(S):
            j = S - 1 - row
            for c in range(S):
                want[row, c] = c >= 2 and j >= 3 and c + 2 * j < 16.5
        assert want.sum() == 25
        assert np.array_equal(r.alpha, want) and np.array_equal(r.face_idx >= 0, want)
        assert np.abs(r.zbuf[want] - 2.0).max() <= 1e-12
        # attribute = vertex position: the rendered value is the pixel's own (xp, yp), the identity render_flow relies on
        img = rn.interpolate(tri[order][None][..., :2], r)
        assert np.abs(img[0][want] - np.broadcast_to(xs[None, :], (S, S))[want]).max() <= 1e-12
        assert np.abs(img[1][want] - np.broadcast_to(ys[:, None], (S, S))[want]).max() <= 1e-12
        assert (img[:, ~want] == 0).all()
        assert r.edge_margin[want].min() >= 0.5 / 10 - 1e-12                 # half a pixel over the 10-pixel leg


def _quad(S, i0, i1, z):
    """Two triangles covering lattice square [i0, i1]^2 at depth z -> (2,3,3)."""
    a, b = lattice(i0, S), lattice(i1, S)
    return np.array([[[a, a, z], [b, a, z], [b, b, z]], [[a, a, z], [b, b, z], [a, b, z]]])


def test_nearer_face_wins_for_both_windings_and_orders():
    S = 8
    # corners (1,1), (7,1), (1,4) in pixels: centre (c + .5, j + .5) is inside iff c, j >= 1 and c + 2 j < 7.5 -- 9 pixels, none on an edge
    near_tri = np.array([[lattice(1, S), lattice(1, S), 2.0], [lattice(7, S), lattice(1, S), 2.0], [lattice(1, S), lattice(4, S), 2.0]])
    far_tri = near_tri.copy()
    far_tri[:, 2] = 3.0
    for a, b, want_idx in ((near_tri, far_tri, 0), (far_tri, near_tri, 1), (near_tri[::-1], far_tri, 0), (far_tri, near_tri[::-1], 1)):
        r = rn.rasterize(np.stack([a, b]), S)
        hit = r.alpha
        assert hit.sum() == 9 and (r.face_idx[hit] == want_idx).all() and np.abs(r.zbuf[hit] - 2.0).max() <= 1e-12
        assert np.abs(r.depth_margin[hit] - 0.5).max() <= 1e-12


def test_equal_depth_keeps_the_lower_index():
    S = 8
    tri = np.array([[lattice(1, S), lattice(1, S), 2.0], [lattice(7, S), lattice(1, S), 2.0], [lattice(1, S), lattice(7, S), 2.0]])
    r = rn.rasterize(np.stack([tri, tri, tri[::-1]]), S)
    assert (r.face_idx[r.alpha] == 0).all() and (r.depth_margin[r.alpha] == 0).all()


def test_depth_range_leaves_colour_but_sets_alpha():
    S = 8
    for z in (0.5, 150.0):                                                    # before near = 1, beyond far = 100
        q = _quad(S, 2, 6, z)
        img, r = rn.render(q, np.ones((2, 3, 3)), S, background=(0.25, 0.5, 0.75))
        assert r.alpha.sum() == 16 and (r.face_idx == -1).all() and (r.zbuf == 0).all()
        assert (img[0] == 0.25).all() and (img[1] == 0.5).all() and (img[2] == 0.75).all()
        assert np.array_equal(img[3], r.alpha.astype(float))
    # a face in range behind one out of range is drawn
    img, r = rn.render(np.concatenate([_quad(S, 2, 6, 0.5), _quad(S, 2, 6, 5.0)]), np.ones((4, 3, 3)), S)
    assert (r.face_idx[r.alpha] >= 2).all() and (img[0][r.alpha] == 1).all()


def test_depth_is_perspective_correct():
    S = 32
    tri = np.array([[lattice(2, S), lattice(2, S), 2.0], [lattice(30, S), lattice(2, S), 4.0], [lattice(2, S), lattice(30, S), 8.0]])
    r = rn.rasterize(tri[None], S)
    xs, ys = rn.pixel_centres(S)
    X, Y = np.meshgrid(xs, ys)
    e = lattice(30, S) - lattice(2, S)
    w1, w2 = (X - lattice(2, S)) / e, (Y - lattice(2, S)) / e
    want = 1.0 / ((1 - w1 - w2) / 2.0 + w1 / 4.0 + w2 / 8.0)
    assert r.alpha.sum() > 300 and np.abs(r.zbuf[r.alpha] - want[r.alpha]).max() <= 1e-12


def test_zero_area_face_draws_nothing():
    S = 8
    flat = np.array([[lattice(1, S), lattice(1, S), 2.0], [lattice(4, S), lattice(4, S), 2.0], [lattice(7, S), lattice(7, S), 2.0]])
    point = np.tile(np.array([[0.125, 0.125, 2.0]]), (3, 1))                  # a pixel centre of S = 8, three times
    for face in (flat, point):
        img, r = rn.render(face[None], np.ones((1, 3, 3)), S)
        assert np.isfinite(img).all() and (img == 0).all() and (r.face_idx == -1).all() and not r.alpha.any()
        assert np.isfinite(r.bary).all() and np.isfinite(r.zbuf).all()


# ---- the scenes of the GPU order tests (tests/test_gpu_mesh_render.py imports these), held here on the oracle alone ----------
REPLICA_SCENES = {"icosphere4": (41, 42, 43), "icosphere2": (44, 45)}         # name -> view seeds; F = 5120 and 320
REPLICA_SIZES = (64, 257)
CHUNK_FACES = (255, 256, 257, 511, 512, 513, 769)                             # around multiples of the kernel's 256-face chunk
CHUNK_SEEDS = (50, 56)                                                        # views in which the last face of each list is drawn


def replica_scene(name):
    return rn.icosphere(int(name[-1]), 0.9)


def _mc_scene(n=32):
    """The marching-cubes scene of tests/test_gpu_mesh_render.py, from the numpy marching cubes."""
    import mc_numpy as mcn
    v, f, _ = mcn.marching_cubes(rn.sphere_volume(n), 0.0)
    assert len(f) > 3000
    return (v - (n - 1) / 2) / (0.5 * n) * 0.8, f


def test_replicated_faces_keep_the_lowest_copy():
    """A face list that holds every face several times draws the image of the single list, face i under the index of its lowest
    copy, exactly: the copies tie at every pixel and only a strictly nearer face replaces the one that holds it."""
    scenes = [(name, replica_scene(name), seeds[:1 if name == "icosphere4" else 2]) for name, seeds in sorted(REPLICA_SCENES.items())]
    scenes.append(("marching cubes", _mc_scene(), (12,)))
    for name, (v, f), seeds in scenes:
        for S in REPLICA_SIZES:
            for verts in rn.views(v, seeds):
                one = rn.rasterize(verts[f], S)
                drawn = one.face_idx >= 0
                assert drawn.sum() > 0.2 * S * S
                for kind, faces, lowest in rn.replicas(f):
                    r = rn.rasterize(verts[faces], S)
                    assert np.array_equal(r.face_idx, np.where(drawn, lowest[np.where(drawn, one.face_idx, 0)], -1)), (name, S, kind)
                    assert np.array_equal(r.bary, one.bary) and np.array_equal(r.zbuf, one.zbuf) and np.array_equal(r.alpha, one.alpha)
                    assert (r.depth_margin[drawn] == 0).all()                 # which is why check_against_oracle cannot be used on them


def test_chunk_boundary_scenes_satisfy_the_left_out_cap():
    """The condition tests/test_gpu_mesh_render.py puts on a scene (at most 1 % of the covered pixels inside the margins),
    checked on the oracle alone for the first F faces of icosphere 4."""
    v, f = rn.icosphere(4, 0.9)
    for F in CHUNK_FACES:
        last_drawn = 0
        for b, verts in enumerate(rn.views(v, CHUNK_SEEDS)):
            r = rn.rasterize(verts[f[:F]], 64)
            ok = (r.edge_margin > 1e-4) & (r.depth_margin > 1e-5)
            covered, left = int(r.alpha.sum()), int((r.alpha & ~ok).sum())
            print(f"F {F} view {b}: covered {covered}, left out {left}, faces drawn {len(np.unique(r.face_idx)) - 1}, "
                  f"highest {r.face_idx[ok].max()}")
            assert covered >= 30 and left <= 0.01 * covered
            last_drawn += int((r.face_idx[ok] == F - 1).sum())
        assert last_drawn > 0                                                 # the last face of the last chunk is compared


def wrap_render_color(verts, faces, colors, eye):
    """numpy fp32 restatement of what render_color (geom_utils.py:690-693), look_at (functional/look_at.py:59) with its identity
    axes, orthogonal (scale 1), the ambient-only lighting and face_vertices do before the kernel."""
    eye = np.asarray(eye, np.float32)
    v = (verts.astype(np.float32) - eye[None, None])
    v[:, :, 1] = -1 * v[:, :, 1]
    v = v - eye[None, None]
    idx = faces.astype(np.int64)
    fv = np.stack([v[b][idx] for b in range(len(v))])
    ft = np.stack([(colors[b].astype(np.float32) * np.float32(1.0))[idx] for b in range(len(v))])
    return fv, ft


def test_oracle_through_the_wrappers_reproduces_g29():
    g = golden("g29_mesh_render")
    S, eye = int(g["image_size"]), g["eye"]
    assert abs(eye[2] + (1.0 / np.tan(np.radians(30.0)) + 1.0)) <= 1e-12 and eye[0] == 0 and eye[1] == 0
    for name in list(g["cases"]) + ["flow"]:
        verts, faces = g[f"{name}_verts"], g[f"{name}_faces"]
        colors = g[f"{name}_colors"] if name != "flow" else g["flow_verts_n"]
        fv, ft = wrap_render_color(verts, faces, colors, eye)
        assert fv.dtype == np.float32 and np.array_equal(fv, g[f"{name}_face_vertices"])
        assert np.array_equal(ft, g[f"{name}_face_textures"])
        assert np.all(np.abs(fv[..., 2] - (verts[:, faces, 2] + 2 * (1.0 / np.tan(np.radians(30.0)) + 1.0))) <= 1e-5)
        imgs = np.stack([rn.render(fv[b], ft[b], S)[0] for b in range(len(fv))])
        if name != "flow":
            want = g[f"{name}_rendered"]
            assert want.shape == (len(verts), 4, S, S)
            assert np.array_equal(imgs[:, 3] > 0, want[:, 3] > 0) and set(np.unique(want[:, 3])) <= {0.0, 1.0}
            assert np.abs(imgs.astype(np.float32) - want).max() <= 1e-12
        else:
            want = g["flow_rendered"]
            assert want.shape == (len(verts), S, S, 3)
            grid = np.arange(S, dtype=np.float32) * 2 / (S - 1) - 1           # geom_utils.py:713-716
            flow = np.zeros_like(want)
            flow[..., 0] = imgs[:, 0].astype(np.float32) - grid[None, None, :]
            flow[..., 1] = imgs[:, 1].astype(np.float32) - grid[None, :, None]
            flow[imgs[:, 3] < 1] = 0
            assert np.array_equal(flow != 0, want != 0) and np.abs(flow - want).max() <= 1e-12
            assert (want[..., 2] == 0).all()
    # scene b: its third view is fully off-screen and must be empty
    assert (g["b_rendered"][2] == 0).all() and (g["b_rendered"][1, 3] > 0).any()


def test_cameras_match_g29():
    g = golden("g29_mesh_render")
    v, R, T, K = (g[k].astype(np.float64) for k in ("cam_verts", "cam_R", "cam_T", "cam_K"))
    cam = v @ np.swapaxes(R, 1, 2) + T[:, None]
    assert np.abs(cam - g["cam_obj_to_cam"]).max() <= 1e-5
    c = g["cam_obj_to_cam"].astype(np.float64)
    x = (K[:, None, 0] * c[..., 0] + K[:, None, 2] * c[..., 2]) / (1e-6 + c[..., 2])
    y = (K[:, None, 1] * c[..., 1] + K[:, None, 3] * c[..., 2]) / (1e-6 + c[..., 2])
    assert np.abs(np.stack([x, y, c[..., 2]], -1) - g["cam_pinhole"]).max() <= 1e-5


def test_axis_angle_to_matrix_is_the_rotation():
    """render_dp's rotations (the pose-CNN's training target) come from a restatement of pytorch3d's axis_angle_to_matrix: held
    here to a float64 Rodrigues formula and to torch.matrix_exp of the skew matrix, on render_dp's own draws, at angles
    below the series switch (1e-6) and around it."""
    import torch
    from moda_amd.mesh_render import axis_angle_to_matrix
    np.random.seed(11)
    np.random.normal(0, 0.5, 16)
    a = np.random.normal(0, 6.28, (16, 3))
    tiny = np.array([[0, 0, 0], [3e-7, 0, 0], [0, -5e-7, 2e-7], [9.9e-7, 0, 0], [1.1e-6, 0, 0], [1e-3, -2e-3, 5e-4]])
    a = np.concatenate([a, tiny])
    want = []
    for v in a:
        K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
        t = np.linalg.norm(v)
        want.append(np.eye(3) + (np.sin(t) / t if t > 0 else 1.0) * K + ((1 - np.cos(t)) / t ** 2 if t > 0 else 0.5) * K @ K)
    want = np.stack(want)
    got64 = axis_angle_to_matrix(torch.as_tensor(a)).numpy()
    assert np.abs(got64 - want).max() <= 1e-13
    K = torch.zeros((len(a), 3, 3), dtype=torch.float64)
    ta = torch.as_tensor(a)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ta[:, 2], ta[:, 1], ta[:, 2], -ta[:, 0], -ta[:, 1], ta[:, 0]
    assert np.abs(got64 - torch.matrix_exp(K).numpy()).max() <= 1e-12
    assert np.abs(got64 @ np.swapaxes(got64, 1, 2) - np.eye(3)).max() <= 1e-13 and np.abs(np.linalg.det(got64) - 1).max() <= 1e-13
    got32 = axis_angle_to_matrix(torch.as_tensor(a, dtype=torch.float32)).numpy()
    # fp32: the angle t carries 2 u t of rounding, the half-angle's sine and cosine u t + 2 u, an entry is twice a sum of two
    # products of them: 4 (t + 3) u
    t = np.linalg.norm(a, axis=1)
    assert got32.dtype == np.float32 and (np.abs(got32 - want).max((1, 2)) <= 4 * (t + 3) * 2.0 ** -24).all()
    # a rotation about z by +90 degrees takes x to y: not the transpose
    r = axis_angle_to_matrix(torch.tensor([[0.0, 0.0, np.pi / 2]], dtype=torch.float64))[0].numpy()
    assert np.abs(r @ [1, 0, 0] - [0, 1, 0]).max() <= 1e-15


def test_resized_crop_is_half_pixel_bilinear_with_zero_padding():
    """torchvision's resized_crop for tensors, restated in mesh_render.py, against a direct numpy evaluation: output pixel i
    samples the crop at (i + 0.5) * n_in / n_out - 0.5, clamped at the crop's border, linear weights; the part of the window
    that leaves the image reads as zero."""
    import torch
    from moda_amd.mesh_render import resized_crop
    rng = np.random.default_rng(4)
    img = rng.standard_normal((3, 20, 24))
    for top, left, h, w, size in ((2, 3, 10, 14, (50, 50)), (-3, 18, 12, 10, (7, 5)), (5, 5, 1, 1, (4, 4)), (15, -2, 9, 30, (50, 50))):
        crop = np.zeros((3, h, w))
        for r in range(h):
            for c in range(w):
                if 0 <= top + r < 20 and 0 <= left + c < 24:
                    crop[:, r, c] = img[:, top + r, left + c]

        def taps(n_in, n_out):
            x = np.maximum((np.arange(n_out) + 0.5) * n_in / n_out - 0.5, 0.0)
            i0 = np.minimum(np.floor(x).astype(int), n_in - 1)
            return i0, np.minimum(i0 + 1, n_in - 1), x - i0
        r0, r1, fr = taps(h, size[0])
        c0, c1, fc = taps(w, size[1])
        rows = crop[:, r0] * (1 - fr)[None, :, None] + crop[:, r1] * fr[None, :, None]
        want = rows[:, :, c0] * (1 - fc) + rows[:, :, c1] * fc
        got = resized_crop(torch.as_tensor(img), top, left, h, w, size).numpy()
        assert got.shape == (3,) + size and np.abs(got - want).max() <= 1e-12


def test_raster_entries_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "moda_hip.h")).read()
    declared = set(re.findall(r"\b(moda_[a-z0-9_]+)\s*\(", hdr))
    from moda_amd import _lib, build
    assert "raster_kernels.hip" in build.SOURCES
    build.build(verbose=False)
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in include/moda_hip.h"
        assert name in _lib.EXPORTS, f"{name} is not bound in moda_amd/_lib.py"
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert lib.moda_abi_version() == _lib.ABI_VERSION == 11

    # shape refusals need no device: they come before any pointer is looked at
    def fwd(B, V, F, S):
        return lib.moda_raster_fwd(None, None, 0, B, V, F, S, 1.0, 100.0, 1, None, None, None, None, None, None, None)

    def interp(B, V, F, C, S):
        return lib.moda_raster_interp(None, None, 0, None, None, None, B, V, F, C, S, None, None)
    assert fwd(1, 3, 1, 0) == -2 and fwd(1, 3, 0, 16) == -2 and fwd(0, 3, 1, 16) == -2 and fwd(1, 0, 1, 16) == -2
    assert fwd(2 ** 20, 3, 1, 64) == -2                                       # B*S*S >= 2^31
    assert fwd(4, 3, 2 ** 29, 16) == -2                                       # B*F >= 2^31
    assert fwd(1, 3, 1, 2 ** 16) == -2
    assert fwd(1, 3, 1, 16) == -1                                             # shape accepted, null pointers refused
    assert interp(1, 3, 1, 0, 16) == -2 and interp(1, 3, 1, 3, 0) == -2 and interp(1, 3, 0, 3, 16) == -2
    assert interp(2 ** 20, 3, 1, 3, 64) == -2 and interp(1, 3, 1, 3, 16) == -1
