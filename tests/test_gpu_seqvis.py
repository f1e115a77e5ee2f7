"""GPU (-m gpu): mesh sequence rendering (moda_amd/seq_render.py, csrc/seqvis_kernels.hip) stage by stage against the float64
restatement tests/seqvis_numpy.py (pinned where it can be by tests/test_seqvis_oracle.py), then the chain, its chunking, graph
capture, the error colours and the refusals.  The rasteriser between the stages is taken as given: it has tests of its own."""
import numpy as np
import pytest
import torch

import seqvis_numpy as sn
from test_seqvis_oracle import NEAR_CAP, OPACITIES, RESIZE_CASES, SHADE_SIZES, resize_case, shade_case

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import moda_amd
    from gpu_helpers import DEV
    from moda_amd import seq_render as SR
    from moda_amd.plasma_table import PLASMA

FIELDS = ("color", "depth", "sil", "frames", "refsil", "ctrajs", "cams", "status")


def np_(t):
    return t.detach().cpu().numpy()


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.uint8) == b.view(torch.uint8)).all())


def rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))[None]
    q[:, 0] *= np.linalg.det(q)
    return q


def random_cams(rng, F, identity=False):
    out = np.zeros((F, 4, 4), np.float32)
    for i in range(F):
        out[i] = sn.camera(None if identity else rotation(rng), rng.uniform(-0.5, 0.5, 3) + (0, 0, 3.0),
                           (40 + rng.uniform(), 38 + rng.uniform(), 24 + rng.uniform(), 20 + rng.uniform()))
    return out


def sphere_sequence(F=3, S=48, bones=True, seed=0):
    """An icosphere (42 vertices, 80 faces) breathing over F frames in front of slowly turning cameras, with two bone ellipsoids
    inside and outside it -> (MeshSequence, host arrays)."""
    rng = np.random.default_rng(seed)
    v, f = sn.icosphere(1)
    verts = np.stack([v * (0.8 + 0.05 * i) + 0.02 * rng.standard_normal(v.shape) for i in range(F)]).astype(np.float32)
    colors = rng.integers(0, 256, (len(v), 3)).astype(np.uint8)
    rtk = np.zeros((F, 4, 4), np.float32)
    for i in range(F):
        rtk[i] = sn.camera(sn.rodrigues([0.1 * i, 0.2 + 0.1 * i, 0.05]), (0.05 * i, -0.03, 3.0 + 0.1 * i), (40.0, 41.0, S / 2 + 0.3, S / 2 - 0.2))
    b = np.zeros((F, 2, 10), np.float32)
    b[:, :, 3] = 1.0
    b[:, 0, :3], b[:, 1, :3] = (0.0, 0.0, -1.2), (0.9, 0.5, 0.0)
    bone_mesh = moda_amd.bone_ellipsoids(dev(b), 6.0)
    rest = moda_amd.bone_ellipsoids(dev(b[:1]), 6.0)
    seq = moda_amd.MeshSequence(dev(verts), dev(f, torch.int32), dev(colors), dev(b), bone_mesh, None, dev(rtk), dev(verts[0] * 1.1),
                                dev(colors), rest)
    return seq, {"verts": verts, "faces": f, "colors": colors, "rtk": rtk}


# ---- view cameras ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 65])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 257])
def test_view_cameras_every_mode_within_one_ulp(F, V):
    rng = np.random.default_rng(100 * F + V)
    verts = (rng.standard_normal((F, V, 3)) + (0.3, -0.2, 0.1)).astype(np.float32)
    worst = 0.0
    for identity in (False, True):
        rtk = random_cams(rng, F, identity)
        for vp in (0, 1, 2, -1, -2):
            for turntable in (False, True):
                v = verts[:1] if turntable else verts
                cams, ctrajs = SR.view_cameras(dev(rtk), dev(v), (37, 48), vp, turntable, 20)
                want, want_c = sn.view_cameras(rtk, v, (37, 48), vp, turntable, 20)
                d = max(sn.ulp_diff(np_(cams), want).max(), sn.ulp_diff(np_(ctrajs), want_c).max())
                worst = max(worst, d)
                assert d <= 1.0, (identity, vp, turntable, d)
    print("view cameras, worst fp32 ulp", worst)


# ---- projection and culling ----------------------------------------------------------------------------------------------------------
def project_on_device(verts, cams, faces, S):
    n, V, Nf = len(cams), verts.shape[1], len(faces)
    cam = torch.empty((n, V, 3), device=DEV)
    ndc = torch.empty((n, V, 3), device=DEV)
    vf = torch.empty((n, Nf, 3), dtype=torch.int32, device=DEV)
    status = torch.zeros(SR.STATUS_WORDS, dtype=torch.int32, device=DEV)
    v_t, c_t, f_t = dev(verts), dev(cams), dev(faces, torch.int32)                    # held: a temporary's memory is reused at once
    SR.L.call("moda_seqvis_project", SR.L.ptr(v_t), SR.L.ptr(c_t), SR.L.ptr(f_t), n, len(verts), V, Nf, S,
              SR.L.ptr(cam), SR.L.ptr(ndc), SR.L.ptr(vf), SR.L.ptr(status), SR.L.stream())
    return cam, ndc, vf, status


@pytest.mark.parametrize("V", [7, 300])
def test_projection_and_culling(V):
    """A face straddling Z = 0, one entirely behind, a vertex exactly at Z = 0, an index outside [0, V); V = 300 takes two
    workgroups of vertices.  The dropped set is exact, the coordinates lie within the restatement's running fp32 bound."""
    rng = np.random.default_rng(V)
    verts = rng.uniform(-1, 1, (2, V, 3)).astype(np.float32)
    verts[:, 0] = (0.5, 0.5, -3.0)               # exactly at Z = 0 under t_z = 3 and an identity rotation
    verts[:, 1] = (0.1, 0.2, -4.0)               # behind
    verts[:, 2] = (0.3, -0.2, -5.0)
    verts[:, 3] = (-0.2, 0.1, -3.5)
    faces = np.array([[4, 5, 6], [1, 5, 6], [1, 2, 3], [0, 4, 5], [4, 5, V], [-1, 4, 5], [6, 5, 4]] +
                     [list(rng.integers(0, V, 3)) for _ in range(290)], np.int64)
    cams = np.stack([sn.camera(None, (0, 0, 3.0), (40, 40, 24, 24)), sn.camera(sn.rodrigues([0.01, 0.3, 0]), (0.1, 0, 3.0), (40, 39, 24, 20))])
    cam, ndc, vf, status = project_on_device(verts, cams, faces, 48)
    dropped = bad = 0
    for i in range(2):
        r = sn.project(verts[i], cams[i], faces, 48)
        assert np.array_equal(np_(vf[i]), r["view_faces"])
        dropped, bad = dropped + int(r["dropped"].sum()), bad + int(r["bad_index"].sum())
        assert np.all(np.abs(np_(cam[i]) - r["cam"]) <= r["cam_bound"])
        assert np.all(np.abs(np_(ndc[i]) - r["ndc"]) <= r["ndc_bound"])
        assert np.array_equal(np_(ndc[i, :, 2]), np_(cam[i, :, 2])) and np.array_equal(np_(cam[i, :, 2]), r["z32"])
        if i == 0:
            assert r["z32"][0] == 0.0 and r["dropped"][1] and r["dropped"][2] and r["dropped"][3] and not r["dropped"][0]
            assert r["bad_index"][4] and r["bad_index"][5] and abs(np_(ndc[0, 0, 0])) > 1e9
    st = np_(status)
    assert st[SR.DROPPED] == dropped and dropped >= 3 and st[SR.BAD_INDEX] == bad == 4 and st[SR.NONFINITE] == 0
    verts[1, 5, 0] = np.nan
    st = np_(project_on_device(verts, cams, faces, 48)[3])
    assert st[SR.NONFINITE] == 1


# ---- normals -----------------------------------------------------------------------------------------------------------------------
def records_on_device(cam, view_faces, faces, colors=None, error=None):
    n, V, Nf = cam.shape[0], cam.shape[1], view_faces.shape[1]
    csr = SR.vertex_csr(dev(faces, torch.int32), V)
    rec = torch.empty((n, V, SR.REC_FLOATS), device=DEV)
    status = torch.zeros(SR.STATUS_WORDS, dtype=torch.int32, device=DEV)
    table = dev(np.asarray(PLASMA, np.float32))
    mode = 2 if error is not None else (0 if colors is not None else 1)
    cam_t, vf_t = dev(cam), dev(view_faces, torch.int32)                              # held: a temporary's memory is reused at once
    col_t, err_t = None if colors is None else dev(colors), None if error is None else dev(error)
    SR.L.call("moda_seqvis_records", SR.L.ptr(cam_t), SR.L.ptr(vf_t), SR.L.ptr(csr[0]), SR.L.ptr(csr[1]), n, V, Nf,
              mode, SR.L.ptr(col_t), 1 if colors is None or colors.ndim == 2 else n, 76.0,
              SR.L.ptr(err_t), SR.L.ptr(table), SR.L.ptr(rec), SR.L.ptr(status), SR.L.stream())
    return rec, status


def normal_meshes():
    ico_v, ico_f = sn.icosphere(1)
    fan_v, fan_f = sn.fan(70)
    tri_v = np.array([[0, 0, 0], [1, 0.1, 0], [0.2, 1, 0.3], [5, 5, 5]], np.float64)            # vertex 3 belongs to no face
    tri_f = np.array([[0, 1, 2]])
    flat_v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0.5], [1, 1, 1]], np.float64)
    flat_f = np.array([[0, 1, 2], [0, 1, 3], [1, 4, 3]])                                        # the first has zero area
    return {"triangle": (tri_v, tri_f), "icosphere": (ico_v * 0.9 + (0, 0, 3), ico_f), "fan": (fan_v, fan_f), "zero_area": (flat_v, flat_f)}


@pytest.mark.parametrize("name", ["triangle", "icosphere", "fan", "zero_area"])
def test_normals_against_float64_and_bitwise_repeatable(name):
    v, f = normal_meshes()[name]
    v = v.astype(np.float32)
    cam = np.stack([v, v * (-1, 1, 1), v * 1.3 + 0.1]).astype(np.float32)                      # frame 1 mirrors frame 0
    vf = np.tile(f[None], (3, 1, 1))
    rec, _ = records_on_device(cam, vf, f)
    rec2, _ = records_on_device(cam, vf, f)
    assert same_bits(rec, rec2)
    for i in range(3):
        alone, _ = records_on_device(cam[i:i + 1], vf[i:i + 1], f)
        assert same_bits(alone[0], rec[i])
        want, bound = sn.vertex_normals(cam[i], vf[i])
        got = np_(rec[i, :, 3:6])
        assert np.all(np.abs(got - want) <= bound + 1e-30), (i, np.abs(got - want).max())
    assert np.all(np_(rec[:, :, :3]) == 76.0) and np.all(np_(rec[:, :, 6:]) == 0.0)
    n0, n1 = np_(rec[0, :, 3:6]), np_(rec[1, :, 3:6])
    # the mirror image: the cross products change sign in y and z, bit for bit
    assert np.array_equal(n1[:, 0], n0[:, 0]) and np.array_equal(n1[:, 1], -n0[:, 1]) and np.array_equal(n1[:, 2], -n0[:, 2])
    if name == "triangle":
        assert np.all(np_(rec[:, 3, 3:6]) == 0.0)
    # a face the view dropped does not contribute
    vf2 = vf.copy()
    vf2[:, 0] = -1
    want, bound = sn.vertex_normals(cam[0], vf2[0])
    assert np.all(np.abs(np_(records_on_device(cam, vf2, f)[0][0, :, 3:6]) - want) <= bound + 1e-30)


# ---- shading, compositing, overlay, crop ---------------------------------------------------------------------------------------------
def shade_on_device(c, H, W, smooth, opacity, bone=True, overlay=False):
    S = c["S"]
    layer = lambda l: tuple(dev(t)[None] if k in (0, 1, 2, 4, 5) else dev(t) for k, t in enumerate(l))
    color = torch.empty((1, H, W, 3), dtype=torch.uint8, device=DEV)
    depth = torch.empty((1, H, W), device=DEV)
    sil = torch.empty((1, H, W), dtype=torch.int16, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    SR.shade(layer(c["body"]), layer(c["bone"]) if bone else None, 1, S, H, W, smooth, opacity, dev(c["overlay"])[None] if overlay else None,
             color, depth, sil, count)
    return np_(color[0]), np_(depth[0]), np_(sil[0]), int(count)


def check_8bit(got, want, near, what, cap=NEAR_CAP):
    """Equal outside `near`, within 1 inside it; `near` holds under `cap` of the pixels (None: the inputs were not chosen, as
    the chain's resize of its own frames, where the weights 0.5 of the scale 48 / 20 put many sums on an exact half)."""
    d = np.abs(got.astype(np.int64) - want.astype(np.int64)).reshape(near.shape + (-1,)).max(-1)
    assert cap is None or near.mean() < cap, (what, near.mean())
    assert np.all(d[~near] == 0) and np.all(d <= 1), (what, int((d[~near] != 0).sum()), int(d.max()))


@pytest.mark.parametrize("H,W", SHADE_SIZES)
def test_shading_compositing_overlay_and_crop(H, W):
    c = shade_case(H, W)
    for smooth in (True, False):
        for op in OPACITIES:
            for bone, overlay in ((True, False), (True, True), (False, True), (False, False)):
                if not bone and op != OPACITIES[0]:
                    continue
                color, depth, sil, count = shade_on_device(c, H, W, smooth, op, bone, overlay)
                r = sn.shade(c["body"], c["bone"] if bone else None, H, W, smooth, op, c["overlay"] if overlay else None)
                check_8bit(color, r["color"], r["near"], (smooth, op, bone, overlay))
                assert np.array_equal(depth, r["depth"].astype(np.float32)) and np.array_equal(sil, r["sil"])
                assert np.all(color[0, 0] == 0) and set(np.unique(sil)) <= {0, 100} and count == int((sil > 0).sum())


# ---- resize ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,ow", RESIZE_CASES)
def test_resize(H, W, ow):
    color, sil = resize_case(H, W)
    h = int(H * ow / W)
    status = torch.zeros(SR.STATUS_WORDS, dtype=torch.int32, device=DEV)
    frames, refsil = SR.resize(dev(color)[None], dev(sil)[None], dev(np.array([0, ], np.int32)), h, ow, status)
    want, near = sn.resize(color, h, ow)
    want_s, near_s = sn.resize(sil, h, ow)
    check_8bit(np_(frames[0]), want, near, "frames")
    check_8bit(np_(refsil[0]), want_s, near_s, "refsil")
    assert np_(status)[SR.EMPTY] == 1                                                 # the count handed in was 0


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
_CHAIN = {}


def chain_sequence():
    if "seq" not in _CHAIN:
        _CHAIN["seq"] = sphere_sequence(3, 48)
    return _CHAIN["seq"]


@pytest.mark.parametrize("mode", ["vp0", "vp1", "vp2", "vp-1", "vp-2", "freeze"])
def test_chain_equals_the_stage_restatements_on_its_own_intermediates(mode):
    seq, host = chain_sequence()
    S, H, W, F = 48, 40, 48, 3
    vp, freeze = (0, True) if mode == "freeze" else (int(mode[2:]), False)
    bones = mode in ("vp-1", "freeze")
    overlay = np.random.default_rng(5).integers(0, 256, (F, H, W, 3)).astype(np.uint8)
    out = seq.render((H, W), vp=vp, freeze=freeze, bones=bones, mesh_opacity=0.5, overlay=dev(overlay), out_width=20)
    v = host["verts"][:1] if freeze else host["verts"]
    want_cams, want_ctrajs = sn.view_cameras(host["rtk"], v, (H, W), vp, freeze, 20)
    assert sn.ulp_diff(np_(out.cams), want_cams).max() <= 1 and sn.ulp_diff(np_(out.ctrajs), want_ctrajs).max() <= 1
    # the stages by hand on the device, every intermediate kept
    status = torch.zeros(SR.STATUS_WORDS, dtype=torch.int32, device=DEV)
    layers = [SR._Layer(dev(v), seq.faces, seq.colors, SR.vertex_csr(seq.faces, v.shape[1]), F, S, DEV)]
    if bones:
        bv = seq.bone_mesh[0][:1] if freeze else seq.bone_mesh[0]
        layers.append(SR._Layer(bv, seq.bone_mesh[1], seq.bone_mesh[2], SR.vertex_csr(seq.bone_mesh[1], bv.shape[1]), F, S, DEV))
    for l in layers:
        l.run(0, F, out.cams, S, 1e-3, 1000.0, 0, 0.0, None, None, status)
    cams = np_(out.cams)
    near_total = 0
    for i in range(F):
        planes = []
        for l in layers:
            lv = np_(l.verts)[0 if l.verts.shape[0] == 1 else i]
            r = sn.project(lv, cams[i], np_(l.faces), S)
            assert np.array_equal(np_(l.view_faces[i]), r["view_faces"])
            assert np.all(np.abs(np_(l.ndc[i]) - r["ndc"]) <= r["ndc_bound"])
            n, bound = sn.vertex_normals(np_(l.cam[i]), np_(l.view_faces[i]))
            assert np.all(np.abs(np_(l.rec[i, :, 3:6]) - n) <= bound + 1e-30)
            assert np.array_equal(np_(l.rec[i, :, :3]), sn.base_u8(np_(l.colors)))
            planes.append(tuple(np_(t) for t in (l.face_idx[i], l.bary[i], l.zbuf[i], l.faces, l.rec[i], l.cam[i])))
        r = sn.shade(planes[0], planes[1] if bones else None, H, W, True, 0.5, overlay[i])
        check_8bit(np_(out.color[i]), r["color"], r["near"], (mode, i))
        assert np.array_equal(np_(out.depth[i]), r["depth"].astype(np.float32)) and np.array_equal(np_(out.sil[i]), r["sil"])
        want, near = sn.resize(np_(out.color[i]), 16, 20)
        want_s, near_s = sn.resize(np_(out.sil[i]), 16, 20)
        check_8bit(np_(out.frames[i]), want, near, (mode, i, "frames"), cap=None)
        check_8bit(np_(out.refsil[i]), want_s, near_s, (mode, i, "refsil"), cap=None)
        assert (np_(out.sil[i]) > 0).any()
    assert not np_(out.status).any() and not np_(status).any() and tuple(out.frames.shape) == (F, 16, 20, 3)


def test_chain_against_render_mesh_at_vp0():
    seq, host = chain_sequence()
    S, F = 48, 3
    out = seq.render((S, S), vp=0, out_width=24)
    assert same_bits(out.cams, seq.rtk)
    for i in range(F):
        color, depth, sil = moda_amd.render_mesh(seq.frame(i), seq.rtk[i], S)
        r = sn.project(host["verts"][i], host["rtk"][i], host["faces"], S)
        band = sn.edge_band(r["ndc"], r["view_faces"], S, S, S)
        got_sil, ref_sil = np_(out.sil[i]) > 0, np_(sil)
        assert band.sum() <= 0.02 * max(ref_sil.sum(), 1)
        assert np.array_equal(got_sil[~band], ref_sil[~band])
        ok = ~band & ref_sil
        d, rd = np_(out.depth[i])[ok], np_(depth)[ok]
        assert np.all(np.abs(d - rd) <= 1e-5 * np.abs(rd))
        dc = np.abs(np_(out.color[i]).astype(int) - np_(color).astype(int))[~band]
        assert dc.max() <= 1


def test_chunk_boundaries_change_no_bit():
    seq, _ = chain_sequence()
    S, H, W = 48, 40, 48
    sizes = [(42, 80), (int(seq.bone_mesh[0].shape[1]), int(seq.bone_mesh[1].shape[0]))]
    unit = sum(Nf * (12 + 96 + 16) + V * 56 + 24 * S * S for V, Nf in sizes)
    assert [SR.frames_per_chunk(k * unit, S, sizes) for k in (1, 2, 3)] == [1, 2, 3]
    outs = [seq.render((H, W), vp=1, bones=True, mesh_opacity=0.5, out_width=20, budget_bytes=k * unit) for k in (1, 2, 3)]
    for o in outs[1:]:
        for k in FIELDS:
            assert same_bits(getattr(o, k), getattr(outs[0], k)), k


def test_capture_and_replay_follow_the_vertices():
    seq, host = sphere_sequence(3, 48, seed=3)
    kw = dict(vp=2, bones=True, mesh_opacity=0.5, out_width=20)
    eager = seq.render((40, 48), **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = seq.render((40, 48), **kw)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        for k in FIELDS:
            assert same_bits(getattr(cap, k), getattr(eager, k)), k
    seq.verts.mul_(1.07).add_(0.01)
    seq.rtk[:, 0, 3] += 0.05
    g.replay()
    torch.cuda.synchronize()
    fresh = seq.render((40, 48), **kw)
    assert not same_bits(fresh.color, eager.color)
    for k in FIELDS:
        assert same_bits(getattr(cap, k), getattr(fresh, k)), k


def test_error_colours_and_status():
    seq, host = chain_sequence()
    F, V = 3, 42
    err = np.random.default_rng(2).uniform(0, 0.25, (F, V)).astype(np.float32)
    err[0, 0], err[1, 1], err[2, 2], err[2, 3] = np.nan, -0.3, 0.2, 7.0                # NaN, under, exactly 1 after the 5 x, over
    table = np.asarray(PLASMA, np.float64)
    want, nan = sn.error_colors(err, table)
    rec, status = records_on_device(host["verts"], np.tile(host["faces"][None], (F, 1, 1)), host["faces"], error=err)
    assert np.array_equal(np_(rec[:, :, :3]), want) and np_(status)[SR.NAN_ERROR] == 1 == int(nan.sum())
    assert tuple(want[0, 0]) == (0, 0, 0) and tuple(want[1, 1]) == PLASMA[0] and tuple(want[2, 2]) == PLASMA[255] == tuple(want[2, 3])
    out = seq.render((48, 48), vertex_error=dev(err), out_width=24)
    st = np_(out.status)
    assert st[SR.NAN_ERROR] == 1 and st[SR.DROPPED] == 0 and st[SR.EMPTY] == 0
    gray = seq.render((48, 48), gray_color=True, smooth=False, out_width=24)
    c = np_(gray.color)[np_(gray.sil) > 0]
    assert c.max() <= int(76 * 1.4) and np.all(c[:, 0] == c[:, 1]) and not same_bits(gray.color, out.color)
    # a sequence behind the camera: every face dropped, every frame empty
    behind = host["rtk"].copy()
    behind[:, 2, 3] = -3.0
    back = seq.render((48, 48), cams=dev(behind), out_width=24)
    st = np_(back.status)
    assert st[SR.EMPTY] == F and st[SR.DROPPED] == F * 80 and not np_(back.sil).any()


def test_tuple_input_save_ctrajs_and_refusals(tmp_path):
    seq, host = chain_sequence()
    tup = (seq.verts, seq.faces, seq.colors, seq.rtk)
    a, b = SR.render_sequence(tup, (40, 48), vp=1, out_width=20), seq.render((40, 48), vp=1, out_width=20)
    for k in FIELDS:
        assert same_bits(getattr(a, k), getattr(b, k)), k
    paths = a.save_ctrajs(str(tmp_path / "run"))
    assert len(paths) == 3 and paths[2].endswith("run-ctrajs-00002.txt")
    assert np.allclose(np.loadtxt(paths[1]), np_(a.ctrajs[1]), rtol=0, atol=0)
    with pytest.raises(ValueError, match="bones"):
        SR.render_sequence(tup, (40, 48), bones=True)
    with pytest.raises(ValueError, match="rest"):
        SR.render_sequence(tup, (40, 48), rest=True)
    rest = seq.render((40, 48), rest=True, bones=True, out_width=20)
    assert (np_(rest.sil) > 0).any() and np_(rest.status)[SR.EMPTY] == 0
    with pytest.raises(NotImplementedError, match="requires grad"):
        SR.render_sequence((seq.verts.clone().requires_grad_(), seq.faces, seq.colors, seq.rtk), (40, 48))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        SR.render_sequence((seq.verts.cpu(), seq.faces, seq.colors, seq.rtk), (40, 48))
    for bad, match in (((seq.verts[0], seq.faces, seq.colors, seq.rtk), "verts"), ((seq.verts, seq.faces[:, :2], seq.colors, seq.rtk), "faces"),
                       ((seq.verts, seq.faces, seq.colors[:5], seq.rtk), "colors"), ((seq.verts, seq.faces, seq.colors, seq.rtk[:2]), "rtk")):
        with pytest.raises(ValueError, match=match):
            SR.render_sequence(bad, (40, 48))
    with pytest.raises(ValueError, match="overlay"):
        seq.render((40, 48), overlay=torch.zeros((3, 40, 47, 3), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="vertex_error"):
        seq.render((40, 48), vertex_error=torch.zeros((3, 41), device=DEV))
    for opt in ("vis_traj", "vis_cam", "floor", "shadows", "vis_gtmesh", "append_img", "clean", "gif", "mp4", "jpg"):
        with pytest.raises(NotImplementedError, match=opt):
            seq.render((40, 48), **{opt: True})
    with pytest.raises(NotImplementedError, match="orthographic"):
        seq.render((40, 48), cam_type="orthographic")
