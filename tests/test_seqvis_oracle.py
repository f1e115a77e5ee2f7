"""CPU: the float64 restatement tests/seqvis_numpy.py against what can be pinned from outside -- Rodrigues to scipy, the committed
plasma table and its lookup rule to the installed matplotlib, obj_to_cam and the pixel projection to oracle/torch_ref.project --
and the structure around it: the CSR order, the fourth ABI header, the exports, the refusals, and that the inputs of the GPU
shading and resize tests keep their near-boundary share under 1 %.  The viewpoint block, the compositing, the overlay and the
resize are restated and UNPINNED: pyrender, trimesh and cv2 are absent, the reference script cannot run."""
import os
import sys

import numpy as np
import pytest
import torch

import seqvis_numpy as sn

HERE = os.path.dirname(os.path.abspath(__file__))
SHADE_SIZES = ((48, 64), (64, 48), (1, 33), (37, 37))
OPACITIES = (0.0, 254 / 255, 0.5, 1.0)
NEAR_CAP = 0.01
NAMES = ("moda_seqvis_cams", "moda_seqvis_project", "moda_seqvis_records", "moda_seqvis_shade", "moda_seqvis_resize")


def shade_case(H, W, seed=0, V=40, Nf=60):
    """Synthetic raster planes of one frame, S = max(H, W): per layer face_idx (-1 on about a third of the pixels), barycentrics,
    depths in [1, 5), records with colours up to 230 (so some pixels reach the clamp at 255) and unit normals, camera-frame
    vertices; an overlay.  Every combination of present / absent and nearer / farther occurs."""
    rng = np.random.default_rng(1000 * H + W + seed)
    S = max(H, W)

    def layer():
        fi = rng.integers(0, Nf, (S, S)).astype(np.int32)
        fi[rng.uniform(size=(S, S)) < 0.33] = -1
        b = rng.uniform(0.05, 1.0, (S, S, 3))
        b = (b / b.sum(-1, keepdims=True)).astype(np.float32)
        z = np.where(fi >= 0, rng.uniform(1.0, 5.0, (S, S)), 0.0).astype(np.float32)
        faces = np.stack([rng.permutation(V)[:3] for _ in range(Nf)]).astype(np.int32)
        n = rng.standard_normal((V, 3))
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        rec = np.zeros((V, 8), np.float32)
        rec[:, :3] = np.floor(rng.uniform(0, 231, (V, 3)))
        rec[:, 3:6] = n
        cam = rng.standard_normal((V, 3)).astype(np.float32)
        return fi, b, z, faces, rec, cam
    return {"S": S, "body": layer(), "bone": layer(), "overlay": rng.integers(0, 256, (H, W, 3)).astype(np.uint8)}


def resize_case(H, W, seed=0):
    """Random bytes and a 0 / 100 silhouette of one block.  At the scales 2 / 15 and 1 / 10 (W = 64 and 48 to 480) the weights are the
    small rationals a / 225 and a / 400, and random bytes put 2-3 % of the outputs on an exact half; there the bytes are
    multiples of 16, which cannot (16 sum(a p) / 225 or / 400 is never an odd half)."""
    rng = np.random.default_rng(77 * H + W + seed)
    step = 16 if W in (48, 64) else 1
    color = (step * rng.integers(0, 256 // step, (H, W, 3))).astype(np.uint8)
    sil = np.zeros((H, W), np.int16)                                                 # a block, as a silhouette is: 100 a / 400 is
    sil[:max(1, (10 * H) // 37), :max(2, (20 * W) // 33)] = 100                          # a half too often for random pixels
    return color, sil


RESIZE_CASES = tuple((H, W, 480) for H, W in SHADE_SIZES) + ((37, 33, 20),)


# ---- the three external pins -------------------------------------------------------------------------------------------------------
def test_rodrigues_equals_scipy():
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(0)
    vecs = [[0, np.pi / 2, 0], [np.pi / 2, 0, 0], [0, np.pi / 3, 0], [np.pi, 0, 0], [0, 0, 0]]
    vecs += [[0, i * 2 * np.pi / F, 0] for F in (1, 2, 65) for i in range(F)]
    vecs += list(rng.uniform(-2, 2, (50, 3)))
    worst = max(np.abs(sn.rodrigues(v) - Rotation.from_rotvec(np.asarray(v, np.float64)).as_matrix()).max() for v in vecs)
    print("rodrigues against scipy", worst)
    assert worst < 1e-15


def test_plasma_table_and_lookup_equal_matplotlib():
    import matplotlib
    sys.path.insert(0, os.path.dirname(HERE))
    from moda_amd import plasma_table as pt
    cm = matplotlib.colormaps['plasma']
    table = np.asarray(pt.PLASMA)
    assert table.shape == (256, 3) and matplotlib.__version__.split(".")[:2] == pt.MATPLOTLIB_VERSION.split(".")[:2]
    assert np.array_equal(table, cm(np.arange(256), bytes=True)[:, :3])
    below = np.nextafter(np.float32(1 / 256), np.float32(0))
    for x in (-0.1, 0.0, 1 / 256, below, 0.999, 1.0, 7.0, np.nan):
        x = np.float32(x)
        got, nan = sn.plasma_lookup(x, table)
        want = cm(x, bytes=True)
        assert np.array_equal(got, np.asarray(want[:3], np.float64)), (x, got, want)
        assert bool(nan) == bool(np.isnan(x)) and (not nan or tuple(got) == pt.BAD)
    got, nan = sn.plasma_lookup([1 / 256, below], table)
    assert np.array_equal(got[0], table[1]) and np.array_equal(got[1], table[0])


def test_projection_equals_the_oracles_project():
    sys.path.insert(0, os.path.dirname(HERE))
    from oracle import torch_ref
    rng = np.random.default_rng(1)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    pts = rng.standard_normal((1, 50, 3))
    fx, fy, px, py = 40.0, 37.0, 24.0, 20.0
    t = np.array([0.1, -0.2, 4.0])
    kinv = np.linalg.inv(np.array([[fx, 0, px], [0, fy, py], [0, 0, 1.0]]))
    vec = np.concatenate([q.reshape(-1), t, kinv.reshape(-1)])[None]
    ref = torch_ref.project(torch.as_tensor(pts), torch.as_tensor(vec))[0].numpy()
    cam = np.eye(4)
    cam[:3, :3], cam[:3, 3], cam[3] = q, t, (fx, fy, px, py)
    xyz = sn.obj_to_cam(pts[0], cam)
    u, v, _ = sn.pixels(xyz, cam[3])
    assert np.abs(xyz[:, 2] - ref[:, 2]).max() < 1e-13
    # the oracle divides by (1e-6 + Z): undo that
    z = ref[:, 2]
    assert np.abs(ref[:, 0] * (1e-6 + z) / z - u).max() < 1e-10 and np.abs(ref[:, 1] * (1e-6 + z) / z - v).max() < 1e-10


# ---- structure --------------------------------------------------------------------------------------------------------------------
def test_csr_of_a_valence_70_fan_is_ascending():
    verts, faces = sn.fan(70)
    off, ent = sn.vertex_csr(faces, len(verts))
    hub = ent[off[0]:off[1]]
    assert len(hub) == 70 and np.array_equal(hub // 3, np.arange(70)) and np.all(hub % 3 == 0)
    for v in range(len(verts)):
        row = ent[off[v]:off[v + 1]]
        assert np.all(np.diff(row) > 0) and np.all(faces.reshape(-1)[row] == v)
    assert off[-1] == 3 * len(faces)
    bad = faces.copy()
    bad[3, 1] = 999
    off, ent = sn.vertex_csr(bad, len(verts))
    assert off[-1] == 3 * len(faces) - 1 and ent[-1] == 3 * 3 + 1


def test_base_colour_is_the_integer_rule():
    c = np.arange(256)
    assert np.array_equal(sn.base_u8(c), (3 * c) // 5)
    assert np.array_equal(np.floor(np.float32(0.6) * c.astype(np.float32)), (3 * c) // 5)      # render_mesh's fp32 floor


def test_fourth_header_parses_and_is_exported():
    sys.path.insert(0, os.path.dirname(HERE))
    from moda_amd import abi, build, _lib
    with open(next(h for h in build.HEADERS if h.endswith("moda_hip_seqvis.h"))) as f:
        protos, structs, consts = abi.parse(f.read())
    assert tuple(protos) == NAMES == tuple(abi.SEQVIS_PROTOTYPES) == _lib.SEQVIS_EXPORTS and not structs
    assert all(k.startswith("MODA_SEQVIS_") for k in consts) and consts == abi.SEQVIS_CONSTANTS
    assert "seqvis_kernels.hip" in build.SOURCES
    assert len(abi.PROTOTYPES) == 141 and len(abi.VIS_PROTOTYPES) == 5 and len(abi.CAM_PROTOTYPES) == 7
    tables = (abi.PROTOTYPES, abi.VIS_PROTOTYPES, abi.CAM_PROTOTYPES, abi.SEQVIS_PROTOTYPES)
    for name in NAMES:
        assert sum(name in t for t in tables) == 1
    text = "".join(open(h).read() for h in build.HEADERS if h.endswith(".h") and os.sep + "include" + os.sep in h)
    for name in NAMES:
        assert text.count(name + "(") == 1, name
    consts_all = (abi.CONSTANTS, abi.VIS_CONSTANTS, abi.CAM_CONSTANTS)
    assert not any(set(consts) & set(c) for c in consts_all)
    lib = _lib.load()
    assert lib.moda_abi_version() == _lib.ABI_VERSION == 11
    for name in NAMES:
        assert getattr(lib, name).argtypes == _lib._SEQVIS_SIGNATURES[name][1]
    src = open(os.path.join(build.CSRC, "seqvis_kernels.hip")).read()
    assert "atomicAdd(" in src and "float* word" not in src and '#include "lanes.h"' in src and "__shfl" not in src


def test_refusals_without_a_gpu():
    sys.path.insert(0, os.path.dirname(HERE))
    import moda_amd
    from moda_amd import seq_render as SR
    assert moda_amd.render_sequence is SR.render_sequence and hasattr(moda_amd.MeshSequence, "render")
    verts, faces = torch.zeros(2, 4, 3), torch.zeros(2, 3, dtype=torch.int32)
    colors, rtk = torch.zeros(4, 3, dtype=torch.uint8), torch.eye(4).repeat(2, 1, 1)
    seq = (verts, faces, colors, rtk)
    for opt, val in (("vis_traj", True), ("vis_cam", True), ("floor", True), ("shadows", True), ("cam_type", "orthographic"),
                     ("vis_gtmesh", True), ("append_img", "yes"), ("clean", True), ("gif", True), ("mp4", True), ("jpg", True)):
        with pytest.raises(NotImplementedError, match=opt if opt != "cam_type" else "orthographic"):
            SR.render_sequence(seq, (8, 8), **{opt: val})
    SR._refuse({"cam_type": "perspective", "append_img": "no", "floor": False})
    with pytest.raises(TypeError, match="unknown option"):
        SR.render_sequence(seq, (8, 8), nonsense=1)
    with pytest.raises(NotImplementedError, match="requires grad"):
        SR.render_sequence((verts.clone().requires_grad_(), faces, colors, rtk), (8, 8))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        SR.render_sequence(seq, (8, 8))
    with pytest.raises(ValueError, match="vp"):
        SR.render_sequence(seq, (8, 8), vp=3)
    with pytest.raises(ValueError, match="image_hw"):
        SR.render_sequence(seq, (8, 0))
    with pytest.raises(ValueError, match="mesh_opacity"):
        SR.render_sequence(seq, (8, 8), mesh_opacity=1.5)
    with pytest.raises(ValueError, match="freeze and rest"):
        SR.render_sequence(seq, (8, 8), freeze=True, rest=True)
    assert SR.GRAY_BASE == 76


def test_budget_holds_the_rasterisers_limits():
    sys.path.insert(0, os.path.dirname(HERE))
    from moda_amd import seq_render as SR
    assert SR.frames_per_chunk(1, 64, [(100, 200)]) == 1
    n = SR.frames_per_chunk(1 << 62, 2048, [(1000, 2000)])
    assert n * 2048 * 2048 < 2 ** 31 and (n + 1) * 2048 * 2048 >= 2 ** 31
    n = SR.frames_per_chunk(1 << 62, 8, [(10, 1 << 20)])
    assert n * (1 << 20) * 3 < 2 ** 31
    per = 200 * (12 + 96 + 16) + 100 * 56 + 24 * 64 * 64
    assert SR.frames_per_chunk(2 * per, 64, [(100, 200)]) == 2 and SR.frames_per_chunk(2 * per - 1, 64, [(100, 200)]) == 1


# ---- the GPU tests' inputs keep away from decision boundaries, by the restatement alone ------------------------------------------
@pytest.mark.parametrize("H,W", SHADE_SIZES)
def test_shading_inputs_stay_under_the_near_boundary_cap(H, W):
    c = shade_case(H, W)
    seen = set()
    for smooth in (True, False):
        for op in OPACITIES:
            r = sn.shade(c["body"], c["bone"], H, W, smooth, op, None)
            share = r["near"].mean()
            assert share < NEAR_CAP, (smooth, op, share)
            assert np.all(r["color"][0, 0] == 0) and set(np.unique(r["sil"])) <= {0, 100}
    fi, fb = c["body"][0][:H, :W], c["bone"][0][:H, :W]
    zb, zo = c["body"][2][:H, :W], c["bone"][2][:H, :W]
    both = (fi >= 0) & (fb >= 0)
    seen = {"front": (both & (zo < zb)).any(), "behind": (both & (zo > zb)).any(), "no_bone": ((fi >= 0) & (fb < 0)).any(),
            "no_body": ((fi < 0) & (fb >= 0)).any()}
    assert all(seen.values()) or H * W < 40, seen
    r = sn.shade(c["body"], None, H, W, True, 1.0, c["overlay"])
    assert r["near"].mean() < NEAR_CAP
    if H * W > 1000:
        assert (r["color"] == 255).any() or (sn.shade(c["body"], None, H, W, True, 1.0, None)["color"] == 255).any()     # the clamp is reached


@pytest.mark.parametrize("H,W,ow", RESIZE_CASES)
def test_resize_inputs_stay_under_the_near_boundary_cap(H, W, ow):
    color, sil = resize_case(H, W)
    h = int(H * ow / W)
    out, near = sn.resize(color, h, ow)
    out_s, near_s = sn.resize(sil, h, ow)
    assert out.shape == (h, ow, 3) and out.dtype == np.uint8 and out_s.shape == (h, ow) and out_s.dtype == np.int16
    assert near.mean() < NEAR_CAP and near_s.mean() < NEAR_CAP


def test_resize_restatement_on_exact_cases():
    a = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert np.array_equal(sn.resize(a, 3, 4)[0], a)                                   # the identity
    b = np.array([[0, 100]], np.int16)
    out, _ = sn.resize(b, 1, 4)                                                       # centres at -0.25, 0.25, 0.75, 1.25
    assert list(out[0]) == [0, 25, 75, 100]
    assert sn.resize(np.array([[1, 2]], np.uint8), 1, 1)[0][0, 0] == 2                # 1.5 rounds to even
