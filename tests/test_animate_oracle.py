"""CPU (-m "not gpu"): the float64 restatement of the mesh sequence export (tests/animate_numpy.py) is pinned to the reference
BEFORE the GPU is compared to it -- its all-frames forward warp, run for the one frame of tests/golden/g13_grid.npz, reproduces
what the reference's warp_fw wrote there -- and the host parts of moda_amd/animate.py: the OBJ writer, the ellipsoid template,
the palette rule, the library's new entries."""
import os
import re

import numpy as np
import pytest
import torch

import animate_numpy as AN
from helpers import golden, rel_err
from moda_amd import _lib, build, synth
from moda_amd import animate as AM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G13 = dict(B=25, P=200, embedid=3)


@pytest.fixture(scope="module")
def g13_points():
    return np.float32(0.15) * synth.normal(13, "g13/pts", (G13["P"], 3))


def test_restatement_reproduces_the_reference_warp_fw(g13_points):
    """The bounds are the ones tests/test_gpu_mesh_queries.py holds the package to for the same keys: 1e-4 for the points, 1e-5
    for the bones."""
    g = golden("g13_grid")
    m = AN.mock_params(G13["B"])
    verts, bones = AN.warp_fw_frames(m, g13_points, [G13["embedid"]])
    assert verts.shape == (1, G13["P"], 3) and bones.shape == (1, G13["B"], 10)
    e_v, e_b = rel_err(verts[0], g["warp_fw"]), rel_err(bones[0], g["warp_fw_bones"][0])
    print(f"restatement vs reference: warp_fw {e_v:.2e}, warp_fw_bones {e_b:.2e}")
    assert e_v < 1e-4, e_v
    assert e_b < 1e-5, e_b
    dis, _ = AN.warp_fw_frames(m, g13_points, [G13["embedid"]], nerf_dis=True)
    e_d = rel_err(dis[0], g["warp_fw_dis"])
    print(f"restatement vs reference: warp_fw_dis {e_d:.2e}")
    assert e_d < 1e-4, e_d
    assert np.abs(dis - verts).max() > 1e-3                         # the displacement field is not a no-op on this model


def test_restatement_frames_are_independent(g13_points):
    """A frame's row does not depend on the other frames of the call (what the kernel's tile independence is checked against)."""
    m = AN.mock_params(G13["B"])
    many, bones = AN.warp_fw_frames(m, g13_points[:7], [3, 0, 49, 3])
    one, b1 = AN.warp_fw_frames(m, g13_points[:7], [3])
    assert np.array_equal(many[0], one[0]) and np.array_equal(many[3], one[0]) and np.array_equal(bones[3], b1[0])
    assert np.abs(many[1] - many[0]).max() > 1e-6                     # the frames do differ


def test_restatement_degenerate_blend_is_nan_in_its_row_only():
    rng = np.random.default_rng(5)
    q = rng.standard_normal((2, 3, 8)).astype(np.float32)
    q[:, 1, :4] = -q[:, 0, :4]                                      # bones 0 and 1: opposite rotations
    skin = np.asarray([[0.5, 0.5, 0.0], [0.2, 0.3, 0.5]], np.float32)
    out = AN.dqs_frames(q, skin, rng.standard_normal((2, 3)).astype(np.float32))
    assert np.isnan(out[:, 0]).all() and np.isfinite(out[:, 1]).all()


def test_obj_round_trip(tmp_path):
    rng = np.random.default_rng(11)
    v = rng.standard_normal((37, 3)).astype(np.float32) * np.float32(1e-3) ** rng.integers(0, 3, (37, 1)).astype(np.float32)
    f = rng.integers(0, 37, (50, 3))
    c = rng.integers(0, 256, (37, 3)).astype(np.uint8)
    p = str(tmp_path / "m.obj")
    AM.write_obj(p, v, f, c)
    lines = open(p).read().splitlines()
    assert len(lines) == 37 + 50 and all(len(l.split()) == 7 and l.startswith("v ") for l in lines[:37])
    assert all(re.fullmatch(r"f \d+ \d+ \d+", l) for l in lines[37:]) and min(int(x) for l in lines[37:] for x in l.split()[1:]) >= 1
    rv, rf, rc = AM.read_obj(p)
    assert np.array_equal(rv.astype(np.float32), v) and np.array_equal(rf, f)            # 9 digits carry an fp32 value
    assert rc.min() >= 0 and rc.max() <= 1 and np.array_equal(np.rint(rc * 255).astype(np.uint8), c)
    AM.write_obj(p, v, f)                                                                  # no colours: `v x y z`
    rv, rf, rc = AM.read_obj(p)
    assert rc is None and np.array_equal(rv.astype(np.float32), v) and open(p).readline().count(" ") == 3
    AM.write_obj(p, v, f, c.astype(np.float64) / 255)                                      # floats are taken as 0..1 already
    assert np.array_equal(np.rint(AM.read_obj(p)[2] * 255).astype(np.uint8), c)
    with pytest.raises(ValueError, match="faces index"):
        AM.write_obj(p, v, f + 1000)
    with pytest.raises(ValueError, match="colours"):
        AM.write_obj(p, v, f, c[:5])


def test_ellipsoid_template_is_a_closed_outward_sphere():
    v, f = AM.uv_sphere()
    R, S = AM.RINGS, AM.SEGMENTS
    assert v.shape == (2 + (R - 1) * S, 3) == (242, 3) and f.shape == (2 * S * (R - 1), 3) == (480, 3)
    assert np.abs(np.linalg.norm(v, axis=1) - 1).max() < 1e-15 and len(np.unique(np.round(v, 12), axis=0)) == len(v)
    assert f.min() == 0 and f.max() == len(v) - 1 and len(np.unique(f)) == len(v)
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
    edges = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    directed = {(int(a), int(b)) for a, b in edges}
    assert len(directed) == len(edges)                                                  # no directed edge twice ...
    assert all((b, a) in directed for a, b in directed)                                 # ... and every one has its opposite: closed, oriented
    assert len(v) - len(edges) // 2 + len(f) == 2                                       # Euler: a sphere
    vol = np.einsum("ni,ni->n", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6
    assert 0.9 * 4 / 3 * np.pi < vol < 4 / 3 * np.pi                                    # positive: faces counter-clockwise from outside
    v2, f2 = AM.uv_sphere(3, 4)
    assert v2.shape == (10, 3) and f2.shape == (16, 3)
    with pytest.raises(ValueError):
        AM.uv_sphere(1, 8)


def test_palette_rule():
    for n in (1, 25, 36, 64):
        p = AM.default_palette(n)
        assert p.dtype == np.uint8 and p.shape == (n, 3) and np.array_equal(p, AN.default_palette(n))
        assert len(np.unique(p, axis=0)) == n and p.max(1).min() >= 240                 # distinct, value 0.95
    assert np.array_equal(AM.default_palette(36)[:25], AM.default_palette(25))          # colour i depends on i alone


def test_library_entries_and_constants():
    names = ("moda_dqs_frames", "moda_color_dirs", "moda_bone_ellipsoids", "moda_skin_colors")
    assert "animate_kernels.hip" in build.SOURCES
    build.build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "moda_hip.h")).read()
    declared = set(re.findall(r"\b(moda_[a-z0-9_]+)\s*\(", hdr))
    for name in names:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.moda_abi_version() == _lib.ABI_VERSION == 11
    for macro, value in (("MODA_ANIM_BLOCK", AM.BLOCK), ("MODA_ANIM_FRAME_TILE", AM.FRAME_TILE), ("MODA_ANIM_MAX_BONES", AM.MAX_BONES)):
        assert int(re.search(rf"#define {macro} (\d+)", hdr).group(1)) == value, macro
    assert AM.MAX_BONES >= 36 and AM.BLOCK % 64 == 0
    # the C entries refuse what the wrappers refuse, before any launch (no GPU is touched: the checks come first)
    assert lib.moda_dqs_frames(None, None, None, 1, 1, AM.MAX_BONES + 1, 0, None, None) == -2      # MODA_ESHAPE
    assert lib.moda_dqs_frames(None, None, None, 1, 1, 25, 0, None, None) == -1                    # MODA_EINVAL
    assert lib.moda_dqs_frames(None, None, None, 0, 1, 25, 0, None, None) == -2
    assert lib.moda_color_dirs(None, None, None, 1, 1, 17, None, 64, None, None) == -2
    assert lib.moda_bone_ellipsoids(None, 1, None, 242, None, None) == -1
    assert lib.moda_skin_colors(None, None, 0, 25, None, None) == -2


def test_host_tensors_and_grad_inputs_are_refused():
    dq, skin, pts = torch.zeros(2, 25, 8), torch.zeros(5, 25), torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        AM.dqs_frames(dq, skin, pts)
    with pytest.raises(NotImplementedError, match="require grad"):
        AM.dqs_frames(dq, skin, pts.requires_grad_(True))
    with pytest.raises(RuntimeError, match="CUDA"):
        AM.skin_colors(skin)
    with pytest.raises(RuntimeError, match="CUDA"):
        AM.bone_ellipsoids(torch.zeros(1, 25, 10), 1.0)
