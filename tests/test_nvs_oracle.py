"""CPU checks of novel-view frame rendering (moda_amd/nvs.py, csrc/nvs_kernels.hip): the numpy restatement tests/nvs_numpy.py
against the reference's own records in tests/golden/g37_nvs.npz, the wiring of the new entries, the public names and the
refusals.  The GPU tests (tests/test_gpu_nvs.py) hold the kernels to this oracle.

The bar for rays_d / rays_o is rel_err < 1e-5, the bar at which the suite holds raycast to its reference record (G12,
test_gpu_feeders.test_raycast_matches_reference; test_oracle_vs_golden has no raycast case of its own).  Everything else the
oracle produces is a selection or a copy and is held exactly."""
import os
import re

import numpy as np
import pytest
import torch

import nvs_numpy as O
from helpers import golden, rel_err
from moda_amd import _lib, build, nvs as NV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("moda_mask_compact_tiles", "moda_mask_compact", "moda_nvs_rays", "moda_nvs_assemble")
RAYCAST_BAR = 1e-5


@pytest.mark.parametrize("tag", ["nf", "auto"])
def test_oracle_matches_reference_record(tag):
    g = golden("g37_nvs")
    S = int(g["img_size"])
    rays = O.construct_rays_nvs(S, g["rtks"], g["near_far"] if tag == "nf" else None, g["masks"])
    assert g["counts"].tolist() == [0, S * S, int((g["masks"][2] > 0).sum())] and 0 < g["counts"][2] < S * S
    assert rays["nsample"] == int(g["counts"].sum()) and rays["bs"] == 1
    for k in ("xys", "near", "far", "rtk_vec"):
        assert np.array_equal(rays[k][0], g[f"{tag}/{k}"]), k
    for k in ("rays_d", "rays_o"):
        assert rays[k][0].shape == g[f"{tag}/{k}"].shape
        assert rel_err(rays[k][0], g[f"{tag}/{k}"]) < RAYCAST_BAR, (k, rel_err(rays[k][0], g[f"{tag}/{k}"]))


def test_oracle_list_rules():
    m = np.zeros((2, 3, 3), np.float32)
    m[0, 0, 1], m[0, 2, 2], m[1, 1, 0] = 1, 0.25, 7
    m[1, 0, 0], m[1, 0, 1], m[1, 0, 2] = np.nan, -0.0, -3
    offsets, pix, frame, rank = O.mask_to_pixels(m)
    assert offsets.tolist() == [0, 2, 3] and pix.tolist() == [1, 8, 3] and frame.tolist() == [0, 0, 1]
    assert rank.reshape(-1).tolist() == [-1, 0, -1, -1, -1, -1, -1, -1, 1, -1, -1, -1, 2, -1, -1, -1, -1, -1]


def test_oracle_assembly_and_8_bit_rules():
    m = np.zeros((1, 3, 3), np.float32)
    m[0, 0, :] = 1
    m[0, 2, 0] = 1
    sil = np.asarray([0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nan, 0.9], np.float32)
    rgb = np.arange(12, dtype=np.float32).reshape(4, 3) / 16
    dep, vis = np.asarray([2, 3, 4, 5], np.float32), np.asarray([0.1, 0.2, 0.3, 0.4], np.float32)
    c_rgb, c_dep, c_sil, c_vis = O.assemble(m, rgb, dep, sil, vis)
    assert c_sil[0, 0, 0] == 0.5 and c_sil[0, 0, 1] == 0 and np.isnan(c_sil[0, 0, 2]) and c_sil[0, 2, 0] == np.float32(0.9)
    assert np.array_equal(c_rgb[0, 0, 0], rgb[0]) and (c_rgb[0, 0, 1] == 1).all() and np.array_equal(c_rgb[0, 0, 2], rgb[2])
    assert c_dep[0, 0].tolist() == [2, 3, 4] and c_vis[0, 2, 0] == np.float32(0.4)
    outside = m[0] == 0
    assert (c_rgb[0][outside] == 1).all() and (c_dep[0][outside] == 1).all() and (c_sil[0][outside] == 1).all() \
        and (c_vis[0][outside] == 1).all()
    # halves go to the even integer, NaN to 0, the ends saturate
    v = np.asarray([0.5 / 255, 1.5 / 255, 2.5 / 255, np.nan, -1, 2, 1, 0, np.inf, -np.inf], np.float32)
    t = v[:3] * np.float32(255)
    assert t.tolist() == [0.5, 1.5, 2.5]
    assert O.to_uint8(v).tolist() == [0, 2, 2, 0, 0, 255, 255, 0, 255, 0]
    assert O.crop_short_edge(np.zeros((2, 10, 10)), 4, 5).shape == (2, 8, 10)
    assert O.crop_short_edge(np.zeros((2, 10, 10, 3)), 5, 3).shape == (2, 10, 6, 3)


# ---- wiring ---------------------------------------------------------------------------------------------------------------
def test_source_is_built():
    assert "nvs_kernels.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "nvs_kernels.hip"))


def test_entries_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "moda_hip.h")).read()
    declared = set(re.findall(r"\b(moda_[a-z0-9_]+)\s*\(", hdr))
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.moda_abi_version() == _lib.ABI_VERSION == 11
    assert NV.SCAN_TILE == int(re.search(r"#define MODA_NVS_SCAN_TILE\s+(\d+)", hdr).group(1))
    max_tiles = int(re.search(r"#define MODA_NVS_MAX_TILES\s+(\d+)", hdr).group(1))
    # the tile count and its refusals are host arithmetic
    assert lib.moda_mask_compact_tiles(3, 33) == 3 * 2 and lib.moda_mask_compact_tiles(1, 32) == 1
    assert lib.moda_mask_compact_tiles(2, 32768) == -1                       # 2^31 pixels
    assert lib.moda_mask_compact_tiles(max_tiles, 1) == -1 and lib.moda_mask_compact_tiles(max_tiles - 1, 1) == max_tiles - 1
    assert lib.moda_mask_compact_tiles(0, 4) == -1 and lib.moda_mask_compact_tiles(4, 0) == -1


def test_public_names():
    import moda_amd
    for n in ("mask_to_pixels", "construct_rays_nvs", "render_nvs", "crop_short_edge", "assemble_frames", "NVSFrames"):
        assert getattr(moda_amd, n) is getattr(NV, n)
    assert NV.NVSFrames._fields == ("rgb", "depth", "sil", "vis", "rgb8", "sil8", "vis8", "offsets")


# ---- refusals (none of them needs a GPU) -----------------------------------------------------------------------------------
def test_refuses_2_to_the_31_pixels_before_any_launch():
    big = torch.empty((2, 32768, 32768), dtype=torch.uint8, device="meta")    # no memory behind it
    with pytest.raises(ValueError, match="2\\^31"):
        NV.mask_to_pixels(big)
    with pytest.raises(ValueError, match="2\\^31"):
        NV._check_masks("render_nvs", big)
    assert NV._check_masks("mask_to_pixels", torch.empty((1, 46340, 46340), dtype=torch.uint8, device="meta")) == (1, 46340)


def test_refuses_shape_mismatch():
    with pytest.raises(ValueError, match="masks must be"):
        NV.mask_to_pixels(torch.zeros(2, 6, 8))
    with pytest.raises(ValueError, match="masks must be"):
        NV.mask_to_pixels(torch.zeros(6, 6))
    with pytest.raises(ValueError, match="not resized"):                      # a silhouette at another size than the render
        NV.construct_rays_nvs(8, np.zeros((1, 4, 4), np.float32), None, np.ones((6, 6)), "cpu")
    with pytest.raises(ValueError, match="not resized"):
        NV.construct_rays_nvs(8, np.zeros((2, 4, 4), np.float32), None, np.ones((3, 8, 8)), "cpu")
    with pytest.raises(ValueError, match="rtks"):
        NV.construct_rays_nvs(8, np.zeros((2, 3, 4), np.float32), None, np.ones((8, 8)), "cpu")
    with pytest.raises(ValueError, match="rank"):
        NV.assemble_frames(torch.zeros(1, 4, 5, dtype=torch.int32), torch.zeros(0, 3), torch.zeros(0), torch.zeros(0), torch.zeros(0))


def test_refuses_dtype_cpu_tensors_and_grad():
    with pytest.raises(ValueError, match="float32"):
        NV.mask_to_pixels(torch.zeros(1, 4, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="contiguous"):
        NV.mask_to_pixels(torch.zeros(1, 4, 8)[:, :, ::2])
    with pytest.raises(NotImplementedError, match="grad"):
        NV.mask_to_pixels(torch.zeros(1, 4, 4, requires_grad=True))
    with pytest.raises(RuntimeError, match="CUDA"):
        NV.mask_to_pixels(torch.zeros(1, 4, 4))
    with pytest.raises(RuntimeError, match="CUDA"):
        NV.construct_rays_nvs(4, np.zeros((1, 4, 4), np.float32), None, np.ones((4, 4)), "cpu")
    with pytest.raises(RuntimeError, match="CUDA"):
        NV.assemble_frames(torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(0, 3), torch.zeros(0), torch.zeros(0), torch.zeros(0))


def test_crop_short_edge_returns_views():
    fr = NV.NVSFrames(torch.zeros(2, 10, 10, 3), torch.zeros(2, 10, 10), torch.zeros(2, 10, 10), torch.zeros(2, 10, 10))
    vert = NV.crop_short_edge(fr, 5, 3)                                       # portrait: the columns [:6]
    assert vert.rgb.shape == (2, 10, 6, 3) and vert.depth.shape == vert.sil.shape == vert.vis.shape == (2, 10, 6)
    assert vert.rgb8 is None and vert.rgb.data_ptr() == fr.rgb.data_ptr()
    hori = NV.crop_short_edge(fr, 4, 5)                                       # landscape: the rows [:8]
    assert hori.rgb.shape == (2, 8, 10, 3) and hori.vis.shape == (2, 8, 10)
    assert NV.crop_short_edge(fr.sil[0], 4, 5).shape == (8, 10)
    assert NV.crop_short_edge(fr, 7, 7).sil.shape == (2, 10, 10)
