"""CPU checks of the frame tables (moda_amd/frame_state.py, csrc/frames_kernels.hip): the float64 restatement
tests/frames_numpy.py against the reference's own records in tests/golden/g33_frames.npz, and the wiring of the new entries.

Three of these are SELF-CHECKS OF THE ORACLE, not of the product: that the reference's fp32 records lie inside the error bound
the oracle states for its float64 values (if one does not, the bound is wrong), that the restated box corners give the planes
of the 8 corners passed explicitly, and that the last-occurrence rule equals numpy's fancy assignment.  The GPU tests
(tests/test_gpu_frames.py) hold the kernels to that oracle and those bounds."""
import os
import re

import numpy as np
import pytest
import torch

import frames_numpy as fn
from moda_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "g33_frames.npz"))
NEW_ENTRIES = ("moda_frames_scatter", "moda_near_far")
CASES = [str(n) for n in G["names"]]
GRID = [(int(M), int(N)) for M in G["grid/M"] for N in G["grid/N"]]


def close(got, want, bound):
    """NaN where want is NaN, the same infinity where want is infinite, within `bound` elsewhere -> the largest excess (<= 0)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern"
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), "infinities"
    return float((np.abs(got[fin] - want[fin]) - np.broadcast_to(bound, want.shape)[fin]).max()) if fin.any() else 0.0


def case_inputs(name):
    rtk = G[name + "/rtk"]
    if name + "/rtk_all" in G.files:
        rtk = fn.patch_poses(rtk, G[name + "/idk"], G[name + "/rtk_all"])
    return G[name + "/pts"], rtk, G[name + "/idk"], G[name + "/nf0"], float(G[name + "/tol"])


@pytest.mark.parametrize("name", CASES)
def test_oracle_equals_the_reference_in_float64(name):
    pts, rtk, idk, nf0, tol = case_inputs(name)
    nf, _ = fn.get_near_far(nf0, rtk, idk, pts, tol)
    assert close(nf, G[name + "/nf64"], 1e-10) <= 0
    if name + "/rtk32" in G.files:                         # the patch copies: exact
        assert np.array_equal(rtk.astype(np.float32), G[name + "/rtk32"])


@pytest.mark.parametrize("M,N", GRID)
def test_oracle_equals_the_reference_in_float64_on_the_grid(M, N):
    nf, bound = fn.get_near_far(G["grid/nf0"][:M], G["grid/rtk"][:M], np.ones(M), G["grid/pts"][:N])
    assert close(nf, G[f"grid/{M}x{N}/nf64"], 1e-10) <= 0
    assert close(G[f"grid/{M}x{N}/nf32"], nf, bound) <= 0               # self-check of the bound


@pytest.mark.parametrize("name", CASES)
def test_reference_fp32_lies_inside_the_stated_bound(name):
    pts, rtk, idk, nf0, tol = case_inputs(name)
    nf, bound = fn.get_near_far(nf0, rtk, idk, pts, tol)
    assert close(G[name + "/nf32"], nf, bound) <= 0
    keep = idk != 1
    assert np.array_equal(G[name + "/nf32"][keep], nf0[keep])             # untouched rows keep their bits


def test_restated_corners_give_the_planes_of_explicit_corners():
    c = fn.box_corners(G["box/bounds"])
    assert sorted(map(tuple, c.tolist())) == sorted(map(tuple, G["box/pts"].astype(np.float64).tolist()))
    a, _ = fn.get_near_far(G["box/nf0"], G["box/rtk"], G["box/idk"], c)
    b, _ = fn.get_near_far(G["box/nf0"], G["box/rtk"], G["box/idk"], G["box/pts"])
    assert np.array_equal(a, b)
    from moda_amd import frame_state
    assert np.array_equal(frame_state.box_corners(G["box/bounds"]), c)
    assert abs(fn.near_far_to_bound(G["box/nf64"]) - float(G["bound64"])) <= 1e-12
    assert abs(fn.near_far_to_bound(G["box/nf32"]) - float(G["bound32"])) <= 1e-6


def test_last_occurrence_equals_numpy_fancy_assignment():
    rng = np.random.default_rng(5)
    for _ in range(200):
        M, bs = int(rng.integers(1, 12)), int(rng.integers(1, 24))
        fid = rng.integers(0, M, bs)
        vals = rng.standard_normal((bs, 3))
        want = np.zeros((M, 3))
        want[fid] = vals
        ids, src, refused = fn.last_occurrence(fid, M)
        got = np.zeros((M, 3))
        got[ids] = vals[src]
        assert refused == 0 and np.array_equal(got, want)
    assert fn.last_occurrence([-1, 2, 5, 2], 5)[2] == 2


@pytest.mark.parametrize("name", [str(n) for n in G["slv/names"]])
def test_save_latest_vars_oracle_against_the_reference(name):
    tabs = {k: G["slv/tab_" + k] for k in ("rtk", "rt_raw", "idk")}
    p = "slv/" + name
    out, bound, refused = fn.save_latest_vars(tabs, G[p + "/rtk"], G[p + "/kaug"], G[p + "/rt_raw"], G[p + "/frameid"])
    assert refused == 0
    for k in ("rtk", "rt_raw", "idk"):
        assert np.abs(out[k] - G[f"{p}/out_{k}64"]).max() <= 1e-10
    b = np.zeros((tabs["rtk"].shape[0], 4, 4))
    b[:, 3] = bound
    assert (np.abs(G[p + "/out_rtk32"].astype(np.float64) - out["rtk"]) <= b).all()          # self-check of the bound
    assert np.array_equal(G[p + "/out_rt_raw32"], out["rt_raw"].astype(np.float32))


def test_new_entries_are_bound_declared_and_exported():
    assert _lib.ABI_VERSION == 11
    header = open(os.path.join(ROOT, "include", "moda_hip.h")).read()
    for name in NEW_ENTRIES:
        assert name in _lib.EXPORTS
        assert re.search(r"\bint " + name + r"\(", header), name
    assert "moda_near_far_splits" in _lib.EXPORTS and re.search(r"\bint32_t moda_near_far_splits\(", header)
    assert "frames_kernels.hip" in build.SOURCES
    lib = _lib.load()
    assert lib.moda_abi_version() == 11
    for name in NEW_ENTRIES:
        assert hasattr(lib, name)
    from moda_amd import frame_state as FS
    m = re.search(r"#define MODA_NEAR_FAR_MAX_SPLIT (\d+)", header)
    assert m and int(m.group(1)) == FS.MAX_SPLIT
    ESHAPE, EINVAL = -2, -1
    assert lib.moda_near_far(None, 0, None, None, None, 4, 1.2, None, 0, None, None, None) == ESHAPE
    assert lib.moda_near_far(None, 8, None, None, None, 0, 1.2, None, 0, None, None, None) == ESHAPE
    assert lib.moda_near_far(None, 8, None, None, None, 4, 1.2, None, 2, None, None, None) == EINVAL       # 8 points are not split
    assert lib.moda_near_far(None, 100, None, None, None, 4, 1.2, None, FS.MAX_SPLIT + 1, None, None, None) == EINVAL
    assert lib.moda_near_far(None, 100, None, None, None, 4, 1.2, None, 0, None, None, None) == EINVAL     # NULL pointers
    assert lib.moda_frames_scatter(None, None, None, None, -1, None, None, None, 4, None, None) == ESHAPE
    assert lib.moda_frames_scatter(None, None, None, None, 2, None, None, None, 0, None, None) == ESHAPE
    assert lib.moda_frames_scatter(None, None, None, None, 2, None, None, None, 4, None, None) == EINVAL
    # the launch shape: no split of the per-step reset, none when the frames alone fill the device, a split on either side of 4096
    assert FS.near_far_splits(8, 1024) == 1 and FS.near_far_splits(27554, 1024) == 1
    assert FS.near_far_splits(4096, 1) == 1 and FS.near_far_splits(4097, 1) == 2
    assert FS.near_far_splits(262144, 64) == 16 and FS.near_far_splits(10 ** 6, 1) == 245


def test_frame_state_imports_and_refuses_without_a_gpu():
    import moda_amd
    from moda_amd import frame_state as FS
    for name in ("FrameState", "save_latest_vars", "get_near_far", "reset_near_far", "near_far_to_bound", "reset_nf", "reset_obj_bound"):
        assert getattr(moda_amd, name) is getattr(FS, name)
    with pytest.raises(TypeError, match="FrameState"):
        FS.save_latest_vars(type("M", (), {"latest_vars": {}})())
    with pytest.raises(NotImplementedError, match="require grad"):
        FS._no_grad("get_near_far", torch.zeros(3, requires_grad=True))
    with pytest.raises(RuntimeError, match="CUDA"):
        FS._table(torch.zeros(4, 2), (4, 2), "near_far")
    assert float(FS.near_far_to_bound(torch.tensor([[1.0, 3.0], [2.0, 6.0]]))) == 1.5
