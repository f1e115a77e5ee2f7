"""CPU checks of the warm-up stages (moda_amd/warmup.py, csrc/warmup_kernels.hip): the restatement tests/warmup_numpy.py against the
reference's own records in tests/golden/g36_warmup.npz (float64 at 1e-10, fp32 inside the derived bounds, the sample points bit
for bit), the quaternion round trip, the wiring of the new entries and the refusals.  The GPU tests (tests/test_gpu_warmup.py)
hold the kernels to this oracle."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import warmup_numpy as O  # noqa: E402
from _ref_import import _quaternion_to_matrix  # noqa: E402  (the published closed form restated there; it imports nothing else)
from moda_amd import _lib, build, geom_utils, loss_utils, warmup  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "g36_warmup.npz"))
NEW_ENTRIES = ("moda_shape_target", "moda_shape_loss_fwd", "moda_shape_loss_bwd", "moda_rtk_loss_fwd", "moda_rtk_loss_bwd",
               "moda_root_sm1_fwd", "moda_root_sm1_bwd", "moda_matrix_to_quat")
MODES = (("ellips", True), ("sphere", False))
TOL64 = 1e-10


def close64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() <= TOL64 * max(1.0, np.abs(b).max())


def obj_bound():
    return np.abs(G["shape/pts"]).max(0)


# ---- shape_init_loss ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,ellips", MODES)
def test_sample_points_match_reference_bit_for_bit(mode, ellips):
    val, _ = O.shape_target(G[f"shape/{mode}/u"], obj_bound(), float(G["shape/bound_factor"]), ellips, np.float32)
    assert val["pts"].dtype == np.float32 and np.array_equal(val["pts"], G[f"shape/{mode}/f32/pts_samp"])
    wide, _ = O.shape_target(G[f"shape/{mode}/u"], obj_bound(), float(G["shape/bound_factor"]), ellips, np.float64, wide_pts=True)
    assert close64(wide["pts"], G[f"shape/{mode}/f64/pts_samp"])


@pytest.mark.parametrize("mode,ellips", MODES)
def test_shape_loss_float64_matches_reference(mode, ellips):
    pre = f"shape/{mode}/f64/"
    tgt, _ = O.shape_target(G[f"shape/{mode}/u"], obj_bound(), float(G["shape/bound_factor"]), ellips, np.float64, wide_pts=True)
    val, _ = O.shape_loss(G[pre + "y"], tgt["dis"])
    assert close64(val["loss"], G[pre + "loss"]) and close64(val["dy"], G[pre + "dy"])
    n = len(G[pre + "y"])
    assert close64(tgt["dis"], -G[pre + "y"] + G[pre + "dy"] * n / 2)        # the targets, through dy = -2 (-y - dis) / N


@pytest.mark.parametrize("mode,ellips", MODES)
def test_shape_loss_fp32_inside_the_bound(mode, ellips):
    pre = f"shape/{mode}/f32/"
    t32, _ = O.shape_target(G[f"shape/{mode}/u"], obj_bound(), float(G["shape/bound_factor"]), ellips, np.float32)
    t64, tb = O.shape_target(G[f"shape/{mode}/u"], obj_bound(), float(G["shape/bound_factor"]), ellips, np.float64)
    assert (np.abs(t32["dis"].astype(np.float64) - t64["dis"]) <= tb["dis"]).all()
    assert tb["dis"].max() < 1e-6                                              # the bound is a few ulp of the bound's size
    v64, b = O.shape_loss(G[pre + "y"], t32["dis"])
    assert abs(float(G[pre + "loss"]) - v64["loss"]) <= b["loss"]
    # the reference's dy was formed from ITS fp32 targets: the targets' bound enters through d dy / d dis = 2 / N
    n = len(G[pre + "y"])
    assert (np.abs(G[pre + "dy"].astype(np.float64) - v64["dy"]) <= b["dy"] + 2 * tb["dis"] * 2 / n).all()
    v32, _ = O.shape_loss(G[pre + "y"], t32["dis"], dtype=np.float32)
    assert abs(float(v32["loss"]) - v64["loss"]) <= b["loss"] and (np.abs(v32["dy"] - v64["dy"]) <= b["dy"]).all()


# ---- rtk_loss -------------------------------------------------------------------------------------------------------------------
def test_rtk_loss_float64_matches_reference():
    for which, g in (("total", (1.0, 0.0, 0.0)), ("rot", (0.0, 1.0, 0.0))):
        val, _ = O.rtk_loss(G["rtk/pred"], G["rtk/raw"], g)
        assert close64(val["drtk"], G[f"rtk/f64/d_{which}"])
    for k in ("total", "rot_loss", "trn_loss"):
        assert close64(val[k], G[f"rtk/f64/{k}"])


def test_rtk_loss_fp32_inside_the_bound():
    for which, g in (("total", (1.0, 0.0, 0.0)), ("rot", (0.0, 1.0, 0.0))):
        val, b = O.rtk_loss(G["rtk/pred"], G["rtk/raw"], g)
        assert (np.abs(G[f"rtk/f32/d_{which}"] - val["drtk"]) <= b["drtk"]).all()
        v32, _ = O.rtk_loss(G["rtk/pred"], G["rtk/raw"], g, np.float32)
        assert (np.abs(v32["drtk"] - val["drtk"]) <= b["drtk"]).all()
    for k in ("total", "rot_loss", "trn_loss"):
        assert abs(float(G[f"rtk/f32/{k}"]) - val[k]) <= b[k] and abs(float(v32[k]) - val[k]) <= b[k]
    assert b["total"] < 1e-5 * val["total"] and b["drtk"].max() < 1e-3 * np.abs(val["drtk"]).max()     # the bounds are not vacuous


def test_rtk_loss_clamp_cases_are_in_the_record():
    val, _ = O.rtk_loss(G["rtk/pred"], G["rtk/raw"], (0.0, 1.0, 0.0))
    assert (val["drtk"][3, :3, :3] == 0).all() and (val["drtk"][5, :3, :3] == 0).all()       # clamped at the top / at the bottom
    assert (np.abs(val["drtk"][[0, 1, 2, 4], :3, :3]).reshape(4, -1).max(1) > 0).all()
    assert (val["drtk"][:, 3] == 0).all()


# ---- compute_root_sm_loss -------------------------------------------------------------------------------------------------------
def test_root_sm_loss_matches_reference():
    val, b = O.root_sm_loss(G["sm/rtk"], G["sm/data_offset"])
    assert val["pairs"] == 0 + 1 + 2 + 33
    assert close64(val["loss"], G["sm/f64/loss"]) and close64(val["drtk"], G["sm/f64/d"])
    assert abs(float(G["sm/f32/loss"]) - val["loss"]) <= b["loss"]
    assert (np.abs(G["sm/f32/d"] - val["drtk"]) <= b["drtk"]).all()
    v32, _ = O.root_sm_loss(G["sm/rtk"], G["sm/data_offset"], dtype=np.float32)
    assert abs(float(v32["loss"]) - val["loss"]) <= b["loss"] and (np.abs(v32["drtk"] - val["drtk"]) <= b["drtk"]).all()
    assert b["loss"] < 1e-5 * val["loss"]
    assert (val["drtk"][0] == 0).all()                                         # the one-frame video has no pair


def test_root_sm_loss_degenerate_cases():
    rtk = G["sm/rtk"][:4]
    val, _ = O.root_sm_loss(rtk, (0, 1, 2, 3, 4))                              # only one-frame videos: no pair at all
    assert np.isnan(val["loss"]) and val["pairs"] == 0 and (val["drtk"] == 0).all()
    rep = np.stack([rtk[0], rtk[0], rtk[1]])                                   # a repeated frame: zero difference, gradient 0
    val, _ = O.root_sm_loss(rep, (0, 3))
    assert np.isfinite(val["drtk"]).all() and (val["drtk"][0, :3, 3] == 0).all()


def test_zero_norm_subgradient_is_torchs():
    t = torch.zeros(2, 3, dtype=torch.float64, requires_grad=True)
    (t[0] - t[1]).norm(2, -1).backward()
    assert (t.grad == 0).all()


# ---- matrix_to_quaternion -------------------------------------------------------------------------------------------------------
def quat_cases():
    return np.concatenate([O.random_rotations(np.random.default_rng(5), 500), O.half_turns(), np.eye(3, dtype=np.float32)[None]])


@pytest.mark.parametrize("dtype,bound", [(np.float64, O.ROUNDTRIP_F64), (np.float32, O.ROUNDTRIP_F32)])
def test_quaternion_round_trip(dtype, bound):
    R = quat_cases()
    q = O.matrix_to_quaternion(R, dtype)
    assert (q[:, 0] >= 0).all()
    assert np.abs(np.linalg.norm(q.astype(np.float64), axis=1) - 1).max() <= 8 * (O.U32 if dtype == np.float32 else 1e-15)
    back = _quaternion_to_matrix(torch.from_numpy(q.astype(np.float64))).numpy()
    assert np.abs(back - R).max() <= bound
    assert np.abs(O.quaternion_to_matrix(q) - back).max() <= 1e-14             # the oracle's own inverse agrees with _ref_import's


def test_quaternion_half_turns_take_one_branch_per_axis():
    q = O.matrix_to_quaternion(O.half_turns()[:3])
    assert np.array_equal(np.abs(q), np.eye(4)[1:])                            # real part 0: x, y, z dominate in turn
    assert np.array_equal(O.matrix_to_quaternion(np.eye(3, dtype=np.float32)[None]), [[1, 0, 0, 0]])


# ---- wiring ---------------------------------------------------------------------------------------------------------------------
def test_source_is_built():
    assert "warmup_kernels.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "warmup_kernels.hip"))


def test_entries_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "moda_hip.h")).read()
    declared = set(re.findall(r"\b(moda_[a-z0-9_]+)\s*\(", hdr))
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.moda_abi_version() == _lib.ABI_VERSION == 11
    from moda_amd import autograd
    assert autograd.SHAPE_LOSS_MAX_BLOCKS == int(re.search(r"#define MODA_SHAPE_LOSS_MAX_BLOCKS\s+(\d+)", hdr).group(1))


def test_public_names():
    import moda_amd
    for n in ("shape_init_loss", "rtk_loss", "compute_root_sm_loss"):
        assert getattr(moda_amd, n) is getattr(loss_utils, n)
    assert moda_amd.matrix_to_quaternion is geom_utils.matrix_to_quaternion
    for n in ("forward_warmup_shape", "forward_warmup_rootmlp", "preset_root_rotations", "WarmupHarness"):
        assert getattr(moda_amd, n) is getattr(warmup, n)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refuses_cpu_tensors():
    from moda_amd import NeRF, Embedding
    net, emb = NeRF(D=5, W=64, in_channels_xyz=63), Embedding(3, 10)
    rtk = torch.eye(4).repeat(3, 1, 1)
    for name, call in (("pts", lambda: loss_utils.shape_init_loss(torch.zeros(4, 3), None, net, emb, 2.4)),
                       ("u", lambda: loss_utils.shape_targets(torch.zeros(4, 3), torch.ones(3), 2.4)),
                       ("rtk", lambda: loss_utils.rtk_loss(rtk, rtk, {})),
                       ("rtk_all", lambda: loss_utils.compute_root_sm_loss(rtk, (0, 3))),
                       ("R", lambda: geom_utils.matrix_to_quaternion(rtk[:, :3, :3])),
                       ("dp_verts_unit", lambda: warmup.WarmupHarness(net, emb, torch.zeros(4, 3), dict(warmup_shape_ep=5)))):
        with pytest.raises(RuntimeError, match=name + r"\b.*CUDA"):
            call()


def test_refuses_other_root_modules_before_anything_else():
    from moda_amd import RTExplicit
    with pytest.raises(NotImplementedError, match="RTExplicit.*expmlp"):
        warmup.preset_root_rotations(RTExplicit(4), torch.eye(4).repeat(4, 1, 1))
    with pytest.raises(NotImplementedError, match="Linear"):
        warmup.preset_root_rotations(torch.nn.Linear(2, 2), torch.eye(4).repeat(4, 1, 1))
