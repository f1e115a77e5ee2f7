"""CPU (-m "not gpu"): the float64 restatement of the PoseNet (tests/posecnn_torch.py) against what the reference's own Encoder,
RTHead and refine_rt gave (tests/golden/g38_posecnn.npz, written by tests/golden/gen_golden_posecnn.py); the parameter names of
moda_amd.Encoder + RTHead; checkpoint.build_pose_cnn's prefixes and its refusals by name; the BatchNorm fold; the bindings of the
new entries; the refusals that need no device."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import posecnn_torch as PT
from moda_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("moda_conv2d_nhwc", "moda_conv2d_tile", "moda_maxpool3x3s2_nhwc", "moda_posecnn_input", "moda_posecnn_tail")


@pytest.fixture(scope="module")
def g38():
    return np.load(os.path.join(ROOT, "tests", "golden", "g38_posecnn.npz"))


@pytest.fixture(scope="module")
def state():
    return PT.state_tensors(PT.make_state(PT.SEED))


def close(a, b, tol=1e-10):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b).max()
    assert err <= tol * max(1.0, np.abs(b).max()), err


# ---- the restatement against the reference's float64 records ---------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_equals_the_reference(g38, state, tag):
    x_a, x_b = PT.golden_inputs()
    img = {"a": x_a, "b": x_b}[tag]
    assert np.array_equal(img, g38["x_" + tag])                       # the stored inputs are the seeded ones
    feat, rts, rtk = PT.posenet(state, img, g38["ks"], g38["dataid_" + tag], torch.float64)
    close(feat.numpy(), g38[f"feat_{tag}_64"])
    close(rts.numpy(), g38[f"rts_{tag}_64"])
    close(rtk.numpy(), g38[f"rtk_{tag}_64"])


def test_golden_inputs_are_sparse_and_unit_norm(g38):
    assert g38["x_a"].shape == (3, 16, 112, 112) and g38["x_b"].shape == (2, 16, 100, 123)
    for k in ("x_a", "x_b"):
        n = np.sqrt((g38[k].astype(np.float64) ** 2).sum(1))
        inside = n > 0
        assert 0.05 < inside.mean() < 0.5 and np.abs(n[inside] - 1).max() < 1e-6


# ---- the module's names and the checkpoint loader --------------------------------------------------------------------------------
def _posenet_module():
    import moda_amd
    return torch.nn.Sequential(moda_amd.Encoder((112, 112), in_channels=16, out_channels=128),
                               moda_amd.RTHead(use_quat=True, D=1, in_channels_xyz=128, in_channels_dir=0, out_channels=7, raw_feat=True))


def test_state_dict_keys_are_the_references(g38, state):
    keys = [str(k) for k in g38["keys"]]
    m = _posenet_module()
    assert set(m.state_dict().keys()) == set(keys) and len(keys) == len(m.state_dict())
    assert set(state) == set(keys)
    assert not any(".fc." in k for k in keys)
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == tuple(state[k].shape), k
    m.load_state_dict(state, strict=True)


def test_initialisation_is_deterministic_and_needs_no_torchvision():
    import sys
    import moda_amd
    torch.manual_seed(1)
    a = moda_amd.Encoder((112, 112), in_channels=16)
    torch.manual_seed(2)
    b = moda_amd.Encoder((112, 112), in_channels=16)
    assert all(torch.equal(p, q) for p, q in zip(a.state_dict().values(), b.state_dict().values()))
    assert "torchvision" not in sys.modules
    assert float(a.resnet_conv.resnet.layer3[0].conv1.weight.detach().std()) > 0


@pytest.mark.parametrize("prefix", ["module.nerf_root_rts.", "module.dp_root_rts.", ""])
def test_build_pose_cnn_loads_under_each_prefix(state, prefix):
    from moda_amd import checkpoint
    from moda_amd.pose_cnn import Encoder
    m = checkpoint.build_pose_cnn({prefix + k: v for k, v in state.items()}, device="cpu")
    assert isinstance(m[0], Encoder) and not m.training and m[0].in_channels == 16
    for k, v in m.state_dict().items():
        assert torch.equal(v, state[k]), k


def test_build_pose_cnn_fails_by_name(state):
    from moda_amd import checkpoint
    dropped = {k: v for k, v in state.items() if k != "0.resnet_conv.resnet.layer2.0.downsample.1.running_var"}
    with pytest.raises(KeyError, match=r"layer2\.0\.downsample\.1\.running_var"):
        checkpoint.build_pose_cnn(dropped, device="cpu")
    extra = dict(state)
    extra["0.resnet_conv.resnet.fc.weight"] = torch.zeros(3)
    with pytest.raises(KeyError, match=r"resnet\.fc\.weight"):
        checkpoint.build_pose_cnn(extra, device="cpu")
    with pytest.raises(KeyError, match="conv1.weight"):
        checkpoint.build_pose_cnn({"module.nerf_root_rts.base_rt.se3": torch.zeros(4, 7)}, device="cpu")


# ---- the BatchNorm fold ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key, bn, stride, pad, bias_key", [
    ("0.resnet_conv.resnet.layer2.0.conv1.weight", "0.resnet_conv.resnet.layer2.0.bn1", 2, 1, None),
    ("0.resnet_conv.resnet.layer3.0.downsample.0.weight", "0.resnet_conv.resnet.layer3.0.downsample.1", 2, 0, None),
    ("0.conv1.0.weight", "0.conv1.1", 1, 1, "0.conv1.0.bias"),
])
def test_fold_matches_conv_then_batchnorm_in_float64(state, key, bn, stride, pad, bias_key):
    from moda_amd.pose_cnn import fold_bn
    w = state[key]
    cb = None if bias_key is None else state[bias_key]
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.standard_normal((2, w.shape[1], 7, 6)))
    y = F.conv2d(x, w.double(), None if cb is None else cb.double(), stride, pad)
    y = F.batch_norm(y, state[bn + ".running_mean"].double(), state[bn + ".running_var"].double(), state[bn + ".weight"].double(),
                     state[bn + ".bias"].double(), False, 0.0, 1e-5)
    wf, bf = fold_bn(w, cb, state[bn + ".weight"], state[bn + ".bias"], state[bn + ".running_mean"], state[bn + ".running_var"], 1e-5,
                     cin_pad=w.shape[1] + 16)
    assert wf.dtype == torch.float64 and wf.shape == (w.shape[0], w.shape[2], w.shape[3], w.shape[1] + 16)
    assert float(wf[..., w.shape[1]:].abs().max()) == 0
    got = F.conv2d(x, wf[..., :w.shape[1]].permute(0, 3, 1, 2), bf, stride, pad)
    assert float((got - y).abs().max()) <= 1e-12 * max(1.0, float(y.abs().max()))


# ---- bindings --------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_bound_declared_and_exported():
    import moda_amd
    from moda_amd import build
    hdr = open(os.path.join(ROOT, "include", "moda_hip.h")).read()
    declared = set(re.findall(r"\b(moda_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in _lib.EXPORTS and name in declared and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 11 and lib.moda_abi_version() == 11
    assert "posecnn_kernels.hip" in build.SOURCES
    for name in ("Encoder", "ResNetConv", "build_pose_cnn", "extract_cams", "pose_cnn"):
        assert hasattr(moda_amd, name), name
    from moda_amd import pose_cnn
    for const, macro in ((pose_cnn.K_CHUNK, "MODA_CONV_K_CHUNK"), (pose_cnn.ACT_LEAKY, "MODA_CONV_ACT_LEAKY"), (pose_cnn.TILE_64, "MODA_CONV_TILE_64")):
        assert re.search(rf"#define {macro} {const}\b", hdr), macro


def test_entries_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    EINVAL, ESHAPE = -1, -2
    assert lib.moda_conv2d_nhwc(None, None, None, None, None, 1, 4, 4, 16, 32, 3, 3, 1, 1, 0, 0, None) == EINVAL        # NULL
    assert lib.moda_conv2d_nhwc(None, None, None, None, None, 1, 4, 4, 12, 32, 3, 3, 1, 1, 0, 0, None) == ESHAPE        # Cin % 16
    assert lib.moda_conv2d_nhwc(None, None, None, None, None, 1, 1, 1, 16, 32, 3, 3, 1, 0, 0, 0, None) == ESHAPE        # image < kernel
    assert lib.moda_maxpool3x3s2_nhwc(None, 1, 4, 4, 6, None, None) == ESHAPE                                          # C % 4
    assert lib.moda_posecnn_input(None, 1, 16, 4, 4, 8, 0, None, None) == ESHAPE                                       # Cp < C
    assert lib.moda_posecnn_tail(None, 1, 16, 128, None, None) == EINVAL
    # the tile form is a function of the shape alone: 64 x 64 from 256 workgroups on
    assert lib.moda_conv2d_tile(50 * 56 * 56, 64, 0) == 2 and lib.moda_conv2d_tile(16, 512, 0) == 1 and lib.moda_conv2d_tile(16, 512, 2) == 2
    assert lib.moda_conv2d_tile(64 * 64, 256, 0) == 2 and lib.moda_conv2d_tile(64 * 64 - 64, 256, 0) == 1


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_encoder_refusals():
    import moda_amd
    enc = moda_amd.Encoder((112, 112), in_channels=16).eval()
    good = torch.zeros(1, 16, 112, 112)
    for bad in (torch.zeros(1, 16, 64, 64), torch.zeros(1, 16, 112, 129), torch.zeros(1, 16, 96, 112), torch.zeros(1, 3, 112, 112),
                torch.zeros(16, 112, 112)):
        with pytest.raises(ValueError):
            enc(bad)
    with pytest.raises(RuntimeError, match="CUDA"):
        enc(good)
    with pytest.raises(RuntimeError, match="CUDA"):
        enc(torch.zeros(2, 16, 100, 123))                             # an accepted size
    with pytest.raises(NotImplementedError, match="requires? grad|require grad"):
        enc(good.clone().requires_grad_(True))
    enc.train()
    with pytest.raises(NotImplementedError, match="training"):
        enc(good)
    with pytest.raises(NotImplementedError, match="batch_norm"):
        moda_amd.Encoder((112, 112), in_channels=16, batch_norm=False)
    assert moda_amd.Encoder.map_size(112, 112) == (4, 4) and moda_amd.Encoder.map_size(97, 128) == (4, 4)
    assert moda_amd.Encoder.map_size(96, 112) == (3, 4)


def test_cnn_basis_without_features_is_refused_by_name():
    import moda_amd
    m = _posenet_module().eval()
    with pytest.raises(NotImplementedError, match="Encoder"):
        moda_amd.convert_root_pose(m, torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(1, 4))
    with pytest.raises(NotImplementedError, match="Encoder"):
        moda_amd.compute_rts(m, 4)
    with pytest.raises(NotImplementedError, match="cnn"):
        moda_amd.checkpoint.build_root_pose({"nerf_root_rts.0.conv1.0.weight": torch.zeros(1)}, [0, 4], device="cpu")
