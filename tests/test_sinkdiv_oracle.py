"""CPU checks of the Sinkhorn-divergence restatement (tests/sinkdiv_numpy.py), of the bindings' argument refusals and of the
Python surface that needs no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sinkdiv_numpy as sn
from moda_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE = -1, -2


def family():
    rng = np.random.default_rng(5)
    out = []
    for N, M, target in ((3, 17, 7.3), (25, 200, 7.6), (36, 120, 2.9), (5, 5, 1.9)):
        x, y = sn.with_diameter(sn.gaussian_bones(rng, N), sn.squashed_sphere(rng, M), target)
        out.append((x, y))
    return out


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def test_autograd_through_the_detach_pattern_gives_the_analytic_gradients():
    for x, y in family():
        ref = sn.sinkdiv(x, y)
        tx, ty = torch.tensor(x, requires_grad=True), torch.tensor(y, requires_grad=True)
        loss, info = sn.sinkdiv_torch(tx, ty)
        gx, gy = torch.autograd.grad(loss, (tx, ty))
        assert info["n"] == ref["n"]
        assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12 * abs(ref["loss"])
        assert rel(gx.numpy(), ref["grad_x"]) <= 1e-12 and rel(gy.numpy(), ref["grad_y"]) <= 1e-12


def test_loss_of_a_cloud_with_itself_is_zero():
    for x, _ in family():
        r = sn.sinkdiv(x, x.copy())
        assert abs(r["loss"]) <= 1e-12                           # absolute (the four matrices coincide, and so do the potentials)


def test_loss_is_invariant_under_a_common_translation():
    for x, y in family():
        t = np.array([0.5, -1.25, 2.0])                          # exactly representable: the differences do not change
        a, b = sn.sinkdiv(x, y), sn.sinkdiv(x + t, y + t)
        assert a["n"] == b["n"]
        assert abs(a["loss"] - b["loss"]) <= 1e-9 * abs(a["loss"])
        assert rel(b["grad_x"], a["grad_x"]) <= 1e-9


def test_schedule_length():
    for x, y in family():
        r = sn.sinkdiv(x, y)
        f = sn.frac_log2(r["d"])
        assert 0.05 <= f <= 0.95
        assert r["n"] == 2 + int(np.ceil(np.log2(r["d"] / 0.05)))
        assert r["eps"][0] == r["d"] ** 2 and r["eps"][-1] == 0.05 ** 2
        assert abs(r["eps"][1] - r["eps"][0]) <= 1e-13 * r["eps"][0]            # the second entry is d^2 again, as exp(2 ln d)
    for d, n in ((0.05 * 2 ** 5.5, 8), (0.05 * 2 ** 7.5, 10), (0.05 * 2 ** 11.5, 14)):
        assert len(sn.epsilon_schedule(d, 0.05, 0.5)) == n


def test_entries_are_bound_and_declared():
    hdr = open(os.path.join(ROOT, "include", "moda_hip.h")).read()
    declared = set(re.findall(r"\b(moda_[a-z0-9_]+)\s*\(", hdr))
    for name in ("moda_sinkdiv_ws_bytes", "moda_sinkdiv"):
        assert name in _lib.EXPORTS and name in declared, name
    assert _lib.ABI_VERSION == 11 and _lib.load().moda_abi_version() == 11
    from moda_amd import build
    assert "sinkdiv_kernels.hip" in build.SOURCES
    assert "MODA_SINKDIV_MAX_STEPS 24" in hdr and "MODA_SINKDIV_MAX_POINTS 4096" in hdr


def test_entries_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    assert lib.moda_sinkdiv_ws_bytes(36, 1000) == 4 * (32 + 5 * 1036)
    assert lib.moda_sinkdiv_ws_bytes(0, 8) == 0 and lib.moda_sinkdiv_ws_bytes(4000, 97) == 0
    buf = (ctypes.c_float * 64)()
    st = (ctypes.c_int32 * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    s = ctypes.cast(st, ctypes.c_void_p)
    ok = dict(x=p, y=p, N=4, M=4, blur=0.05, scaling=0.5, diameter=0.0, ws=p, loss=p, gx=p, gy=None, status=s)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.moda_sinkdiv(a["x"], a["y"], a["N"], a["M"], a["blur"], a["scaling"], a["diameter"], a["ws"], a["loss"], a["gx"],
                                a["gy"], a["status"], None)

    for name in ("x", "y", "ws", "loss", "gx", "status"):
        assert call(**{name: None}) == EINVAL, name
    assert call(N=0) == EINVAL and call(M=0) == EINVAL and call(blur=0.0) == EINVAL and call(blur=-1.0) == EINVAL
    assert call(scaling=1.0) == EINVAL and call(scaling=0.0) == EINVAL
    assert call(N=4000, M=97) == ESHAPE and call(N=1, M=4096) == ESHAPE            # refused before anything is launched


def test_samples_loss_refuses_each_unserved_option_by_name():
    from moda_amd.samples_loss import SamplesLoss
    import moda_amd
    assert moda_amd.SamplesLoss is SamplesLoss
    for kw, name in ((dict(loss="energy"), "loss"), (dict(p=1), "p"), (dict(reach=1.0), "reach"), (dict(debias=False), "debias"),
                     (dict(potentials=True), "potentials"), (dict(backend="online"), "backend"), (dict(cost="SqDist(X,Y)"), "cost")):
        with pytest.raises(NotImplementedError, match=name):
            SamplesLoss(**kw)
    loss = SamplesLoss("sinkhorn", p=2, blur=.05)
    assert loss.blur == 0.05 and loss.scaling == 0.5 and loss.diameter is None
    x = torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match="weights"):
        loss(torch.ones(4) / 4, x, torch.ones(4) / 4, x)
    with pytest.raises(NotImplementedError, match="batched"):
        loss(x[None], x[None])
    with pytest.raises(NotImplementedError, match="D="):
        loss(torch.zeros(4, 2), torch.zeros(4, 2))
    with pytest.raises(NotImplementedError, match="device"):
        loss(x, x)
    with pytest.raises(ValueError):
        SamplesLoss(blur=0.0)
    with pytest.raises(ValueError):
        SamplesLoss(scaling=1.0)


def test_bone_loc_loss_skips_a_degenerate_mesh():
    from moda_amd import loss_utils as LU, synth

    class Mesh:
        pass
    m = Mesh()
    m.vertices, m.faces = synth.make_rest_mesh(1)                # 42 vertices
    assert len(m.vertices) == 42
    assert LU.bone_loc_loss(None, m) is None                     # before the model is touched: a shape test
    m.vertices = np.zeros((100, 3))
    assert LU.bone_loc_loss(None, m) is None
    v, f = synth.make_rest_mesh(2)
    assert v.shape == (162, 3) and f.shape == (320, 3) and v.dtype == np.float32 and f.dtype == np.int32
    assert f.min() == 0 and f.max() == 161


def test_forward_loss_contract_of_bone_loc():
    from moda_amd import loss_utils as LU
    with pytest.raises(NotImplementedError, match="bone_loc_reg") as e:
        LU.forward_loss({}, dict())
    assert "bone_loc=" in str(e.value) and "bone_loc_loss" in str(e.value)
    # bone_loc=False is the reference's skip: the call gets past that check (and then misses its inputs)
    with pytest.raises(KeyError):
        LU.forward_loss({}, dict(), bone_loc=False)
    with pytest.raises(NotImplementedError, match="ft_cse"):
        LU.forward_loss({}, dict(ft_cse=True), bone_loc=False)
    assert LU.LOSS_OPTS["bone_loc_reg"] == 0.1
