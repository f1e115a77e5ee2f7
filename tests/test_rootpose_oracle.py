"""CPU (-m "not gpu"): the float64 restatement of the root-pose chain (tests/rootpose_numpy.py) against what the reference's own
modules gave (tests/golden/g32_root_pose.npz, written by tests/golden/gen_golden_root_pose.py), its hand-written gradients against
central differences, the bindings of the new entries, and RTExpMLP's state-dict keys.

The tests of the second group (finite differences, the magnification identity, id_rows_sum's order, the MLP's gradient) are
self-checks of the oracle: they run tests/rootpose_numpy.py alone and do not depend on the package, so unlike the others they do
not tell a tree with the root-pose kernels from one without."""
import os
import re

import numpy as np
import pytest

import rootpose_cases as C
import rootpose_numpy as rn
from moda_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("moda_root_pose", "moda_id_rows_sum", "moda_ray_cams")
CLAMP64 = 1e-4            # the reference's float64 run clamps at the double 1e-4


@pytest.fixture(scope="module")
def g32():
    return np.load(os.path.join(ROOT, "tests", "golden", "g32_root_pose.npz"))


def close(a, b, tol=1e-10):
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b).max()
    assert err <= tol * max(1.0, np.abs(b).max()), err


# ---- the restatement against the reference's float64 records ---------------------------------------------------------------------
@pytest.mark.parametrize("tag,n_out", [("rthead_q", 7), ("rthead_w", 6)])
def test_rthead_restatement_equals_the_reference(g32, tag, n_out):
    p = C.head_params(tag, n_out)
    rows = rn.mlp(p, g32["x"])
    g4 = rn.rts12_bwd(g32[tag + "_w"].astype(np.float64))
    res = rn.root_pose(delta=rows, raw="none", g=g4, clamp=CLAMP64)
    close(rn.rts12(res["rtk"]), g32[tag + "_out_64"])
    _, grads = rn.mlp(p, g32["x"], g=res["d_delta"])
    close(grads["d_x"], g32[tag + "_d_x_64"])
    close(grads["rgb.0.weight"], g32[tag + "_d_rgb_64"])


@pytest.mark.parametrize("tag,delta", [("exp_q", False), ("exp_w", True)])
def test_rtexplicit_restatement_equals_the_reference(g32, tag, delta):
    se3 = C.se3_table(delta, 8)
    res = rn.root_pose(se3=se3, ids=C.EDGE_IDS, raw="none", g=rn.rts12_bwd(g32[tag + "_w"].astype(np.float64)), clamp=CLAMP64)
    close(rn.rts12(res["rtk"]), g32[tag + "_out_64"])
    close(res["d_se3"], g32[tag + "_d_se3_64"])


@pytest.mark.parametrize("tag,delta", [("expmlp_q", False), ("expmlp_w", True)])
def test_rtexpmlp_restatement_equals_the_reference(g32, tag, delta):
    sd = C.expmlp_state(delta)
    mlp_p = {k[len("mlp_rt."):]: v for k, v in sd.items() if k.startswith("mlp_rt.")}
    code = g32[tag + "_code_32"].astype(np.float64)
    rows = rn.mlp(mlp_p, code)
    res = rn.root_pose(se3=sd["base_rt.se3"], ids=C.IDS, delta=rows, raw="none",
                       g=rn.rts12_bwd(g32[tag + "_w"].astype(np.float64)), clamp=CLAMP64)
    close(rn.rts12(res["rtk"]), g32[tag + "_out_64"])
    close(res["d_se3"], g32[tag + "_d_se3_64"])
    _, grads = rn.mlp(mlp_p, code, g=res["d_delta"])
    close(grads["rgb.0.weight"], g32[tag + "_d_rgb_64"])
    assert np.all(res["d_se3"][[1, 2, 5, 10, 63]] == 0)                       # frames absent from the batch
    # the reference's own fp32 run lies within a few of its recorded errors of the restatement
    assert np.abs(g32[tag + "_out_32"] - rn.rts12(res["rtk"])).max() <= 1.01 * float(g32[tag + "_dref_out"])


def test_refine_and_ray_cams_restatements_equal_the_reference(g32):
    raw, root = g32["refine_rt_raw"].astype(np.float64), g32["refine_root"].astype(np.float64)
    R, t = root[:, 0, :9].reshape(-1, 3, 3), root[:, 0, 9:]
    close(rn.refine_rt(raw, R, t), g32["refine_out_64"])
    assert np.array_equal(rn.create_base_se3(3), g32["base_se3"].astype(np.float64))
    kaug = g32["kaug"].astype(np.float64)
    res = rn.ray_cams(raw, kaug, g32["cams_wR"].astype(np.float64), g32["cams_wT"].astype(np.float64), g32["cams_wK"].astype(np.float64))
    close(res["Rmat"], g32["cams_out_64"])
    close(res["Tmat"], g32["cams_Tmat_64"])
    close(res["Kinv"], g32["cams_Kinv_64"])
    close(res["d_rtk"], g32["cams_d_rtk_64"])
    krow = g32["cams_d_rtk_64"][:, 3]                                          # the K row on its own scale (1 / fx^2 and smaller)
    assert np.abs(res["d_rtk"][:, 3] - krow).max() <= 1e-10 * np.abs(krow).max()
    close(rn.K2inv(kaug), g32["cams_K2inv_64"])
    close(rn.Kmatinv(rn.K2mat(raw[:, 3])), g32["cams_Kmatinv_64"])
    assert np.array_equal(rn.mat2K(rn.K2mat(raw[:, 3])), raw[:, 3])


# ---- hand gradients against central differences ----------------------------------------------------------------------------------
def _fd(f, x, idx, h=1e-6):
    p, m = x.copy(), x.copy()
    p[idx] += h
    m[idx] -= h
    return (f(p) - f(m)) / (2 * h)


@pytest.mark.parametrize("cols,dcols,raw", [(7, 6, "base"), (6, 7, "rows"), (6, 6, "by_id"), (7, None, "rows"), (None, 6, "base")])
def test_tail_gradients_against_finite_differences(cols, dcols, raw):
    rng = np.random.default_rng(5)
    n, T = 6, 4
    ids = np.asarray([0, 3, 3, 1, 3, 0])
    se3 = None if cols is None else rng.normal(size=(T, cols)) * 0.7
    delta = None if dcols is None else rng.normal(size=(n, dcols)) * 0.7
    if cols == 6:
        se3[1, 3:] *= 0.005                                   # below the clamp
    rt_raw = None
    if raw != "base":
        rt_raw = np.zeros((T if raw == "by_id" else n, 3, 4))
        rt_raw[:, :3, :3] = rn.so3_exp(rng.normal(size=(len(rt_raw), 3)))
        rt_raw[:, :3, 3] = rng.normal(size=(len(rt_raw), 3))
    ks, dataid = rng.normal(size=(2, 4)) + 5, np.asarray([0, 1, 1, 0, 1, 1])
    w = rng.normal(size=(n, 4, 4))
    kw = dict(ids=ids, rt_raw=rt_raw, raw=raw, obj_scale=1.7, dataid=dataid)
    f = lambda se3_, delta_, ks_: float((w * rn.root_pose(se3=se3_, delta=delta_, ks=ks_, **kw)["rtk"]).sum())
    res = rn.root_pose(se3=se3, delta=delta, ks=ks, g=w, **kw)
    if se3 is not None:
        # with both given the forward VALUE is x * 10 - x * 9 = x while the gradient is the magnified one (nerf.py:456's detach)
        mag = 10.0 if delta is not None else 1.0
        for idx in [(0, 0), (3, 2), (3, 3), (3, cols - 1), (1, 4), (2, 3)]:
            fd = mag * _fd(lambda x: f(x, delta, ks), se3, idx)
            assert abs(fd - res["d_se3"][idx]) < 1e-7 + 1e-6 * abs(fd), idx
        assert np.all(res["d_se3"][2] == 0)
    if delta is not None:
        for idx in [(0, 0), (2, 3), (4, dcols - 1), (5, 1)]:
            fd = _fd(lambda x: f(se3, x, ks), delta, idx)
            assert abs(fd - res["d_delta"][idx]) < 1e-7 + 1e-6 * abs(fd), idx
    for idx in [(0, 0), (1, 3)]:
        assert abs(_fd(lambda x: f(se3, delta, x), ks, idx) - res["d_ks"][idx]) < 1e-7


def test_magnification_is_ten_times_the_exp_basis_gradient():
    rng = np.random.default_rng(6)
    se3, ids, w = rng.normal(size=(3, 7)), np.asarray([0, 2, 2, 1]), rng.normal(size=(4, 4, 4))
    zero = np.zeros((4, 6))                                   # a zero delta: identity below the clamp
    a = rn.root_pose(se3=se3, ids=ids, delta=zero, raw="base", g=w)
    b = rn.root_pose(se3=se3, ids=ids, raw="base", g=w)
    assert np.abs(a["rtk"] - b["rtk"]).max() < 1e-15
    assert np.abs(a["d_se3"] - 10 * b["d_se3"]).max() < 1e-12 * np.abs(b["d_se3"]).max() * 10


def test_ray_cams_and_raycast_gradients_against_finite_differences():
    rng = np.random.default_rng(7)
    n, ns = 3, 5
    rtk = rng.normal(size=(n, 4, 4))
    rtk[:, 3] = np.abs(rtk[:, 3]) * 50 + [300, 500, 200, 250]
    kaug = np.abs(rng.normal(size=(n, 4))) + 0.5
    xys = rng.uniform(0, 512, size=(n, ns, 2))
    wd, wo = rng.normal(size=(n, ns, 3)), rng.normal(size=(n, ns, 3))

    def f(r):
        c = rn.ray_cams(r, kaug)
        rays = rn.raycast(xys, c["Rmat"], c["Tmat"], c["Kinv"])
        return float((wd * rays["rays_d"]).sum() + (wo * rays["rays_o"]).sum())
    c = rn.ray_cams(rtk, kaug)
    rays = rn.raycast(xys, c["Rmat"], c["Tmat"], c["Kinv"], wd, wo)
    d = rn.ray_cams(rtk, kaug, rays["d_Rmat"], rays["d_Tmat"], rays["d_Kinv"])["d_rtk"]
    for idx in [(0, 0, 0), (1, 2, 1), (2, 1, 3), (0, 3, 0), (1, 3, 1), (2, 3, 2), (0, 3, 3)]:
        fd = _fd(f, rtk, idx, h=1e-5)
        assert abs(fd - d[idx]) < 1e-8 + 1e-6 * abs(fd), idx


def test_mlp_gradient_against_finite_differences():
    p = {k: v.astype(np.float64) for k, v in C.head_params("rthead_w", 6).items()}
    x = C.synth.normal(C.SEED, "g32/x", (3, C.CODE)).astype(np.float64)
    w = np.random.default_rng(8).normal(size=(3, 6))
    _, grads = rn.mlp(p, x, g=w)
    for name, idx in (("rgb.0.weight", (2, 5)), ("xyz_encoding_5.0.weight", (7, 200)), ("xyz_encoding_1.0.bias", (3,))):
        def f(v, name=name):
            return float((w * rn.mlp({**p, name: v}, x)).sum())
        fd = _fd(f, p[name], idx)
        assert abs(fd - grads[name][idx]) < 1e-8 + 1e-6 * abs(fd), name
    fd = _fd(lambda v: float((w * rn.mlp(p, v)).sum()), x, (1, 17))
    assert abs(fd - grads["d_x"][1, 17]) < 1e-8 + 1e-6 * abs(fd)


def test_id_rows_sum_order_and_refusals():
    rows = np.arange(12, dtype=np.float64).reshape(6, 2)
    out = rn.id_rows_sum(rows, [2, -1, 2, 5, 0, 2], 4)
    assert np.array_equal(out, [[8, 9], [0, 0], [0 + 4 + 10, 1 + 5 + 11], [0, 0]])


# ---- bindings and the module's keys ----------------------------------------------------------------------------------------------
def test_new_entries_are_bound_and_declared():
    hdr = open(os.path.join(ROOT, "include", "moda_hip.h")).read()
    declared = set(re.findall(r"\b(moda_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in _lib.EXPORTS and name in declared and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 11 and lib.moda_abi_version() == 11
    assert "additive entries of ABI 11" in hdr
    from moda_amd import build
    assert "rootpose_kernels.hip" in build.SOURCES


def test_entries_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    EINVAL = -1
    z = [None] * 7
    assert lib.moda_root_pose(None, 0, 0, None, 0, 4, None, 0, None, 1, 0, 1.0, None, None, 0, 0, 4, *z) == EINVAL      # no status
    assert lib.moda_id_rows_sum(None, None, 0, 4, 4, 9, None, 0, None) == EINVAL                                         # C > 8
    assert lib.moda_id_rows_sum(None, None, 0, 4, 4, 7, None, 96, None) == EINVAL                                        # lanes % 64
    assert lib.moda_ray_cams(None, None, 4, *([None] * 8)) == EINVAL
    assert lib.moda_root_pose(None, 0, 0, None, 0, 0, None, 0, None, 1, 0, 1.0, None, None, 0, 0, 4, *z) == 0            # no rows


def test_rtexpmlp_state_dict_keys_are_the_references(g32):
    import torch
    from moda_amd import feeders as FD
    m = FD.RTExpMLP(C.T, C.NUM_FREQS, C.CODE, np.asarray(C.DATA_OFFSET))
    keys = [str(k) for k in g32["expmlp_keys"]]
    assert len(keys) == 55 and list(m.state_dict().keys()) == keys
    assert set(C.expmlp_state(False)) == set(keys)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in C.expmlp_state(False).items()}, strict=True)
    assert m.delta_rt[0] is m.root_code and m.delta_rt[1] is m.mlp_rt
    assert all(float(l.bias.abs().max()) == 0 for l in FD.RTHead(use_quat=True, out_channels=7, raw_feat=True, **C.HEAD_KW).modules()
               if isinstance(l, torch.nn.Linear))
    for uq in (True, False):
        assert FD.RTHead(use_quat=uq, out_channels=7 if uq else 6, raw_feat=True, **C.HEAD_KW).num_output == (7 if uq else 6)
    assert FD.RTExplicit(5, delta=True).se3.shape == (5, 6) and FD.RTExplicit(5).se3.shape == (5, 7)


def test_cnn_basis_is_refused_by_name():
    from moda_amd import feeders as FD, root_pose
    import torch

    class Encoder(torch.nn.Module):
        pass
    head = FD.RTHead(use_quat=True, D=1, W=16, in_channels_xyz=8, in_channels_dir=0, out_channels=7, raw_feat=True)
    with pytest.raises(NotImplementedError, match="Encoder"):
        root_pose.compute_rts(torch.nn.Sequential(Encoder(), head), 4)
