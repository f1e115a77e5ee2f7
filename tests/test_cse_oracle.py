"""CPU checks of the DensePose-CSE matching (moda_amd/cse.py, csrc/cse_kernels.hip): the float64 restatement tests/cse_numpy.py
against the reference's own records in tests/golden/g34_cse.npz, the wiring of the new entries, and the refusals.

`test_reference_fp32_inside_bound_*` are SELF-CHECKS OF THE ORACLE, not of the product: the reference's fp32 records must lie
inside the error bound the oracle states for its float64 values (if one does not, the bound is wrong).  The GPU tests
(tests/test_gpu_cse.py) hold the kernels to that oracle and those bounds."""
import os
import re

import numpy as np
import pytest
import torch

import cse_numpy as O
from moda_amd import _lib, build, cse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "g34_cse.npz"))
NEW_ENTRIES = ("moda_feat_argmax", "moda_feat_argmax_splits", "moda_grid_resample", "moda_ood_error")
RS = [str(n) for n in G["rs/names"]]
OOD = [str(n) for n in G["ood/names"]]
FLOW = [str(n) for n in G["flow/names"]]


def rs_inputs(name):
    return G["rs/" + str(G[f"rs/{name}/src"])], G[f"rs/{name}/bbox"], G["rs/kaug"], int(G[f"rs/{name}/target"])


def live_rows(name):
    """The batch rows whose coordinates are numbers: in the `mixed` case row 0 has a zero box on the grid branch, its affine is
    1 / 0, and what F.grid_sample makes of NaN coordinates is not specified (the kernel writes zeros, see cse.py)."""
    _, bbox, _, _ = rs_inputs(name)
    return [i for i in range(bbox.shape[0]) if np.abs(bbox).sum() == 0 or np.abs(bbox[i]).sum() != 0]


@pytest.mark.parametrize("name", RS)
def test_resample_oracle_matches_reference_f64(name):
    feats, bbox, kaug, target = rs_inputs(name)
    out, _ = O.resample_dp(feats, bbox, kaug, target)
    rows = live_rows(name)
    assert np.abs(out[rows] - G[f"rs/{name}/out64"][rows]).max() <= 1e-10
    if f"rs/{name}/n64" in G.files:
        outn, _ = O.resample_dp(feats, bbox, kaug, target, normalize=True)
        assert np.abs(outn[rows] - G[f"rs/{name}/n64"][rows]).max() <= 1e-10
    d2r = O.bbox_dp2rnd(bbox, kaug)
    assert np.abs(d2r - G[f"rs/{name}/d2r64"]).max() <= 1e-10


@pytest.mark.parametrize("name", RS)
def test_reference_fp32_inside_bound_resample(name):
    feats, bbox, kaug, target = rs_inputs(name)
    out, bound = O.resample_dp(feats, bbox, kaug, target)
    rows = live_rows(name)
    assert (np.abs(G[f"rs/{name}/out32"][rows] - out[rows]) <= bound[rows]).all()
    if f"rs/{name}/n32" in G.files:
        outn, boundn = O.resample_dp(feats, bbox, kaug, target, normalize=True)
        assert (np.abs(G[f"rs/{name}/n32"][rows] - outn[rows]) <= boundn[rows]).all()


def test_mixed_batch_takes_the_grid_branch():
    feats, bbox, kaug, target = rs_inputs("mixed")
    interp, _ = O.resample(feats, target, target, "interp")
    assert np.abs(G["rs/mixed/out64"][1] - interp[1]).max() > 1e-3           # row 1 is not the plain resize
    assert np.abs(O.resample_dp(feats, bbox, kaug, target)[0][0]).max() == 0  # the degenerate row: zeros


@pytest.mark.parametrize("name", OOD)
def test_ood_oracle_matches_reference(name):
    feats, embed, dp_idx = G[f"ood/{name}/feats"], G[f"ood/{name}/embed"], G[f"ood/{name}/dp_idx"]
    valid, err, bound, idx = O.ood_check_cse(feats, embed, dp_idx)
    assert np.array_equal(idx, G[f"ood/{name}/idx64"])
    want = G[f"ood/{name}/err64"]
    assert np.array_equal(np.isnan(err), np.isnan(want)) and np.isnan(want[2])
    assert np.nanmax(np.abs(err - want)) <= 1e-10
    assert np.array_equal(valid, G[f"ood/{name}/valid64"]) and not valid[2]
    # self-check of the bound: the reference's fp32 record (its mean is an fp32 sum: n u more)
    n = feats.shape[-1] ** 2
    assert np.nanmax(np.abs(G[f"ood/{name}/err32"] - want) - (bound + n * O.U32 * np.abs(want))) <= 0
    assert np.array_equal(G[f"ood/{name}/valid32"], valid)


@pytest.mark.parametrize("name", FLOW)
def test_flow_oracle_matches_reference(name):
    a, b = G[f"flow/{name}/a"], G[f"flow/{name}/b"]
    fa, ba, fb, bb, ma, mb, s = O.compute_flow_cse(a, b, G[f"flow/{name}/warp_a"], G[f"flow/{name}/warp_b"], int(G[f"flow/{name}/img_size"]))
    assert np.array_equal(ma, G[f"flow/{name}/ma64"]) and np.array_equal(mb, G[f"flow/{name}/mb64"])
    assert np.abs(fa - G[f"flow/{name}/fa64"]).max() <= 1e-10 and np.abs(fb - G[f"flow/{name}/fb64"]).max() <= 1e-10
    assert (np.abs(G[f"flow/{name}/fa32"] - fa) <= ba).all() and (np.abs(G[f"flow/{name}/fb32"] - fb) <= bb).all()
    qa, qb = a.reshape(16, -1).T, b.reshape(16, -1).T
    assert (O.margin(s) > 8 * O.argmax_bound(qa, qb)).all() and (O.margin(s.T) > 8 * O.argmax_bound(qb, qa)).all()


@pytest.mark.parametrize("inn,out", [(512, 112), (256, 112), (112, 112), (7, 5)])
def test_nearest_index_rule(inn, out):
    assert np.array_equal(O.nearest_index(out, inn), G[f"nearest/{inn}_{out}"])


def test_argmax_rule_ties_nan_zero():
    s = np.asarray([[1.0, 3.0, 3.0, 2.0], [0.0, -0.0, -1.0, 0.0], [-0.0, 0.0, -1.0, -2.0], [1.0, np.nan, 5.0, np.nan],
                    [-np.inf, -np.inf, -np.inf, -np.inf]])
    assert O.argmax_rule(s).tolist() == [1, 0, 0, 1, 0]
    assert O.argmax_rule(s).tolist() == torch.from_numpy(s).argmax(1).tolist()


# ---- wiring ---------------------------------------------------------------------------------------------------------------
def test_source_is_built():
    assert "cse_kernels.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "cse_kernels.hip"))


def test_entries_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "moda_hip.h")).read()
    declared = set(re.findall(r"\b(moda_[a-z0-9_]+)\s*\(", hdr))
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.moda_abi_version() == _lib.ABI_VERSION
    assert (cse.CHANNELS, cse.QUERY_TILE, cse.CAND_TILE, cse.OOD_MAX_BLOCKS) == tuple(
        int(re.search(rf"#define {n}\s+(\d+)", hdr).group(1)) for n in ("MODA_CSE_CHANNELS", "MODA_CSE_QUERY_TILE", "MODA_CSE_CAND_TILE", "MODA_OOD_MAX_BLOCKS"))


def test_split_plan():
    build.build(verbose=False)
    T = cse.CAND_TILE
    assert cse.argmax_splits(8, 27554, 12544) == (1, 12544)               # 1728 workgroups already
    n, rng = cse.argmax_splits(1, 27554, 12544)
    assert n > 1 and rng % T == 0 and (n - 1) * rng < 12544 <= n * rng
    assert cse.argmax_splits(1, 64, 3 * T + 1, 2) == (2, 2 * T)
    assert cse.argmax_splits(1, 64, T, 5) == (1, T)                        # never more ranges than tiles
    assert cse.argmax_splits(1, 64, 4 * T, 3) == (2, 2 * T)               # no empty range


def test_public_names():
    import moda_amd
    for n in ("bbox_dp2rnd", "resample_dp", "ood_check_cse", "feat_argmax", "match2coords", "match2flo", "compute_flow_cse"):
        assert getattr(moda_amd, n) is getattr(cse, n)


def test_cpu_helpers_match_reference_records():
    bbox, kaug = torch.from_numpy(G["rs/grid/bbox"]), torch.from_numpy(G["rs/kaug"])
    assert np.abs(cse.bbox_dp2rnd(bbox, kaug).numpy() - G["rs/grid/d2r32"]).max() <= 1e-6 * np.abs(G["rs/grid/d2r32"]).max()
    m = torch.tensor([0, 5, 17, 24])
    assert cse.match2coords(m, 5).tolist() == [[0, 0], [0, 1], [2, 3], [4, 4]]


# ---- refusals -------------------------------------------------------------------------------------------------------------
def _args():
    f = torch.zeros(2, 16, 8, 8)
    return f, torch.zeros(2, 4), torch.ones(2, 4), torch.zeros(30, 16), torch.zeros(2, 8, 8, dtype=torch.int64), torch.eye(3)


def test_refuses_cpu_tensors():
    f, bbox, kaug, emb, dpi, warp = _args()
    for call in (lambda: cse.resample_dp(f, bbox, kaug, 4), lambda: cse.ood_check_cse(f, emb, dpi),
                 lambda: cse.feat_argmax(emb, emb), lambda: cse.compute_flow_cse(f[0], f[1], warp, warp, 64),
                 lambda: cse.match2flo(torch.zeros(64, dtype=torch.int64), 8, 64, warp, warp, "cpu")):
        with pytest.raises(RuntimeError, match="CUDA"):
            call()


def test_refuses_dtype_and_layout():
    f, bbox, kaug, emb, dpi, warp = _args()
    for bad in (f.double(), f.half(), f.permute(0, 1, 3, 2)[:, :, :, ::2], f.transpose(2, 3)):
        with pytest.raises(ValueError):
            cse.resample_dp(bad, bbox, kaug, 4)
    with pytest.raises(ValueError):
        cse.ood_check_cse(f.double(), emb, dpi)
    with pytest.raises(ValueError):
        cse.ood_check_cse(f, emb.double(), dpi)
    with pytest.raises(ValueError):
        cse.compute_flow_cse(f[0].double(), f[1], warp, warp, 64)
    with pytest.raises(ValueError):
        cse.compute_flow_cse(f[0], f[1].transpose(1, 2), warp, warp, 64)


def test_refuses_other_channel_counts():
    f, bbox, kaug, emb, dpi, warp = _args()
    with pytest.raises(NotImplementedError):
        cse.resample_dp(torch.zeros(2, 8, 8, 8), bbox, kaug, 4)
    with pytest.raises(NotImplementedError):
        cse.ood_check_cse(torch.zeros(2, 32, 8, 8), emb, dpi)
    with pytest.raises(NotImplementedError):
        cse.ood_check_cse(f, torch.zeros(30, 8), dpi)
    with pytest.raises(NotImplementedError):
        cse.compute_flow_cse(torch.zeros(3, 8, 8), torch.zeros(3, 8, 8), warp, warp, 64)
    with pytest.raises(NotImplementedError):
        cse.feat_argmax(torch.zeros(4, 3), torch.zeros(5, 3))


def test_refuses_non_square_images():
    f, bbox, kaug, emb, dpi, warp = _args()
    with pytest.raises(ValueError, match="square"):
        cse.ood_check_cse(torch.zeros(2, 16, 8, 6), emb, dpi)
    with pytest.raises(ValueError, match="square"):
        cse.compute_flow_cse(torch.zeros(16, 6, 8), torch.zeros(16, 6, 8), warp, warp, 64)


def test_refuses_grad():
    f, bbox, kaug, emb, dpi, warp = _args()
    g = f.clone().requires_grad_()
    with pytest.raises(NotImplementedError, match="grad"):
        cse.resample_dp(g, bbox, kaug, 4)
    with pytest.raises(NotImplementedError, match="grad"):
        cse.ood_check_cse(g, emb, dpi)
    with pytest.raises(NotImplementedError, match="grad"):
        cse.ood_check_cse(f, emb.clone().requires_grad_(), dpi)
    with pytest.raises(NotImplementedError, match="grad"):
        cse.compute_flow_cse(g[0], f[1], warp, warp, 64)
    with pytest.raises(NotImplementedError, match="grad"):
        cse.feat_argmax(emb.clone().requires_grad_(), emb)
