"""CPU checks of the frame-pair preparation (moda_amd/frame_pairs.py, csrc/framepair_kernels.hip): the float64 restatement
tests/framepair_numpy.py against the reference's own records in tests/golden/g35_frame_pairs.npz (made with the oracle's sampler
standing in for cv2.remap, so everything but the sampler is pinned to a reference run), the wiring of the new entries, the
refusals, and the cap on the oracle's exemptions.  The GPU tests (tests/test_gpu_framepair.py) hold the kernels to this oracle."""
import os
import re

import numpy as np
import pytest
import torch

import framepair_numpy as O
from moda_amd import _lib, build, frame_pairs as FP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "g35_frame_pairs.npz"))
NAMES = [str(n) for n in G["names"]]
NEW_ENTRIES = ("moda_mask_bbox", "moda_crop_params", "moda_crop_remap", "moda_flow_process", "moda_remap")
EXEMPT_CAP = 0.01


def oracle_params(name):
    S = int(G[f"{name}/img_size"])
    box, _ = O.mask_bbox(G[f"{name}/masks"])
    (kaug, aff, status), _ = O.compute_crop_params(box, S)
    return S, kaug, aff, status


@pytest.mark.parametrize("name", NAMES)
def test_crop_params_match_reference_bit_for_bit(name):
    S, kaug, aff, status = oracle_params(name)
    assert status.tolist() == [0, 0]
    assert np.array_equal(aff, G[f"{name}/kaug"])                          # float64, exactly
    assert np.array_equal(kaug, G[f"{name}/kaug"].astype(np.float32))
    for k in range(2):                                                     # hp0 of the reference is an np.dot: the same bits
        x, y = O.crop_coords(aff[k], S)
        assert np.array_equal(x, G[f"{name}/x0"][k]) and np.array_equal(y, G[f"{name}/y0"][k])


@pytest.mark.parametrize("name", NAMES)
def test_flow_process_matches_reference(name):
    S, _, aff, _ = oracle_params(name)
    (flow, occ), (b_flow, b_occ), exempt = O.flow_process(G[f"{name}/flow_c"], aff, S)
    assert (np.abs(flow - G[f"{name}/flow"]) <= b_flow).all()
    keep = ~exempt
    assert (np.abs(occ - G[f"{name}/occ"])[keep] <= b_occ[keep]).all()
    assert (occ > 0).mean() > 0.2 and (occ == 0).mean() > 0.05           # the case exercises both sides of the threshold


@pytest.mark.parametrize("name", NAMES)
def test_exemptions_stay_under_the_cap(name):
    S, _, aff, _ = oracle_params(name)
    _, _, exempt = O.flow_process(G[f"{name}/flow_c"], aff, S)
    assert exempt.reshape(exempt.shape[0], -1).mean(1).max() <= EXEMPT_CAP
    crop, cb = O.crop_frames(aff, S, flow=G[f"{name}/flow_raw"])           # the chain: the crop's bound handed on
    _, _, ex2 = O.flow_process(crop["flow"].astype(np.float32), aff, S, cb["flow"] + O.U32 * np.abs(crop["flow"]))
    assert ex2.reshape(ex2.shape[0], -1).mean(1).max() <= EXEMPT_CAP


def test_literal_replay_of_the_two_bodies():
    """compute_crop_params and the flow re-expression replayed with plain numpy (np.dot, np.linalg.inv) on one case: the closed
    form of the oracle differs from the inverse only inside the stated bound."""
    name = NAMES[-1]                                                       # the non-dyadic size
    S, _, aff, _ = oracle_params(name)
    x0, y0 = np.meshgrid(range(S), range(S))
    hp, mats = [], []
    for k in range(2):
        Bm = np.asarray([[aff[k][0], 0, aff[k][2]], [0, aff[k][1], aff[k][3]], [0, 0, 1]]).T
        hp.append(np.dot(np.stack([x0, y0, np.ones_like(x0)], -1), np.eye(3).dot(Bm)))
        mats.append(Bm)
    fc = G[f"{name}/flow_c"]
    (flow, _), (b_flow, _), _ = O.flow_process(fc, aff, S)
    for k in range(2):
        fl = fc[k].transpose(1, 2, 0).copy()
        c = np.concatenate([fl + hp[k][:, :, :2], np.ones((S, S, 1))], -1).dot(np.linalg.inv(np.eye(3).dot(mats[1 - k])))
        fl[:, :, :2] = c[:, :, :2] - np.stack([x0, y0], -1)
        fl[:, :, 0] = 2 * (fl[:, :, 0] / S)
        fl[:, :, 1] = 2 * (fl[:, :, 1] / S)
        assert (np.abs(fl.transpose(2, 0, 1) - flow[k]) <= b_flow[k]).all()


def test_sampler_rules():
    plane = np.arange(12, dtype=np.float32).reshape(3, 4)
    f = lambda *v: np.asarray(v, np.float32)
    # integers, the 1/32 lattice, 1/64 offsets (rne to the even lattice point), and the border
    v, _ = O.sample_linear(plane, f(1, 1.5, 1 + 1 / 64, 1 + 3 / 64, -0.5, 3.5, -1, np.nan, np.inf), f(0, 0, 0, 0, 0, 0, 0, 0, 0))
    assert v.tolist() == [1, 1.5, 1, 1 + 2 / 32, 0, 1.5, 0, 0, 0]
    (n, inside), _ = O.sample_nearest(plane, f(0.5, 1.5, 2.5, 3.5, -0.5, np.nan), f(0, 0, 0.5, 2.5, 0, 0))
    assert n.tolist() == [0, 2, 2, 0, 0, 0] and inside.tolist() == [True, True, True, False, True, False]


def test_crop_params_rules():
    (kaug, aff, status), _ = O.compute_crop_params(np.asarray([[3, 10, 2, 9], [3, 11, 2, 8], [40, -1, 24, -1], [5, 5, 1, 9], [0, 1, 0, 1]]), 16)
    assert aff[0].tolist() == [2 * 3 / 16, 2 * 3 / 16, 6 - 3, 5 - 3]       # l = 3: int(3.6) = 3
    assert aff[1].tolist() == [2 * 4 / 16, 2 * 3 / 16, 7 - 4, 5 - 3]       # l = (4, 3): int(4.8) = 4
    assert np.isnan(aff[2:]).all() and status.tolist() == [1, 2]
    assert np.isnan(kaug[2:]).all()
    assert O.pair_major_rows(6).tolist() == [0, 2, 4, 1, 3, 5]


# ---- wiring ---------------------------------------------------------------------------------------------------------------
def test_source_is_built():
    assert "framepair_kernels.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "framepair_kernels.hip"))


def test_entries_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "moda_hip.h")).read()
    declared = set(re.findall(r"\b(moda_[a-z0-9_]+)\s*\(", hdr))
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.moda_abi_version() == _lib.ABI_VERSION == 11
    assert (FP.INTER_NEAREST, FP.INTER_LINEAR) == tuple(int(re.search(rf"#define {n}\s+(\d+)", hdr).group(1))
                                                        for n in ("MODA_REMAP_NEAREST", "MODA_REMAP_LINEAR"))


def test_public_names():
    import moda_amd
    for n in ("mask_bbox", "compute_crop_params", "remap", "warp_flow", "crop_frames", "flow_process", "fb_flow_check",
              "prepare_frame_pairs"):
        assert getattr(moda_amd, n) is getattr(FP, n)


# ---- refusals -------------------------------------------------------------------------------------------------------------
def raw_cpu(bs=1, h=6, w=8):
    return {"img": torch.zeros(bs, 2, h, w, 3, dtype=torch.uint8), "mask": torch.ones(bs, 2, h, w), "flow": torch.zeros(bs, 2, h, w, 2),
            "occ": torch.zeros(bs, 2, h, w), "dp": torch.zeros(bs, 2, h, w, dtype=torch.int32), "dp_feat": torch.zeros(bs, 2, 16, 4, 4),
            "dp_bbox": torch.zeros(bs, 2, 4), "rtk": torch.zeros(bs, 2, 4, 4), "dataid": torch.zeros(bs, 2), "frameid": torch.zeros(bs, 2)}


def test_refuses_cpu_tensors():
    r = raw_cpu()
    aff = torch.ones(2, 4, dtype=torch.float64)
    plane, maps = torch.zeros(2, 6, 8), torch.zeros(6, 8)
    for call in (lambda: FP.mask_bbox(r["mask"]), lambda: FP.compute_crop_params(r["mask"], 8), lambda: FP.remap(plane, maps, maps),
                 lambda: FP.warp_flow(plane, plane), lambda: FP.fb_flow_check(plane, plane),
                 lambda: FP.crop_frames(aff, 8, img=r["img"][0], mask=r["mask"][0]),
                 lambda: FP.flow_process(torch.zeros(2, 2, 8, 8), aff, 8), lambda: FP.prepare_frame_pairs(r, 8)):
        with pytest.raises(RuntimeError, match="CUDA"):
            call()


def test_refuses_grad():
    r = raw_cpu()
    g = torch.zeros(2, 6, 8, requires_grad=True)
    maps = torch.zeros(6, 8)
    for call in (lambda: FP.mask_bbox(g), lambda: FP.compute_crop_params(g, 8), lambda: FP.remap(g, maps, maps),
                 lambda: FP.warp_flow(g, g), lambda: FP.fb_flow_check(g, g),
                 lambda: FP.flow_process(torch.zeros(2, 2, 8, 8, requires_grad=True), torch.ones(2, 4, dtype=torch.float64), 8),
                 lambda: FP.prepare_frame_pairs(dict(r, flow=r["flow"].clone().requires_grad_()), 8)):
        with pytest.raises(NotImplementedError, match="grad"):
            call()


@pytest.mark.parametrize("key,bad", [("img", lambda t: t.float()), ("mask", lambda t: t.double()), ("flow", lambda t: t.half()),
                                     ("occ", lambda t: t.double()), ("dp", lambda t: t.long()), ("dp", lambda t: t.transpose(2, 3)),
                                     ("flow", lambda t: t[..., :1]), ("dp_feat", lambda t: t.double())])
def test_refuses_dtype_and_layout_naming_the_argument(key, bad):
    r = raw_cpu()
    r[key] = bad(r[key])
    with pytest.raises(ValueError, match=key):
        FP.prepare_frame_pairs(r, 8)


def test_refuses_shape_mismatch_and_other_arguments():
    r = raw_cpu()
    with pytest.raises(ValueError, match="share"):                         # a flow stored at another resolution is not resized
        FP.prepare_frame_pairs(dict(r, flow=torch.zeros(1, 2, 3, 4, 2)), 8)
    with pytest.raises(ValueError, match="rtk"):
        FP.prepare_frame_pairs(dict(r, rtk=torch.zeros(1, 2, 3, 4)), 8)
    with pytest.raises(ValueError, match="lacks"):
        FP.prepare_frame_pairs({k: v for k, v in r.items() if k != "dp"}, 8)
    with pytest.raises(ValueError, match="img_size"):
        FP.prepare_frame_pairs(r, 0)
    with pytest.raises(ValueError, match="map_x"):
        FP.remap(torch.zeros(6, 8), torch.zeros(6, 8).double(), torch.zeros(6, 8))
    with pytest.raises(ValueError, match="interpolation"):
        FP.remap(torch.zeros(6, 8), torch.zeros(6, 8), torch.zeros(6, 8), 2)
    with pytest.raises(ValueError, match="affine"):
        FP.flow_process(torch.zeros(2, 2, 8, 8), torch.ones(2, 4), 8)
    with pytest.raises(ValueError, match="masks"):
        FP.mask_bbox(torch.zeros(2, 6, 8, dtype=torch.int32))
