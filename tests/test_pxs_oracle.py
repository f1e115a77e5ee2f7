"""CPU: the numpy restatement of the pixel sampling (tests/pxs_numpy.py) against a literal torch replay of the reference's
view(2,-1) / topk / stack / cat / view(-1) sequence (nnutils/moda.py:1075-1191), the ordering rule of moda_topk_rows against a
stable sort, the new C entries, and the Python refusals of moda_amd.pixel_sampling."""
import os
import re
import types

import numpy as np
import pytest
import torch

import pxs_numpy as pn
from moda_amd import _lib, build
from moda_amd import pixel_sampling as PS

NEW_ENTRIES = ("moda_topk_rows", "moda_pxs_assemble", "moda_obs_gather")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_line_replay(unc_pred, rand_inds, nsample_in, nactive, ids, Rmat):
    """moda.py:1062-1191 for training, lineload, active sampling, on CPU torch, line by line as the reference writes it;
    `unc_pred` (bs, 4 nsample) stands for nerf_unc's output.  -> per-ray rand_inds, ids, batch_map, Rmat."""
    bs = rand_inds.shape[0]
    nsample = nsample_in
    nsample_a = 4 * nsample
    nsample_s = int(nactive * nsample)
    nsample = int(nsample * (1 - nactive))
    rand_inds_a = rand_inds[:, -nsample_a:].clone()
    rand_inds = rand_inds[:, :nsample].clone()
    ids_a = {k: v[:, None].repeat(1, nsample_a) for k, v in ids.items()}
    ids = {k: v[:, None].repeat(1, nsample) for k, v in ids.items()}
    Rmat_a = Rmat[:, None].repeat(1, nsample_a, 1, 1)
    Rmat = Rmat[:, None].repeat(1, nsample, 1, 1)
    batch_map = torch.Tensor(range(bs))[:, None].long()
    batch_map_a = batch_map.repeat(1, nsample_a)
    batch_map = batch_map.repeat(1, nsample)
    unc_pred = unc_pred.view(2, -1)
    rand_inds, rand_inds_a = rand_inds.view(2, -1), rand_inds_a.view(2, -1)
    ids = {k: v.view(2, -1) for k, v in ids.items()}
    ids_a = {k: v.view(2, -1) for k, v in ids_a.items()}
    batch_map, batch_map_a = batch_map.view(2, -1), batch_map_a.view(2, -1)
    Rmat, Rmat_a = Rmat.view(2, -1, 3, 3), Rmat_a.view(2, -1, 3, 3)
    nsample_s = nsample_s * bs // 2
    bs = 2
    topk_samp = unc_pred.topk(nsample_s, dim=-1)[1]
    rand_inds_a = torch.stack([rand_inds_a[i][topk_samp[0]] for i in range(bs)], 0)
    ids_a = {k: torch.stack([v[i][topk_samp[0]] for i in range(bs)], 0) for k, v in ids_a.items()}
    batch_map_a = torch.stack([batch_map_a[i][topk_samp[0]] for i in range(bs)], 0)
    Rmat_a = torch.stack([Rmat_a[i][topk_samp[0]] for i in range(bs)], 0)
    rand_inds = torch.cat([rand_inds, rand_inds_a], 1)
    ids = {k: torch.cat([ids[k], ids_a[k]], 1) for k in ids}
    batch_map = torch.cat([batch_map, batch_map_a], 1)
    Rmat = torch.cat([Rmat, Rmat_a], 1)
    return (rand_inds.view(-1, 1), {k: v.view(-1) for k, v in ids.items()}, batch_map.view(-1), Rmat.view(-1, 3, 3),
            topk_samp[0])


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("nsample", [4, 5, 6])
@pytest.mark.parametrize("nactive", [0.25, 0.5])
def test_closed_form_ray_order_equals_the_reference_sequence(P, nsample, nactive):
    rng = np.random.default_rng(100 * P + 10 * nsample + int(nactive * 4))
    bs, W = 2 * P, 8
    n_u, n_s = pn.split_counts(nsample, nactive)
    if nsample == 5:
        assert (n_u, n_s) == ((3, 1) if nactive == 0.25 else (2, 2))          # the int() roundings
    unc = rng.permutation(bs * 4 * nsample).astype(np.float32).reshape(bs, 4 * nsample)      # distinct: torch.topk is unambiguous
    rand_inds = rng.integers(0, W, (bs, 5 * nsample))
    ids = {k: rng.integers(0, 50, bs) for k in ("frameid", "frameid_sub", "dataid", "errid")}
    Rmat = rng.standard_normal((bs, 3, 3)).astype(np.float32)
    want_rand, want_ids, want_bm, want_R, want_topk = reference_line_replay(
        torch.from_numpy(unc), torch.from_numpy(rand_inds), nsample, nactive, {k: torch.from_numpy(v) for k, v in ids.items()},
        torch.from_numpy(Rmat))
    if n_s == 0:
        topk = np.zeros((0,), np.int64)
    else:
        topk = pn.topk_rows(unc[:P].reshape(1, -1), n_s * P)[0][0]             # the first P lines' candidates only
        assert np.array_equal(topk, want_topk.numpy())
    got = pn.assemble(rand_inds, nsample, n_u, n_s, True, W, np.arange(bs), ids["frameid"], ids["frameid_sub"], ids["dataid"],
                      ids["errid"], topk, np.zeros((50, 2), np.float32), 0)
    assert got["rand_inds"].shape[0] == 2 * (P * n_u + n_s * P)
    assert np.array_equal(got["rand_inds"], want_rand.numpy()[:, 0])
    assert np.array_equal(got["batch_map"], want_bm.numpy())
    for k in ids:
        assert np.array_equal(got[k], want_ids[k].numpy()), k
    assert np.array_equal(Rmat[got["batch_map"]], want_R.numpy())


def test_plain_split_equals_the_reference_sequence():
    """Active sampling off (moda.py:1075-1098, 1181-1191): ray b * nsample + j reads rand_inds[b, j]."""
    rng = np.random.default_rng(3)
    bs, nsample = 6, 5
    rand_inds = rng.integers(0, 8, (bs, 5 * nsample))
    got = pn.assemble(rand_inds, nsample, nsample, 0, True, 8, np.arange(bs), np.arange(bs), np.arange(bs), np.zeros(bs), np.arange(bs),
                      None, np.zeros((bs, 2), np.float32), 0)
    t = torch.from_numpy(rand_inds)
    assert np.array_equal(got["rand_inds"], t[:, :nsample].clone().view(-1, 1).numpy()[:, 0])
    assert np.array_equal(got["batch_map"], torch.arange(bs)[:, None].repeat(1, nsample).view(-1).numpy())


def test_frame_mode_equals_the_reference_sequence():
    """moda.py:1171-1177: per-row top-k, only rand_inds / xys reordered."""
    rng = np.random.default_rng(4)
    bs, nsample, n_u, n_s, S = 3, 4, 2, 2, 8
    unc = rng.permutation(bs * 16).astype(np.float32).reshape(bs, 16)
    rand_inds = rng.integers(0, S * S, (bs, 5 * nsample))
    t, u = torch.from_numpy(rand_inds), torch.from_numpy(unc)
    top = u.topk(n_s, dim=-1)[1]
    a = t[:, -16:].clone()
    want = torch.cat([t[:, :n_u].clone(), torch.stack([a[i][top[i]] for i in range(bs)], 0)], 1)
    topk = pn.topk_rows(unc, n_s)[0]
    assert np.array_equal(topk, top.numpy())
    got = pn.assemble(rand_inds, nsample, n_u, n_s, False, S, None, np.arange(bs), np.arange(bs), np.zeros(bs), np.arange(bs), topk,
                      np.ones((bs, 2), np.float32), 0)
    assert np.array_equal(got["rand_inds"].reshape(bs, -1), want.numpy())
    assert np.array_equal(got["xys"][:, 0], want.numpy().reshape(-1) % S) and np.array_equal(got["xys"][:, 1], want.numpy().reshape(-1) // S)


def test_ordering_rule_against_a_stable_sort():
    inf, nan = np.inf, np.nan
    v = np.asarray([[0.0, -0.0, 1.0, nan, inf, -inf, 1.0, -0.0, nan, 0.0, -1.0, inf]], np.float32)
    idx, vals, n_nan = pn.topk_rows(v, v.shape[1])
    #              NaNs by index, +inf by index, the 1s, the zeros of either sign by index, -1, -inf
    assert idx[0].tolist() == [3, 8, 4, 11, 2, 6, 0, 1, 7, 9, 10, 5] and n_nan == 2
    assert np.signbit(vals[0][7]) and not np.signbit(vals[0][6])                # values come back as stored
    # independent statement: Python's stable sort on (not NaN, -value with -0 == +0)
    rng = np.random.default_rng(0)
    for _ in range(20):
        r = rng.choice(np.asarray([0.0, -0.0, 1.5, -1.5, inf, -inf, nan, 2.0], np.float32), 40)
        key = [(0 if np.isnan(x) else 1, 0.0 if np.isnan(x) else -(float(x) + 0.0)) for x in r]
        want = sorted(range(40), key=lambda i: key[i])
        for k in (1, 5, 40):
            assert pn.topk_rows(r[None], k)[0][0].tolist() == want[:k]
    assert pn.topk_rows(np.zeros((2, 7), np.float32), 3)[0].tolist() == [[0, 1, 2], [0, 1, 2]]     # all equal: pure index order


def test_new_entries_are_bound_declared_and_exported():
    assert _lib.ABI_VERSION == 11
    header = open(os.path.join(ROOT, "include", "moda_hip.h")).read()
    for name in NEW_ENTRIES:
        assert name in _lib.EXPORTS
        assert re.search(r"\bint " + name + r"\(", header), name
    m = re.search(r"#define MODA_TOPK_MAX_N (\d+)", header)
    assert m and int(m.group(1)) == PS.TOPK_MAX_N >= 8192
    assert "pixsample_kernels.hip" in build.SOURCES
    lib = _lib.load()
    assert lib.moda_abi_version() == 11
    for name in NEW_ENTRIES:
        assert hasattr(lib, name)
    ESHAPE, EINVAL = -2, -1
    # refusals come before any pointer is looked at
    assert lib.moda_topk_rows(None, 1, PS.TOPK_MAX_N + 1, 1, None, None, None, None) == ESHAPE
    assert lib.moda_topk_rows(None, 1, 0, 1, None, None, None, None) == ESHAPE
    assert lib.moda_topk_rows(None, 70000, 300, 1, None, None, None, None) == ESHAPE
    assert lib.moda_topk_rows(None, 1, 8, 0, None, None, None, None) == EINVAL
    assert lib.moda_topk_rows(None, 1, 8, 9, None, None, None, None) == EINVAL
    assert lib.moda_topk_rows(None, 1, 8, 8, None, None, None, None) == EINVAL          # NULL pointers
    assert lib.moda_pxs_assemble(None, 3, 4, 2, 2, 1, 8, *([None] * 5), 1, None, None, 4, 0, *([None] * 10)) == EINVAL    # odd bs
    assert lib.moda_pxs_assemble(None, 2, 1, 0, 0, 1, 8, *([None] * 5), 1, None, None, 4, 0, *([None] * 10)) == EINVAL    # no ray
    assert lib.moda_obs_gather(*([None] * 6), 0, 8, None, None, 4, 1, *([None] * 8)) == ESHAPE


def _opts(**kw):
    o = dict(lineload=True, use_unc=True, nactive=0.5, warmup_steps=0.2, use_embed=True, flowbw=False, lbs=False, neudbs=True)
    o.update(kw)
    return types.SimpleNamespace(**o)


def test_python_refusals():
    model = types.SimpleNamespace(opts=_opts(flowbw=True), training=True, progress=0.5, img_size=8)
    args = [None] * 15
    with pytest.raises(NotImplementedError, match="flowbw"):
        PS.sample_pxs(model, 2, 4, *args)
    model.opts = _opts(lbs=True)
    with pytest.raises(NotImplementedError, match="lbs"):
        PS.sample_pxs(model, 2, 4, *args)
    model.opts = _opts()
    with pytest.raises(ValueError, match="odd"):
        PS.sample_pxs(model, 3, 4, *args)
    with pytest.raises(ValueError, match="n_u \\+ n_s == 0"):
        PS.sample_pxs(model, 2, 1, *args)
    with pytest.raises(ValueError, match="MODA_TOPK_MAX_N"):
        PS.sample_pxs(model, 2 * 4097, 4, *args)                                 # 4097 lines x 16 candidates = 65552 > 65536
    img = torch.zeros(2, 3, 8, 1)
    with pytest.raises(ValueError, match="imgs must be contiguous fp32"):
        PS.sample_pxs(model, 2, 4, *([None] * 9), img.double(), *([None] * 5))
    with pytest.raises(ValueError, match="masks must be contiguous fp32"):
        PS.sample_pxs(model, 2, 4, *([None] * 9), img, torch.zeros(2, 1, 8, 2)[..., :1], *([None] * 4))
    assert PS.split_counts(5, 0.5) == (2, 2) and PS.split_counts(5, 0.25) == (3, 1) and PS.split_counts(1, 0.5) == (0, 0)
