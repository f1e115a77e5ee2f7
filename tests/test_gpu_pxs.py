"""GPU (-m gpu): device-resident pixel sampling (moda_amd/pixel_sampling.py, csrc/pixsample_kernels.hip) against the numpy
restatement tests/pxs_numpy.py -- itself pinned to the reference's literal sequence by tests/test_pxs_oracle.py, and otherwise
unpinned to a reference run (moda.py cannot be imported beside the tests)."""
import types

import numpy as np
import pytest
import torch

import pxs_numpy as pn
from helpers import rel_err

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import moda_amd
    from moda_amd import synth, feeders as FD, pixel_lines as PL, pixel_sampling as PS
    from gpu_helpers import T, DEV

# fp32 bars of tests/test_gpu_feeders.py (raycast values 1e-5, its camera gradients 1e-4), applied to the same kernels here
VAL_BAR, GRAD_BAR = 1e-5, 1e-4
# ts = fsub / max_ts * 2 - 1 in fp32: three roundings of values <= 1 in magnitude, 3 * 2^-24 < 2e-7 absolute against float64
TS_BAR = 2e-7


def np_(t):
    return t.detach().cpu().numpy()


def ids_t(a, dtype=torch.int64):
    return torch.as_tensor(np.asarray(a), device=DEV).to(dtype)


# ---- moda_topk_rows ----------------------------------------------------------------------------------------------------------------------
def _rows(n, seed):
    """Four rows of n values: distinct normals; all equal; four levels; normals with +-0, +-inf and NaNs mixed in."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(n).astype(np.float32)
    b = np.full(n, 0.25, np.float32)
    c = rng.choice(np.asarray([-1.0, 0.0, 0.5, 2.0], np.float32), n)
    d = rng.standard_normal(n).astype(np.float32)
    special = np.asarray([0.0, -0.0, np.inf, -np.inf, np.nan, -0.0, 0.0, np.nan], np.float32)
    where = rng.random(n) < 0.3
    d[where] = rng.choice(special, int(where.sum()))
    return np.stack([a, b, c, d])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1000, 4096, 6144, 65536])
def test_topk_rows_matches_the_ordering_rule_exactly(n):
    """n = 256 / 257: the last row length that shares a workgroup and the first that does not; 65536 = MODA_TOPK_MAX_N."""
    assert PS.TOPK_MAX_N == 65536
    v = _rows(n, n)
    for k in sorted({1, max(1, n // 8), n}):
        want_idx, want_val, n_nan = pn.topk_rows(v, k)
        idx, vals, status = PS.topk_rows(T(v), k, return_values=True)
        idx2, vals2, status2 = PS.topk_rows(T(v), k, return_values=True)
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (4, k)
        assert np.array_equal(np_(idx), want_idx), (n, k)
        assert np.array_equal(np_(vals).view(np.uint32), want_val.view(np.uint32)), (n, k)      # bits: a -0 stays -0, NaN payloads kept
        assert np_(status).tolist() == [n_nan, 0, 0, 0]
        assert torch.equal(idx, idx2) and torch.equal(vals.view(torch.int32), vals2.view(torch.int32)) and torch.equal(status, status2)


def test_topk_many_short_rows_and_refusals():
    rng = np.random.default_rng(7)
    v = rng.choice(np.asarray([0.0, 1.0, 2.0, -0.0, np.nan], np.float32), (513, 24))      # rows = 513, n = 24, k = 3: ties everywhere
    idx, status = PS.topk_rows(T(v), 3)
    want, _, n_nan = pn.topk_rows(v, 3)
    assert np.array_equal(np_(idx), want) and int(status[0]) == n_nan
    one = np.asarray([[3.0, 1.0, 2.0]], np.float32)                                       # rows = 1
    assert np_(PS.topk_rows(T(one), 2)[0]).tolist() == [[0, 2]]
    for k in (0, 4):
        with pytest.raises(ValueError, match="k ="):
            PS.topk_rows(T(one), k)
    with pytest.raises(ValueError, match="MODA_TOPK_MAX_N"):
        PS.topk_rows(torch.zeros((1, PS.TOPK_MAX_N + 1), device=DEV), 1)


# ---- moda_pxs_assemble / moda_obs_gather -------------------------------------------------------------------------------------------------
W = 8


def _lines(P, nsample, seed, line=True):
    rng = np.random.default_rng(seed)
    bs = 2 * P
    d = dict(rand_inds=rng.integers(0, W if line else W * W, (bs, 5 * nsample)), lineid=rng.integers(0, W, bs),
             frameid=rng.integers(0, 9, bs), frameid_sub=rng.integers(0, 20, bs), dataid=rng.integers(0, 2, bs),
             errid=rng.integers(0, 1000, bs), near_far=rng.random((9, 2)).astype(np.float32))
    pix = W if line else W * W
    d["obs"] = {k: rng.standard_normal((bs, c, pix)).astype(np.float32)
                for k, c in (("imgs", 3), ("masks", 1), ("vis2d", 1), ("flow", 2), ("occ", 1), ("dp_feats", 16))}
    return d


OBS_KEYS = dict(imgs="img_at_samp", masks="sil_at_samp", vis2d="vis_at_samp", flow="flo_at_samp", occ="cfd_at_samp", dp_feats="feats_at_samp")


def _check_assembly(d, nsample, n_u, n_s, line, topk, id_dtype, with_feats, n_vid=2):
    want = pn.assemble(d["rand_inds"], nsample, n_u, n_s, line, W, d["lineid"], d["frameid"], d["frameid_sub"], d["dataid"], d["errid"],
                       topk, d["near_far"], n_vid)
    got = PS.assemble_rays(ids_t(d["rand_inds"]), nsample, n_u, n_s, line, W, ids_t(d["lineid"], id_dtype), ids_t(d["frameid"], id_dtype),
                           ids_t(d["frameid_sub"], id_dtype), ids_t(d["dataid"], id_dtype), ids_t(d["errid"], id_dtype),
                           None if topk is None else ids_t(topk, torch.int32), T(d["near_far"]), n_vid)
    for k in PS.ASSEMBLED:
        g, w = np_(got[k]), want[k]
        assert g.shape == w.shape, k
        if k == "rand_inds":                       # a refused top-k entry has no column: -1 there, the oracle's column elsewhere
            assert np.array_equal(g, w)
        else:
            assert np.array_equal(g, w, equal_nan=True), k
    assert np_(got["status"]).tolist() == want["status"].tolist()
    # the gather, against the oracle and -- on valid input -- against the torch restatement pixel_lines.obs_to_rays[_line]
    obs = {k: v for k, v in d["obs"].items() if with_feats or k != "dp_feats"}
    dev_obs = {k: T(v) for k, v in obs.items()}
    R = want["rand_inds"].shape[0]
    if line:
        rays = PS.gather_obs({}, got["rand_inds"].view(R, 1), got["batch_map"], dev_obs["imgs"][..., None], dev_obs["masks"], dev_obs["vis2d"],
                             dev_obs["flow"], dev_obs["occ"], dev_obs.get("dp_feats"))
        ref = pn.gather_obs(obs, want["batch_map"], want["rand_inds"])
        shape = lambda c: (R, 1, c)
    else:
        bs = d["rand_inds"].shape[0]
        rays = PS.gather_obs({}, got["rand_inds"].view(bs, -1), None, *(dev_obs[k] for k in ("imgs", "masks", "vis2d", "flow", "occ")),
                             dev_obs.get("dp_feats"))
        ref = pn.gather_obs(obs, np.repeat(np.arange(bs), n_u + n_s), want["rand_inds"])
        shape = lambda c: (bs, n_u + n_s, c)
    assert ("feats_at_samp" in rays) == with_feats
    for k, name in OBS_KEYS.items():
        if k in obs:
            assert tuple(rays[name].shape) == shape(obs[k].shape[1]), name
            assert np.array_equal(np_(rays[name]).reshape(R, -1), ref[k], equal_nan=True), name
    bad_cols = int(want["status"][2])
    assert np_(rays["obs_status"]).tolist() == [0, 0, bad_cols, 0]
    if bad_cols == 0:
        four = {k: v[..., None] for k, v in dev_obs.items()}
        if line:
            pl = PL.obs_to_rays_line({}, got["rand_inds"].view(R, 1), four["imgs"], four["masks"], four["vis2d"], four["flow"], four["occ"],
                                     four.get("dp_feats"), got["batch_map"])
        else:
            pl = PL.obs_to_rays({}, got["rand_inds"].view(d["rand_inds"].shape[0], -1), four["imgs"], four["masks"], four["vis2d"],
                                four["flow"], four["occ"], four.get("dp_feats"))
        for name in pl:
            assert torch.equal(pl[name], rays[name]), name
    return want, got


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("nsample", [4, 5, 6])
@pytest.mark.parametrize("nactive", [0.25, 0.5])
def test_assemble_and_gather_line_mode(P, nsample, nactive):
    d = _lines(P, nsample, 1000 * P + 10 * nsample + int(4 * nactive))
    n_u, n_s = pn.split_counts(nsample, nactive)
    rng = np.random.default_rng(P + nsample)
    K = n_s * P
    topk = rng.permutation(P * 4 * nsample)[:K]
    if K >= 2 and P > 1:
        topk[:2] = [4 * nsample + 1, 4 * nsample + 3]          # one line (l = 1) chosen by several active rays
    for id_dtype, with_feats in ((torch.int64, True), (torch.int32, False)):
        _check_assembly(d, nsample, n_u, n_s, True, topk if K else None, id_dtype, with_feats)
    _check_assembly(d, nsample, nsample, 0, True, None, torch.int64, True)                      # active sampling off: the plain split


def test_assemble_and_gather_frame_mode():
    for nsample, nactive in ((4, 0.5), (5, 0.25), (6, 0.5)):
        d = _lines(2, nsample, 50 + nsample, line=False)
        n_u, n_s = pn.split_counts(nsample, nactive)
        rng = np.random.default_rng(nsample)
        topk = np.stack([rng.permutation(4 * nsample)[:n_s] for _ in range(4)])
        _check_assembly(d, nsample, n_u, n_s, False, topk, torch.int64, True)
        _check_assembly(d, nsample, n_u, n_s, False, topk, torch.int32, False)


def test_out_of_range_columns_and_ids_give_nan_rows_and_exact_counts():
    P, nsample, n_u, n_s = 3, 4, 2, 2
    d = _lines(P, nsample, 77)
    d["rand_inds"][1, 0] = W                 # a uniform column past the line
    d["rand_inds"][4, nsample + 5] = -1      # a candidate column below it: chosen below through c = 1 * 16 + 5, second half
    d["frameid"][2] = 9                      # outside near_far (9 rows)
    d["frameid"][3] = -1
    d["dataid"][5] = 2                       # outside vid_code (2 rows)
    topk = np.asarray([16 + 5, 0, 33, 34, 2, 47])
    want, got = _check_assembly(d, nsample, n_u, n_s, True, topk, torch.int64, True)
    R = 2 * (P * n_u + P * n_s)
    bad_col = np.isnan(want["xys"][:, 0])
    assert bad_col.sum() == 2 and want["status"].tolist() == [0, int((want["frameid"] == 9).sum() + (want["frameid"] == -1).sum()
                                                                    + (want["dataid"] == 2).sum()), 2, 0]
    assert np.isnan(np_(got["near_far"])).any(1).tolist() == ((want["frameid"] < 0) | (want["frameid"] > 8)).tolist()
    assert not np.isnan(np_(got["xys"])[~bad_col]).any()                                          # the neighbours are untouched
    # a top-k entry outside the candidates is refused as a column is, and nothing is read through it
    bad = PS.assemble_rays(ids_t(d["rand_inds"]), nsample, n_u, n_s, True, W, *(ids_t(d[k]) for k in ("lineid", "frameid", "frameid_sub",
                           "dataid", "errid")), ids_t([48, -1, 0, 1, 2, 3], torch.int32), T(d["near_far"]), 0)
    half = P * n_u + P * n_s
    assert np_(bad["rand_inds"])[[P * n_u, P * n_u + 1, half + P * n_u, half + P * n_u + 1]].tolist() == [-1] * 4
    assert int(bad["status"][2]) >= 4
    # the gather alone: a row outside the batch
    obs = {k: T(v) for k, v in d["obs"].items()}
    rays = PS.gather_obs({}, ids_t([[1], [2], [3]]), ids_t([0, 6, -1]), *(obs[k] for k in ("imgs", "masks", "vis2d", "flow", "occ")), obs["dp_feats"])
    assert np_(rays["obs_status"]).tolist() == [0, 2, 0, 0]
    assert torch.equal(rays["img_at_samp"][0, 0], obs["imgs"][0, :, 1]) and torch.isnan(rays["feats_at_samp"][1:]).all()
    with pytest.raises(ValueError, match="contiguous fp32"):
        PS.gather_obs({}, ids_t([[1]]), ids_t([0]), obs["imgs"].double(), *(obs[k] for k in ("masks", "vis2d", "flow", "occ")))


# ---- sample_pxs end to end ---------------------------------------------------------------------------------------------------------------
N_FRAMES, MAX_TS, BONES = 12, 12.0, 25


def _model(seed, lineload=True, use_unc=True, progress=0.5):
    from gpu_helpers import unc_models, make_models
    models, emb = unc_models(seed, BONES)
    models["nerf_feat"] = make_models(seed, BONES, with_feat=True)[0]["nerf_feat"]
    model = types.SimpleNamespace(device=DEV, training=True, progress=progress, img_size=W, max_ts=MAX_TS, num_bone_used=BONES)
    model.opts = types.SimpleNamespace(lineload=lineload, use_unc=use_unc, nactive=0.5, warmup_steps=0.2, use_embed=True, flowbw=False,
                                       lbs=False, neudbs=True, num_bones=BONES, env_code=True, appearance_code=True)
    off = np.asarray([0, N_FRAMES])
    model.pose_code = FD.FrameCodeTable(N_FRAMES, 6, 128, off).to(DEV)
    model.env_code = FD.FrameCodeTable(N_FRAMES, 6, 64, off).to(DEV)
    model.appearance_code = FD.FrameCodeTable(N_FRAMES, 6, 128, off).to(DEV)
    head = FD.DQ_RTHead(use_quat=True, in_channels_xyz=128, in_channels_dir=0, out_channels=7 * BONES, raw_feat=True).to(DEV)
    with torch.no_grad():
        head.rgb[0].weight.mul_(0.05)
        head.rgb[0].bias.copy_(torch.tensor([0, 0, 0, 1, 0, 0, 0.0], device=DEV).repeat(BONES))
    model.nerf_body_rts = torch.nn.Sequential(model.pose_code, head)
    model.rest_pose_code = models["rest_pose_code"]
    model.vid_code = torch.nn.Embedding(2, 32).to(DEV)
    model.vid_code.weight.data = T(synth.normal(seed, "pxs/vid_code", (2, 32)))
    model.embedding_xyz = emb["xyz"]
    model.nerf_models = models
    model.near_far = T(np.stack([np.full(N_FRAMES, 0.6, np.float32), np.linspace(1.3, 1.5, N_FRAMES).astype(np.float32)], 1))
    return model, emb


def _batch(seed, P, nsample, line=True):
    d = _lines(P, nsample, seed, line=line)
    bs = 2 * P
    cam = synth.make_cameras(seed, bs)
    d["frameid"] = np.arange(bs) % N_FRAMES
    d["frameid_sub"] = d["frameid"].copy()
    dev = {k: ids_t(d[k]) for k in ("dataid", "frameid", "frameid_sub", "lineid", "errid")}
    obs = [T(d["obs"][k])[..., None].contiguous() for k in ("imgs", "masks", "vis2d", "flow", "occ", "dp_feats")]
    cams = [T(cam[k]).requires_grad_(True) for k in ("Rmat", "Tmat", "Kinv")]
    return d, cam, dev, obs, cams


def _call(model, bs, nsample, cams, dev, obs, rand_inds, **kw):
    return PS.sample_pxs(model, bs, nsample, *cams, dev["dataid"], dev["frameid"], dev["frameid_sub"], dev["frameid"], dev["lineid"],
                         dev["errid"], *obs, rand_inds=rand_inds, **kw)


def test_sample_pxs_line_mode_end_to_end():
    moda_amd.set_precision("fp32")
    P, nsample = 3, 4
    bs, n_u, n_s = 2 * P, 2, 2
    model, emb = _model(31)
    d, cam, dev, obs, cams = _batch(31, P, nsample)
    rand_inds, rays, frameid, errid = _call(model, bs, nsample, cams, dev, obs, ids_t(d["rand_inds"]), return_unc=True)
    assert frameid.is_cuda and errid.is_cuda and np_(rays["pxs_status"]).tolist() == [0, 0, 0, 0]
    unc = np_(rays["unc_candidates"])
    assert unc.shape == (P, 4 * nsample)
    # the selection is the oracle's top-k of the predictions it was made from ...
    topk = pn.topk_rows(unc.reshape(1, -1), n_s * P)[0][0]
    want = pn.assemble(d["rand_inds"], nsample, n_u, n_s, True, W, d["lineid"], d["frameid"], d["frameid_sub"], d["dataid"], d["errid"],
                       topk, np_(model.near_far), 2)
    R = 2 * (P * n_u + P * n_s)
    assert np.array_equal(np_(rand_inds), want["rand_inds"].reshape(R, 1)) and np.array_equal(np_(frameid), want["frameid"])
    assert np.array_equal(np_(errid), want["errid"]) and np.array_equal(np_(rays["xys"]), want["xys"].reshape(R, 1, 2))
    assert np.array_equal(np_(rays["near"]).reshape(-1), want["near_far"][:, 0]) and np.array_equal(np_(rays["far"]).reshape(-1), want["near_far"][:, 1])
    # ... and equals evaluating all 2P lines and reading row 0, as the reference does
    cand = ids_t(d["rand_inds"])[:, nsample:]
    xys_all = torch.stack([cand.float(), dev["lineid"][:, None].float().expand(bs, 4 * nsample)], -1)
    unc_all = PS._predict_unc(model, dev["dataid"], dev["frameid_sub"], xys_all, cams[2])
    assert torch.equal(unc_all.view(2, -1)[0], rays["unc_candidates"].reshape(-1))
    # ray tensors against float64
    line = want["ray_line"]
    d64, o64 = pn.raycast(want["xys"], cam["Rmat"][line], cam["Tmat"][line], cam["Kinv"][line])
    ts64, vid64, xysn64 = pn.unc_inputs(want["xys"], cam["Kinv"][line], want["frameid_sub"], want["dataid"], np_(model.vid_code.weight), MAX_TS)
    assert rel_err(np_(rays["rays_d"]).reshape(R, 3), d64) < VAL_BAR and rel_err(np_(rays["rays_o"]).reshape(R, 3), o64) < VAL_BAR
    assert rel_err(np_(rays["xysn"]).reshape(R, 2), xysn64) < VAL_BAR
    assert np.abs(np_(rays["ts"]).reshape(R, 1) - ts64).max() < TS_BAR
    assert np.array_equal(np_(rays["vid_code"]).reshape(R, 32), vid64.astype(np.float32))             # a gather: exact
    rtk = np.concatenate([cam["Rmat"].reshape(bs, 9), cam["Tmat"].reshape(bs, 3), cam["Kinv"].reshape(bs, 9)], 1)
    assert np.array_equal(np_(rays["rtk_vec"]).reshape(R, 21), rtk[line])                             # the row gather: exact
    assert np.array_equal(np_(rays["rtk_vec_target"]).reshape(2, R // 2, 21), rtk[line].reshape(2, R // 2, 21)[::-1])
    ref_obs = pn.gather_obs(d["obs"], want["batch_map"], want["rand_inds"])
    for k, name in OBS_KEYS.items():
        assert np.array_equal(np_(rays[name]).reshape(R, -1), ref_obs[k]), name
    # gradients onto the cameras and the video code against the float64 restatement
    cf = {k: synth.normal(31, "pxs/c/" + k, tuple(rays[k].shape)) for k in ("rays_d", "rays_o", "xysn", "vid_code")}
    sum((T(c) * rays[k]).sum() for k, c in cf.items()).backward()
    dR, dT, dK = pn.raycast_grads(want["xys"], cam["Rmat"][line], cam["Tmat"][line], cam["Kinv"][line], cf["rays_d"].reshape(R, 3),
                                  cf["rays_o"].reshape(R, 3), cf["xysn"].reshape(R, 2), line, bs)
    for t, w, name in zip(cams, (dR, dT, dK), ("Rmat", "Tmat", "Kinv")):
        assert rel_err(np_(t.grad), w) < GRAD_BAR, name
    dv = np.zeros((2, 32))
    np.add.at(dv, want["dataid"], cf["vid_code"].reshape(R, 32).astype(np.float64))
    assert rel_err(np_(model.vid_code.weight.grad), dv) < GRAD_BAR
    # render_rays takes the dict
    from gpu_helpers import make_opts
    skip = ("unc_candidates", "pxs_status", "obs_status")
    flat = {k: v.detach().reshape(R, -1) for k, v in rays.items() if torch.is_tensor(v) and k not in skip}
    with torch.no_grad():
        res = moda_amd.render_rays(model.nerf_models, emb, flat, N_samples=16, noise_std=0.0, opts=make_opts(dist_corresp=True),
                                   img_size=W, obj_bound=np.asarray([0.2, 0.2, 0.2], np.float32))
    assert tuple(res["unc_pred"].shape)[0] == R and torch.isfinite(res["unc_pred"]).all()


def test_sample_pxs_plain_below_warmup_frame_mode_and_eval():
    moda_amd.set_precision("fp32")
    P, nsample = 2, 4
    bs = 2 * P
    d, cam, dev, obs, cams = _batch(32, P, nsample)
    for kw in (dict(progress=0.1), dict(use_unc=False)):                   # below warmup_steps; no uncertainty head in use
        model, _ = _model(32, **kw)
        rand_inds, rays, frameid, errid = _call(model, bs, nsample, cams, dev, obs, ids_t(d["rand_inds"]), return_unc=True)
        want = pn.assemble(d["rand_inds"], nsample, nsample, 0, True, W, d["lineid"], d["frameid"], d["frameid_sub"], d["dataid"],
                           d["errid"], None, np_(model.near_far), 0)
        assert "unc_candidates" not in rays and tuple(rand_inds.shape) == (bs * nsample, 1)
        assert np.array_equal(np_(rand_inds)[:, 0], want["rand_inds"]) and np.array_equal(np_(frameid), want["frameid"])
        assert np.array_equal(np_(rays["xys"]).reshape(-1, 2), want["xys"]) and ("xysn" in rays) == model.opts.use_unc
        assert tuple(rays["rtk_vec_target"].shape) == (bs * nsample, 1, 21)
    # frame mode with active sampling: per-row selection, only rand_inds / xys reordered
    model, _ = _model(32, lineload=False)
    df, _, devf, obsf, _ = _batch(33, P, nsample, line=False)
    rand_inds, rays, frameid, errid = _call(model, bs, nsample, cams, devf, obsf, ids_t(df["rand_inds"]), return_unc=True)
    topk = pn.topk_rows(np_(rays["unc_candidates"]), 2)[0]
    want = pn.assemble(df["rand_inds"], nsample, 2, 2, False, W, None, df["frameid"], df["frameid_sub"], df["dataid"], df["errid"], topk,
                       np_(model.near_far), 2)
    assert np.array_equal(np_(rand_inds), want["rand_inds"].reshape(bs, 4)) and np.array_equal(np_(frameid), want["frameid"])
    assert np.array_equal(np_(rays["xys"]), want["xys"].reshape(bs, 4, 2)) and tuple(rays["img_at_samp"].shape) == (bs, 4, 3)
    ref = pn.gather_obs(df["obs"], np.repeat(np.arange(bs), 4), want["rand_inds"])
    assert np.array_equal(np_(rays["feats_at_samp"]).reshape(bs * 4, 16), ref["dp_feats"])
    # eval: every pixel of every frame, the reference's return_all path
    model.training = False
    rand_inds, rays, frameid, errid = _call(model, bs, nsample, cams, devf, obsf, None)
    assert tuple(rays["rays_d"].shape) == (bs, W * W, 3) and tuple(rays["img_at_samp"].shape) == (bs, W * W, 3)
    assert torch.equal(rays["img_at_samp"], obsf[0][..., 0].permute(0, 2, 1)) and tuple(rays["xysn"].shape) == (bs, W * W, 2)


def test_sample_pxs_replays_from_a_graph():
    """Captured after an eager warm-up; the rand_inds buffer and nerf_unc's weights are then overwritten in place: the replay must
    equal a fresh eager call on the new contents, exactly."""
    moda_amd.set_precision("fp32")
    P, nsample = 3, 4
    bs = 2 * P
    model, _ = _model(34)
    d, cam, dev, obs, cams = _batch(34, P, nsample)
    cams = [c.detach() for c in cams]
    buf = ids_t(d["rand_inds"])
    keys = ("rays_d", "rays_o", "xys", "near", "xysn", "vid_code", "bone_rts", "img_at_samp", "feats_at_samp", "unc_candidates", "pxs_status")
    with torch.no_grad():
        _call(model, bs, nsample, cams, dev, obs, buf, return_unc=True)                    # warm-up: tables and constants are built here
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g_rand, g_rays, g_fid, g_eid = _call(model, bs, nsample, cams, dev, obs, buf, return_unc=True)
        rng = np.random.default_rng(99)
        buf.copy_(ids_t(rng.integers(0, W, (bs, 5 * nsample))))
        for p in model.nerf_models["nerf_unc"].parameters():
            p.mul_(-0.75)
        graph.replay()
        torch.cuda.synchronize()
        e_rand, e_rays, e_fid, e_eid = _call(model, bs, nsample, cams, dev, obs, buf.clone(), return_unc=True)
    assert torch.equal(g_rand, e_rand) and torch.equal(g_fid, e_fid) and torch.equal(g_eid, e_eid)
    for k in keys:
        assert torch.equal(g_rays[k], e_rays[k]), k
