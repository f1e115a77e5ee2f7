"""GPU (-m gpu): evaluation-frame rendering (moda_amd/eval_frames.py, csrc/evalvis_kernels.hip) against the float64 restatement
tests/evalvis_numpy.py, itself pinned to the reference by tests/test_evalvis_oracle.py where the reference can be run."""
import importlib
import os
import types

import numpy as np
import pytest
import torch

import evalvis_numpy as en

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import moda_amd
    from moda_amd import synth
    from gpu_helpers import T, DEV
    EF = importlib.import_module("moda_amd.eval_frames")       # (moda_amd.eval_frames is the function of that name)

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g39_evalvis.npz"))


def np_(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    if a.dtype == torch.float32 and b.dtype == torch.float32:
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


# ---- flow colouring ----------------------------------------------------------------------------------------------------------------------
def check_flow(got, flow, golden=None, after=np.float64):
    """The rule of comparison, per call (all frames pooled).  Against the float64 restatement on the float64 copy of the flow:
      * a channel is undecided when it is not exact by construction and 255 col lies within 0.01 of an integer (the fp32 radius
        maximum and, in the fp32 mode, the fp32 angle move 255 col by 3e-3 at most; 0.01 is three times that): it may differ by
        one level;
      * the pixels of maximal radius sit on the `rad <= 1` branch: they equal the reference's fp32 golden where there is one,
        else one of the two branch values;
      * every other channel is equal; at most 3 % of the channels are undecided."""
    img, pre, exact, top, alt = en.flow_to_images(flow.astype(np.float64))
    top = top | en.flow_to_images(flow, after)[3]
    t = np.broadcast_to(top[..., None], img.shape)
    und = ~exact & (np.abs(pre - np.round(pre)) < 0.01) & ~t
    d = got.astype(int) - img.astype(int)
    print(f"flow {flow.shape}: undecided {und.mean():.4f}, differing undecided {(d[und] != 0).sum()}, top pixels {top.sum()}, "
          f"differing elsewhere {(d != 0)[~und & ~t].sum()}")
    assert not (d != 0)[~und & ~t].any()
    assert np.abs(d[und]).max(initial=0) <= 1
    if golden is not None:
        assert np.array_equal(got[t], golden[t])
    else:
        assert ((got[t] == img[t]) | (got[t] == alt[t])).all()
    assert und.mean() <= 0.03


@pytest.mark.parametrize("case", ["one1x1", "zero5x7", "nan5x7", "unknown33x31", "rand64", "smooth64"])
def test_flow_to_image_golden_frames(case):
    """1 x 1, 5 x 7 (all zero; a NaN), 33 x 31 (unknown flow, a third channel), 64 x 64: the default arithmetic equals the
    reference's fp32 run bit for bit on the pixels of maximal radius and by the rule elsewhere; the fp32 arithmetic by the rule."""
    flow = G[case + "/flow"]
    x = T(flow[None])
    got = EF.flow_to_image(x)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1,) + flow.shape[:2] + (3,)
    check_flow(np_(got), flow[None], golden=G[case + "/img32"][None])
    assert np.array_equal(np_(x), flow[None], equal_nan=True)                       # the caller's tensor is not written
    check_flow(np_(EF.flow_to_image(x, f64_after_norm=False)), flow[None], after=np.float32)
    assert torch.equal(EF.flow_to_image(x[0]), got[0])                              # one (H, W, C) frame
    if case == "zero5x7":
        assert (np_(got) == 255).all()


@pytest.mark.parametrize("where", [0, 255, 256, 2047, 2048, 4095])
def test_flow_maximum_at_the_ends_and_the_seams(where):
    """Three 64 x 64 frames with different maxima in one call; frame 1's maximum sits at pixel `where`: the first and last pixel,
    either side of a workgroup's seam (256 lanes) and of a reduction tile's (2048 pixels)."""
    rng = np.random.default_rng(where)
    flow = rng.standard_normal((3, 64, 64, 2)).astype(np.float32) * np.asarray([0.2, 1.0, 7.0], np.float32)[:, None, None, None]
    flow[1].reshape(-1, 2)[where] = [30.5, -41.25]
    for mode, after in ((True, np.float64), (False, np.float32)):
        got = EF.flow_to_image(T(flow), f64_after_norm=mode)
        check_flow(np_(got), flow, after=after)
        assert torch.equal(got, EF.flow_to_image(T(flow), f64_after_norm=mode))     # the same bits twice
        for i in range(3):                                                          # a frame alone has the frame's bits in the batch
            assert torch.equal(EF.flow_to_image(T(flow[i:i + 1]), f64_after_norm=mode)[0], got[i])


# ---- canvases ----------------------------------------------------------------------------------------------------------------------------
KEYS_C = dict(flo_coarse=2, img_loss_samp=1, frame_cyc_dis=1, pts_pred=3, pts_exp=3, sil_coarse=1, feat_err=1, proj_err=1, unc_pred=1,
              img_coarse=3, dis_reg=1)
OPTS = dict(use_embed=True, use_proj=True, use_unc=True)


def _chunk(seed, bs, S, Sm, scale=1.0):
    rng = np.random.default_rng(seed)
    r = {k: (scale * rng.random((bs, S, S, c))).astype(np.float32) for k, c in KEYS_C.items()}
    r["unc_pred"] -= np.float32(0.3)
    masks = (rng.random((bs + 1, Sm, Sm)) > 0.4).astype(np.float32)
    obs = dict(masks=masks, imgs=rng.random((bs + 1, 3, Sm, Sm)).astype(np.float32), flow=rng.standard_normal((bs + 1, 2, Sm, Sm)).astype(np.float32),
               occ=rng.random((bs + 1, Sm, Sm)).astype(np.float32), dp_feats=rng.standard_normal((bs + 1, 16, 4, 4)).astype(np.float32))
    return r, obs


def ulp_check(got, want, k):
    """|got - want| <= 2 ulp of the float64 result rounded to fp32; NaN where NaN."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), k
    w32 = want[~nan].astype(np.float32)
    with np.errstate(over="ignore"):
        err = np.abs(got[~nan].astype(np.float64) - want[~nan]) / np.spacing(np.abs(w32)).astype(np.float64)
    inf = np.isinf(w32)
    assert np.array_equal(got[~nan][inf], w32[inf]), k
    worst = err[~inf].max(initial=0)
    print(f"  {k}: worst {worst:.3f} ulp over {err.size} elements")
    assert worst <= 2.0, (k, worst)


def run_canvases(r, obs, S):
    opts = types.SimpleNamespace(render_size=S, **OPTS)
    rt = {k: T(v) for k, v in r.items()}
    out, status = EF.eval_canvases(rt, {k: T(v) for k, v in obs.items()}, opts)
    for k, v in r.items():
        assert np.array_equal(np_(rt[k]), v, equal_nan=True), k                    # the inputs are not written
    return out, status


@pytest.mark.parametrize("bs,Sm", [(1, 8), (2, 12), (3, 16), (2, 5), (1, 64)])
def test_eval_canvases_per_element(bs, Sm):
    """Per element against float64.  With silhouettes of 0 and 1 the masking product is exact, so a masked, scaled canvas carries
    two roundings, the division 255 / max and the final product: each is at most half an ulp of its own result, which is at most
    one ulp of the final result wherever that lies in its binade, hence 2 ulp.  unc_pred adds x - min and max - min.
    render_size 8 with masks of 8, 12, 16 and 5 (equal, 1.5 x, 2 x, upsampling); (1, 64): render_size 64, two reduction tiles, the
    maximum of feat_err moved to either side of the seam and to the ends.  Two chunks with different maxima: each its own."""
    S = 64 if Sm == 64 else 8
    for seed, scale in ((bs * 100 + Sm, 1.0), (bs * 100 + Sm + 1, 37.5)):
        for where in sorted({min(w, bs * S * S - 1) for w in ((0, 2047, 2048, 4095) if S == 64 else (0, bs * S * S - 1, 63, 64))}):
            r, obs = _chunk(seed, bs, S, Sm, scale)
            obs["masks"][:bs] = np.maximum(obs["masks"][:bs], 0)
            r["feat_err"].reshape(-1)[where] = 1000.0
            r["unc_pred"].reshape(-1)[where] = -5.0
            r["proj_err"].reshape(-1)[min(where + 1, bs * S * S - 1)] = 2000.0
            yx = np.unravel_index(where % (S * S), (S, S))
            ys, xs = (min(int(np.floor(np.float32(v) * (np.float32(Sm) / np.float32(S)))), Sm - 1) for v in yx)
            obs["masks"][where // (S * S), ys, xs] = 1.0                            # the planted maximum stays inside the silhouette
            out, status = run_canvases(r, obs, S)
            want = en.eval_canvases(r, obs["masks"], **OPTS)
            assert "dis_reg" not in out and np_(status).tolist() == [0, 0, 0, 0]
            for k, w in want.items():
                ulp_check(np_(out[k]), w, k)
            assert float(out["unc_pred"].min()) == 0.0
            for k in ("img_coarse", "sil_coarse"):                                  # untouched keys pass through
                assert np.array_equal(np_(out[k]), r[k])
            assert np.array_equal(np_(out["img"]), obs["imgs"].transpose(0, 2, 3, 1)[:bs]) and tuple(out["sil"].shape) == (bs, Sm, Sm, 1)
            assert np.array_equal(np_(out["flo"]), obs["flow"].transpose(0, 2, 3, 1)[:bs]) and tuple(out["occ"].shape) == (bs, Sm, Sm, 1)
            assert np.allclose(np_(out["feat"])[..., 0], obs["dp_feats"].std(1, ddof=1)[:bs], rtol=1e-5, atol=1e-6) and "dpc" not in out
            # the nearest resize alone, against torch on the CPU
            sil = torch.nn.functional.interpolate(torch.from_numpy(obs["masks"][:bs, None]), (S, S))[:, 0, ..., None].numpy()
            assert np.array_equal(np_(out["img_loss_samp"]), r["img_loss_samp"] * sil)


def test_eval_canvases_zero_mask_nan_and_refusals():
    r, obs = _chunk(7, 2, 8, 12)
    obs["masks"][:] = 0                                                             # every masked maximum is 0: 255 / 0 = inf, 0 * inf = NaN
    out, status = run_canvases(r, obs, 8)
    assert torch.isnan(out["feat_err"]).all() and torch.isnan(out["proj_err"]).all() and (out["flo_coarse"] == 0).all()
    assert np_(status).tolist() == [2, 0, 0, 0]
    want = en.eval_canvases(r, obs["masks"], **OPTS)
    ulp_check(np_(out["unc_pred"]), want["unc_pred"], "unc_pred")
    r, obs = _chunk(8, 2, 8, 8)
    obs["masks"][:] = 1
    r["proj_err"][1, 3, 4, 0] = np.nan                                              # NaN wins the maximum, as in torch: the whole key is NaN
    out, status = run_canvases(r, obs, 8)
    assert torch.isnan(out["proj_err"]).all() and np_(status).tolist() == [0, 1, 0, 0]
    ulp_check(np_(out["feat_err"]), en.eval_canvases(r, obs["masks"], **OPTS)["feat_err"], "feat_err")
    opts = types.SimpleNamespace(render_size=8, **OPTS)
    dev = {k: T(v) for k, v in r.items()}
    with pytest.raises(NotImplementedError, match="require grad"):
        EF.eval_canvases({**dev, "feat_err": dev["feat_err"].clone().requires_grad_(True)}, {k: T(v) for k, v in obs.items()}, opts)
    with pytest.raises(ValueError, match="render_size"):
        EF.eval_canvases(dev, {k: T(v) for k, v in obs.items()}, types.SimpleNamespace(render_size=9, **OPTS))
    with pytest.raises(KeyError, match="unc_pred"):
        EF.eval_canvases({k: v for k, v in dev.items() if k != "unc_pred"}, {k: T(v) for k, v in obs.items()}, opts)


# ---- grid, display, video ----------------------------------------------------------------------------------------------------------------
def test_image_grid_to_display_video_frames_bit_equal():
    rng = np.random.default_rng(5)
    img = rng.standard_normal((10, 5, 7, 3)).astype(np.float32)
    for row, col in ((3, 3), (1, 1), (2, 5), (5, 2)):
        assert np.array_equal(np_(EF.image_grid(T(img), row, col)), en.image_grid(img, row, col))
    assert np.array_equal(np_(EF.image_grid(T(G["grid/img"]), 3, 3)), G["grid/out"])
    with pytest.raises(ValueError, match="frames for a"):
        EF.image_grid(T(img), 4, 3)
    grid = en.image_grid(img, 3, 3)
    grid[0, 0, 0], grid[-1, -1, -1] = 9.0, -7.5                                     # the extrema at the two ends
    for tag in ("depth_rnd", "img_coarse"):
        got = np_(EF.to_display(tag, T(grid)))
        assert np.array_equal(got.view(np.uint32), en.to_display(tag, grid).astype(np.float32).view(np.uint32)), tag
    g2 = grid.copy()
    g2[2, 2, 1] = np.nan
    assert torch.isnan(EF.to_display("occ", T(g2))).all()                           # NaN extrema, as torch's min / max
    got = np_(EF.to_display("sil_coarse", T(g2)))
    assert np.isnan(got[2, 2, 1]) and np.array_equal(got, en.to_display("sil_coarse", g2).astype(np.float32), equal_nan=True)
    flo = grid[..., :2].copy()
    check_flow(np_(EF.to_display("flo_coarse", T(flo)))[None], flo[None])
    # video frames: the 8-bit rule at its edges; frame 0 has a maximum <= 1 and is scaled, frame 1 is not, frame 2 holds a NaN
    fr = np.zeros((3, 2, 4, 1), np.float32)
    fr[0].reshape(-1)[:] = [-0.5, 0.999, 1.0, 0.5, 0.0, -1.0, 0.25, 0.75]
    fr[1].reshape(-1)[:] = [-0.5, 0.999, 1.0, 255.9, 256.0, 1e9, -1e9, 100.5]
    fr[2].reshape(-1)[:] = [np.nan, 0.999, 1.0, 255.9, 256.0, 3.0, -0.999, 255.0]
    for up in (3, 7, 0.5, 30):
        st = EF.new_status(DEV)
        got = EF.video_frames(T(fr), up, status=st)
        want, ns, nn = en.video_frames(fr, up, False)
        assert got.dtype == torch.uint8 and np.array_equal(np_(got), want), up
        assert np_(st).tolist() == [0, 1, ns, nn], up                               # (frame 2's maximum is NaN: counted as a NaN extremum)
    flows = G["rand64/flow"][None].repeat(2, 0) * np.asarray([1.0, 0.0], np.float32)[:, None, None, None]
    got = EF.video_frames(T(flows), 4, is_flow=True)
    want = en.video_frames(flows.astype(np.float64), 4, True)[0]
    assert tuple(got.shape) == (4, 64, 64, 3) and np.array_equal(np_(got)[2:], want[2:])     # the zero flow: white
    check_flow(np_(got)[:1], flows[:1], golden=G["rand64/img32"][None])


# ---- nerf_render_eval / render_vid -------------------------------------------------------------------------------------------------------
def _eval_model(seed, P=2):
    from test_gpu_pxs import _model, _batch, W
    from gpu_helpers import make_opts
    model, emb = _model(seed, lineload=False)
    d, cam, dev, obs, _ = _batch(seed, P, 4, line=False)
    bs = 2 * P
    model.training = False
    model.embeddings = emb
    model.opts = types.SimpleNamespace(**{**vars(make_opts(dist_corresp=True)), **vars(model.opts), "ndepth": 16, "chunk": 100, "perturb": 0,
                                          "noise_std": 0.0, "fine_steps": 1.1, "rnd_frame_chunk": 3, "render_size": W})
    model.latest_vars = {"obj_bound": np.asarray([0.2, 0.2, 0.2], np.float32)}
    model.vis_min, model.vis_len = np.asarray([-0.2, -0.25, -0.3], np.float32), np.asarray([0.4, 0.5, 0.6], np.float32)
    rtk = np.zeros((bs, 4, 4), np.float32)
    rtk[:, :3, :3], rtk[:, :3, 3] = cam["Rmat"], cam["Tmat"]
    rtk[:, 3] = [12.0, 12.0, W / 2, W / 2]
    model.rtk, model.kaug = T(rtk), T(np.tile(np.asarray([1, 1, 0, 0], np.float32), (bs, 1)))
    for k in ("dataid", "frameid", "frameid_sub", "errid"):
        setattr(model, k, dev[k])
    model.embedid, model.lineid = dev["frameid"], None
    for k, t in zip(("imgs", "masks", "vis2d", "flow", "occ", "dp_feats"), obs):
        setattr(model, k, t)
    return model, bs, W


def test_nerf_render_eval_equals_the_chunks_gathered_by_hand():
    """img_size 8, ndepth 16, two frame pairs (256 rays).  The canvases equal the per-chunk render_rays calls concatenated by hand,
    bit for bit, and are the same for chunks of 100 and 37 rays, neither of which divides 256 -- every key but flo_loss_samp, which
    the reference normalises by the mean confidence of the chunk's own rays (rendering.py:554-555) and eval() never shows."""
    before = moda_amd.get_precision()
    moda_amd.set_precision("fp32")
    try:
        _render_eval_checks()
    finally:
        moda_amd.set_precision(before)             # the library's mode is process-wide: leave it as it was found


def _render_eval_checks():
    from moda_amd import feeders as FD, geom_utils as GU, pixel_sampling as PS
    model, bs, W = _eval_model(41)
    opts = model.opts
    res, rand_inds = EF.nerf_render_eval(model, model.rtk, model.kaug, model.embedid)
    assert tuple(rand_inds.shape) == (bs, W * W)
    with torch.no_grad():
        Rm, Tm, Ki = GU.prepare_ray_cams(model.rtk, model.kaug)
        _, rays, _, _ = PS.sample_pxs(model, bs, 256, Rm, Tm, Ki, model.dataid, model.frameid, model.frameid_sub, model.embedid, None,
                                      model.errid, model.imgs, model.masks, model.vis2d, model.flow, model.occ, model.dp_feats)
        rays = {k: v.contiguous() if torch.is_tensor(v) else v for k, v in rays.items() if k not in ("unc_candidates", "pxs_status", "obs_status")}
        parts = [moda_amd.render_rays(model.nerf_models, model.embeddings, FD.chunk_rays(rays, i, 100), N_samples=16, perturb=0,
                                      noise_std=0.0, chunk=100, obj_bound=model.latest_vars["obj_bound"], use_fine=False, img_size=W,
                                      progress=model.progress, opts=opts) for i in range(0, bs * W * W, 100)]
    for k in ("img_coarse", "sil_coarse", "flo_coarse", "img_loss_samp", "feat_err", "proj_err", "unc_pred"):
        assert k in res, (k, sorted(res))
    vmin, vlen = T(model.vis_min[None]), T(model.vis_len[None])
    for k, v in res.items():
        if v.dim() == 0:
            assert torch.equal(v, torch.stack([p[k] for p in parts]).mean()), k
            continue
        hand = torch.cat([p[k] for p in parts], 0).view(bs, W, W, -1)
        if k in ("pts_pred", "pts_exp"):
            hand = ((hand - vmin) / vlen).clamp(0, 1)
            assert float(v.min()) >= 0 and float(v.max()) <= 1
        assert tuple(v.shape[:3]) == (bs, W, W) and same_bits(v, hand), k
    res37, _ = EF.nerf_render_eval(model, model.rtk, model.kaug, model.embedid, chunk=37)
    for k, v in res.items():
        if k == "flo_loss_samp":        # the reference divides a chunk's confidences by THEIR mean (rendering.py:554-555): per chunk by definition
            continue
        assert same_bits(v, res37[k]), k
    vid = EF.render_vid(model)
    assert not set(vid) & set(EF.VIS_KEYS) and "pts_pred_vis" in res
    for k, v in vid.items():
        assert same_bits(v, res[k][:bs // 2]), k
    # the loop of eval(): two chunks of rnd_frame_chunk = 3 frames' worth of calls, each chunk normalised on its own
    calls = []

    def set_input(m, idx):
        calls.append(list(idx))
        m.masks = (model_masks[:, 0, :, 0].reshape(bs, W, W) > 0).float()

    model_masks = model.masks
    ef = moda_amd.eval_frames(model, [0, 1, 2, 3], set_input)
    model.masks = model_masks
    assert calls == [[0, 1, 2], [3]] and isinstance(ef, moda_amd.EvalFrames)
    assert tuple(ef.rendered_seq["feat_err"].shape) == (2 + 1, W, W, 1)             # bs // 2 = 2 rows a call, the second chunk keeps 1
    for part in (ef.rendered_seq["feat_err"][:2], ef.rendered_seq["feat_err"][2:]):
        assert abs(float(part.max()) - 255.0) < 1e-3 or float(part.max()) == 0.0 or bool(torch.isnan(part).all())
    with pytest.raises(ValueError, match="frames for a"):
        ef.grid("feat_err")
    assert tuple(ef.grid("feat_err", 1, 3).shape) == (W, 3 * W, 1) and tuple(ef.video("flo_coarse").shape) == (3, W, W, 3)
    # refusals
    model.training = True
    with pytest.raises(ValueError, match="training mode"):
        EF.nerf_render_eval(model, model.rtk, model.kaug, model.embedid)
    model.training = False
    with pytest.raises(NotImplementedError, match="require grad"):
        EF.nerf_render_eval(model, model.rtk.clone().requires_grad_(True), model.kaug, model.embedid)
    model.opts.lbs = True
    with pytest.raises(NotImplementedError, match="linear blend skinning"):
        EF.render_vid(model)


# ---- repeatability and capture -----------------------------------------------------------------------------------------------------------
def test_same_bits_twice_and_from_a_graph():
    """eval_canvases + flow_to_image, eager twice and replayed from a captured graph (one chain, no parallel branches) after the
    inputs were overwritten in place: the same bits as a fresh eager call on the new contents."""
    r, obs = _chunk(11, 3, 8, 12)
    opts = types.SimpleNamespace(render_size=8, **OPTS)
    rt, ot = {k: T(v) for k, v in r.items()}, {k: T(v) for k, v in obs.items()}
    keys = ("flo_coarse", "img_loss_samp", "frame_cyc_dis", "pts_pred", "pts_exp", "feat_err", "proj_err", "unc_pred")

    def run():
        out, status = EF.eval_canvases(rt, ot, opts)
        return out, status, EF.flow_to_image(out["flo_coarse"])

    a, b = run(), run()                                                             # (the first call builds the cached tables)
    for k in keys:
        assert torch.equal(a[0][k].view(torch.int32), b[0][k].view(torch.int32)), k
    assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g = run()
    r2, _ = _chunk(12, 3, 8, 12, scale=5.0)
    for k, v in r2.items():
        rt[k].copy_(T(v))
    graph.replay()
    torch.cuda.synchronize()
    e = run()
    for k in keys:
        assert torch.equal(g[0][k].view(torch.int32), e[0][k].view(torch.int32)), k
    assert torch.equal(g[2], e[2]) and torch.equal(g[1], e[1])
    assert not torch.equal(e[2], a[2])
