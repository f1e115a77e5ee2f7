"""GPU checks of the frame-pair preparation (moda_amd/frame_pairs.py, csrc/framepair_kernels.hip) against the float64 oracle
tests/framepair_numpy.py within the bounds it states.  Boxes, crop parameters, crop coordinates and nearest planes are exact; the
crop's linear planes are held at EVERY pixel; flow_process may exempt the pixels the oracle marks (a half-integer of the 1/32
lattice within the flow bound, occ within its bound of 0.25), at most 1 % of a plane.  Source frames 24 x 40 and 37 x 65,
img_size 16 and 32 (alp dyadic: every coordinate exact) and 24 (not dyadic)."""
import numpy as np
import pytest
import torch

import framepair_numpy as O
from moda_amd import frame_pairs as FP
from moda_amd import pixel_sampling
from test_framepair_oracle import EXEMPT_CAP, G, NAMES

pytestmark = pytest.mark.gpu
SHAPES = [(24, 40, 16), (37, 65, 32), (37, 65, 24)]


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def within(got, want, bound, exempt=None):
    bad = np.abs(got - want) > bound
    if exempt is not None:
        assert exempt.reshape(exempt.shape[0], -1).mean(1).max() <= EXEMPT_CAP
        bad &= ~(exempt if exempt.shape == bad.shape else np.broadcast_to(exempt[:, None], bad.shape))
    assert not bad.any(), (int(bad.sum()), float(np.abs(got - want)[bad].max()))


def blob(rng, h, w, lo=0.2, hi=0.33):
    yy, xx = np.mgrid[:h, :w]
    cy, cx, ry, rx = rng.uniform(0.35, 0.65) * h, rng.uniform(0.35, 0.65) * w, rng.uniform(lo, hi) * h, rng.uniform(lo, hi) * w
    return ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) < 1).astype(np.uint8)


def make_raw(rng, bs, h, w):
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    d = np.stack([1.5 + 0.8 * np.sin(yy / 5.0), -1.0 + 0.6 * np.cos(xx / 7.0)], -1)
    flow = np.stack([np.stack([d + rng.standard_normal((h, w, 2)) * 0.05,
                               -d + rng.standard_normal((h, w, 2)) * 0.15 * (rng.random((h, w, 1)) < 0.7)]) for _ in range(bs)])
    return {"img": rng.integers(0, 256, (bs, 2, h, w, 3), dtype=np.uint8),
            "mask": np.stack([np.stack([blob(rng, h, w), blob(rng, h, w)]) for _ in range(bs)]),
            "flow": flow.astype(np.float32), "occ": rng.random((bs, 2, h, w)).astype(np.float32),
            "dp": rng.integers(0, 5000, (bs, 2, h, w)).astype(np.int32),
            "dp_feat": rng.standard_normal((bs, 2, 16, 12, 12)).astype(np.float32),
            "dp_bbox": np.tile(np.asarray([4, 3, w - 5, h - 4], np.float32), (bs, 2, 1)),
            "rtk": rng.standard_normal((bs, 2, 4, 4)).astype(np.float32),
            "dataid": np.zeros((bs, 2), np.int64), "frameid": np.arange(2 * bs, dtype=np.int64).reshape(bs, 2) * 3}


# ---- mask_bbox ------------------------------------------------------------------------------------------------------------
def bbox_cases(h, w):
    m = np.zeros((9, h, w), np.float32)
    m[0, -1, 3:5] = 1                                                      # the last row only
    m[1, 2:4, -1] = 2.5                                                    # the last column only
    m[2, h // 2, w // 3] = 1                                               # a single pixel
    m[4] = 1                                                               # the full frame (3: empty)
    m[5, 0, 0] = m[5, -1, -1] = 1                                          # two corners
    m[6, 1:-2, 2:-3] = np.random.default_rng(h * w).random((h - 3, w - 5)) > 0.7
    m[7] = -1                                                              # nothing is > 0
    m[7, 3, 1] = np.nan
    m[7, 4, 2] = 1e-30
    m[8, 0, -1] = 1                                                        # a corner pixel
    return m


@pytest.mark.parametrize("h,w", [(5, 63), (5, 64), (5, 65), (24, 40), (37, 65), (70, 130)])
def test_bbox_exact_and_repeatable(h, w):
    m = bbox_cases(h, w)
    want, _ = O.mask_bbox(m)
    assert want[3].tolist() == [w, -1, h, -1] and want[4].tolist() == [0, w - 1, 0, h - 1] and want[7].tolist() == [2, 2, 4, 4]
    got = host(FP.mask_bbox(dev(m)))
    assert np.array_equal(got, want)
    assert np.array_equal(host(FP.mask_bbox(dev(m))), got)                 # the same bits on a second run
    u8 = (np.nan_to_num(m) > 0).astype(np.uint8) * 200
    assert np.array_equal(host(FP.mask_bbox(dev(u8))), O.mask_bbox(u8)[0])
    assert np.array_equal(host(FP.mask_bbox(dev(u8).view(3, 3, h, w))).reshape(9, 4), O.mask_bbox(u8)[0])


# ---- crop parameters ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [16, 24, 32])
def test_crop_params_bit_equal_and_status(S):
    h, w = 37, 65
    m = np.zeros((8, h, w), np.uint8)
    for i, (x0, x1, y0, y1) in enumerate([(3, 10, 2, 9), (3, 11, 2, 8), (0, 64, 0, 36), (20, 43, 5, 30), (7, 8, 1, 20), (5, 5, 1, 9)]):
        m[i, y0:y1 + 1, x0:x1 + 1] = 1                                      # odd and even extents; 4: lx = 0; 5: one column
    m[7, 10, 10] = 1                                                       # a single pixel (6: empty)
    box, _ = O.mask_bbox(m)
    (kaug, aff, status), _ = O.compute_crop_params(box, S)
    assert status.tolist() == [1, 3]
    k, a, st = FP.compute_crop_params(dev(m), S)
    assert np.array_equal(host(k).view(np.uint32), kaug.view(np.uint32))   # bit-equal, the NaN rows included
    assert np.array_equal(host(a).view(np.uint64)[:4], aff.view(np.uint64)[:4]) and np.isnan(host(a)[4:]).all()
    assert host(st).tolist() == [1, 3]
    (kp, ap, _), _ = O.compute_crop_params(box, S, pair_major=True)
    k2, a2, _ = FP.compute_crop_params(dev(m).view(4, 2, h, w), S, pair_major=True)
    assert np.array_equal(np.isnan(host(k2)), np.isnan(kp)) and np.array_equal(np.nan_to_num(host(k2)), np.nan_to_num(kp))
    assert np.array_equal(np.nan_to_num(host(a2)), np.nan_to_num(ap))


# ---- crop remap -----------------------------------------------------------------------------------------------------------
def check_crop(raw_flat, aff, S, pair_major, lead):
    want, bound = O.crop_frames(aff, S, img=raw_flat["img"], flow=raw_flat["flow"], occ=raw_flat["occ"], mask=raw_flat["mask"],
                                dp=raw_flat["dp"], pair_major=pair_major)
    got = FP.crop_frames(dev(aff), S, pair_major=pair_major, **{k: dev(v).view(*lead, *v.shape[1:]) for k, v in raw_flat.items()})
    for k in ("masks", "dps", "vis2d"):
        assert np.array_equal(host(got[k]), want[k]), k                    # nearest planes: exact
    for k in ("imgs", "flow", "occ"):
        within(host(got[k]), want[k], bound[k])                            # linear planes: every pixel
    return want, got


@pytest.mark.parametrize("h,w,S", SHAPES)
def test_crop_remap_box_beyond_the_frame(h, w, S):
    rng = np.random.default_rng(S + h)
    raw = make_raw(rng, 2, h, w)
    raw["mask"][:] = 0
    raw["mask"][0, 0] = 1                                                  # 1.2 x the box reaches outside on all four sides
    raw["mask"][0, 1] = blob(rng, h, w)
    raw["mask"][1, 0, 4:5, :] = 1                                          # half-length 0 in y: refused
    raw["mask"][1, 1] = blob(rng, h, w, 0.3, 0.45)
    flat = {k: raw[k].reshape(4, *raw[k].shape[2:]) for k in ("img", "flow", "occ", "mask", "dp")}
    box, _ = O.mask_bbox(flat["mask"])
    (_, aff, status), _ = O.compute_crop_params(box, S, pair_major=True)
    assert status.tolist() == [0, 1] and np.isnan(aff[1]).all()             # frame (1, 0) is output row 1
    want, got = check_crop(flat, aff, S, True, (2, 2))
    v = want["vis2d"][0]
    assert v[0].sum() == 0 and v[:, 0].sum() == 0 and v.sum() > 0          # rows sample the cells' top-left corners, so at
    if S > 16:                                                             # 16 the last row and column are still inside
        assert v[-1].sum() == 0 and v[:, -1].sum() == 0
    assert all(np.abs(host(got[k])[1]).max() == 0 for k in got)            # the refused frame: zeros
    assert all(np.abs(want[k][[0, 2, 3]]).max() > 0 for k in want)         # the others untouched by it
    assert np.array_equal(host(got["masks"]), want["masks"] * want["vis2d"])


def test_crop_remap_integers_halves_and_64ths():
    h, w, S = 9, 8, 16
    rng = np.random.default_rng(5)
    raw = make_raw(rng, 1, h, w)
    flat = {k: raw[k].reshape(2, *raw[k].shape[2:]) for k in ("img", "flow", "occ", "mask", "dp")}
    flat["mask"] = rng.integers(0, 2, (2, h, w)).astype(np.float32) * 3
    aff = np.asarray([[0.5, 0.5, -2.0, -1.5],                              # integers and k + 0.5: rne picks the even pixel
                      [65 / 64, 49 / 64, -3.0, -2.5]])                     # 1/64 offsets: the 1/32 lattice rounds half to even
    x, y = O.crop_coords(aff[1], S)
    assert ((x * 64) % 2 == 1).any() and ((y * 64) % 2 == 1).any()
    want, _ = check_crop(flat, aff, S, False, (2,))
    v = want["vis2d"][1]                                                   # outside on all four sides
    assert v[0].sum() == 0 and v[-1].sum() == 0 and v[:, 0].sum() == 0 and v[:, -1].sum() == 0 and v.sum() > 0


# ---- remap, warp_flow, fb_flow_check --------------------------------------------------------------------------------------
def test_remap_explicit_maps_nan_and_out_of_range():
    """A NaN or infinite coordinate, like one outside the image, samples 0."""
    rng = np.random.default_rng(11)
    src = rng.standard_normal((3, 7, 9)).astype(np.float32)
    mx = rng.uniform(-2, 11, (6, 70)).astype(np.float32)
    my = rng.uniform(-2, 9, (6, 70)).astype(np.float32)
    mx[0, :8] = [np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, 8.5, -0.5]
    my[1, :3] = [np.nan, np.inf, 2 ** 31]
    mx[2, :6], my[2, :6] = [0, 8, 8.015625, 2.5, 3.5, 4.484375], [0, 6, 6, 1.5, 2.5, 0.515625]
    for mode in (FP.INTER_LINEAR, FP.INTER_NEAREST):
        want, bound = O.remap(src, mx, my, mode)
        got = host(FP.remap(dev(src), dev(mx), dev(my), mode))
        assert np.isfinite(got).all() and (np.abs(got - want) <= bound).all(), mode
        assert (got[:, 0, :6] == 0).all() and (got[:, 1, :3] == 0).all()
        if mode == FP.INTER_NEAREST:
            assert np.array_equal(got, want)
    assert np.array_equal(host(FP.remap(dev(src[0]), dev(mx), dev(my))), host(FP.remap(dev(src), dev(mx), dev(my)))[0])


def test_warp_flow_and_fb_flow_check():
    rng = np.random.default_rng(12)
    h, w = 13, 21
    img = rng.standard_normal((2, h, w)).astype(np.float32)
    flow = (rng.standard_normal((2, h, w)) * 3).astype(np.float32)
    flow[:, 0, :3] = np.nan
    for normed in (False, True):
        f = flow / (8 if normed else 1)
        want, bound, ex = O.warp_flow(img, f, normed)
        got = host(FP.warp_flow(dev(img), dev(f), normed))
        within(got, want, bound, np.broadcast_to(ex, (2, h, w)))
        assert (got[:, 0, :3] == 0).all()
    a = (rng.standard_normal((2, h, w)) * 0.1).astype(np.float32)
    b = (-a + rng.standard_normal((2, h, w)) * 0.01).astype(np.float32)
    a[:, 2, 2] = 0                                                         # a zero flow: its error is 0
    (wf, wb), (bf, bb), (ef, eb) = O.fb_flow_check(a, b)
    gf, gb = FP.fb_flow_check(dev(a), dev(b))
    within(host(gf)[None], wf[None], bf[None], ef[None])
    within(host(gb)[None], wb[None], bb[None], eb[None])
    assert host(gf)[2, 2] == 0 and wf.max() > 0


# ---- flow_process ---------------------------------------------------------------------------------------------------------
def run_flow(flow_c, aff, S, e_in=None):
    (wf, wo), (bf, bo), ex = O.flow_process(flow_c, aff, S, e_in)
    gf, go = FP.flow_process(dev(flow_c), dev(aff), S)
    within(host(gf), wf, bf)
    within(host(go), wo, bo, ex)
    return host(gf), host(go), wo


@pytest.mark.parametrize("S", [16, 24, 32])
def test_flow_process_zero_flow_and_constant_shift(S):
    aff = np.asarray([[1.5, 1.25, 4.0, 3.0], [1.5, 1.25, 4.0, 3.0]])       # the same crop: a zero flow stays zero
    flow, occ, _ = run_flow(np.zeros((2, 2, S, S), np.float32), aff, S)
    assert (flow == 0).all() and (occ == 1).all()
    aff = np.asarray([[1.5, 1.25, 4.0, 3.0], [1.5, 1.25, 7.0, 3.0]])       # the partner's crop starts 3 px = 2 cells later
    flow, occ, _ = run_flow(np.zeros((2, 2, S, S), np.float32), aff, S)
    assert (flow[0, 0] == np.float32(-4.0 / S)).all() and (flow[1, 0] == np.float32(4.0 / S)).all() and (flow[:, 1] == 0).all()
    assert (occ[0, :, 2:] == 1).all() and occ[0, 0, 0] == 1                # the taps of the first two columns are outside: the
    assert (occ[0, :, :2] == 0).sum() == 2 * S - 1                         # sample is 0, far from every pixel but (0, 0)
    assert (occ[1, :, :-2] == 1).all() and (occ[1, :, -2:] == 0).all()
    shift = np.zeros((2, 2, S, S), np.float32)                             # a constant shift and its inverse: consistent inside
    shift[0, 0], shift[1, 0] = 3.0, -3.0
    flow, occ, _ = run_flow(shift, np.asarray([[1.5, 1.25, 4.0, 3.0]] * 2), S)
    assert (flow[0, 0] == np.float32(4.0 / S)).all() and (occ[0, :, :-2] == 1).all() and (occ[0, :, -2:] == 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_flow_process_stored_cases(name):
    S = int(G[f"{name}/img_size"])
    box, _ = O.mask_bbox(G[f"{name}/masks"])
    (_, aff, _), _ = O.compute_crop_params(box, S)
    flow, occ, want = run_flow(G[f"{name}/flow_c"], aff, S)
    assert (want > 0).mean() > 0.2 and (want == 0).mean() > 0.05
    assert np.array_equal(host(FP.flow_process(dev(G[f"{name}/flow_c"]), dev(aff), S)[1]), occ)


def test_flow_process_refused_pair_is_zero():
    S = 16
    rng = np.random.default_rng(2)
    fc = rng.standard_normal((4, 2, S, S)).astype(np.float32)
    aff = np.asarray([[1.5, 1.25, 4.0, 3.0], [1.0, 1.0, 2.0, 2.0], [1.25, 1.5, 3.0, 4.0], [np.nan] * 4])
    flow, occ, _ = run_flow(fc, aff, S)
    assert (flow[[1, 3]] == 0).all() and (occ[[1, 3]] == 0).all() and np.abs(flow[[0, 2]]).min() > 0


# ---- prepare_frame_pairs --------------------------------------------------------------------------------------------------
def check_prepared(out, raw, S):
    want, bound, exempt = O.prepare_frame_pairs(raw, S)
    bs = raw["mask"].shape[0]
    rows = want["rows"]
    assert host(out["status"]).tolist() == want["status"].tolist()
    assert np.array_equal(host(out["kaug"]).view(np.uint32), want["kaug"].view(np.uint32))
    for k in ("masks", "vis2d", "dps"):
        assert np.array_equal(host(out[k]), want[k]), k
    within(host(out["imgs"]), want["imgs"], bound["imgs"])
    within(host(out["flow"]), want["flow"], bound["flow"])
    within(host(out["occ"]), want["occ"], bound["occ"], exempt)
    for k in ("rtk", "dp_bbox", "dataid", "frameid"):
        assert np.array_equal(host(out[k]), raw[k].reshape(2 * bs, *raw[k].shape[2:])[rows]), k
    assert np.array_equal(host(out["rt_raw"]), host(out["rtk"])[:, :3])
    return want


@pytest.mark.parametrize("h,w,S", SHAPES)
def test_prepare_frame_pairs_end_to_end(h, w, S):
    from moda_amd import cse
    rng = np.random.default_rng(S * 3 + h)
    raw = make_raw(rng, 3, h, w)
    d = {k: dev(v) for k, v in raw.items()}
    out = FP.prepare_frame_pairs(d, S)
    want = check_prepared(out, raw, S)
    assert (want["occ"] > 0).mean() > 0.1 and want["masks"].mean() > 0.1
    B = 6
    feats = torch.nn.functional.normalize(d["dp_feat"].transpose(0, 1).reshape(B, 16, 12, 12), 2, 1)
    assert torch.equal(out["dp_feats"], feats)
    assert torch.equal(out["dp_feats_rsmp"], cse.resample_dp(feats, out["dp_bbox"], out["kaug"], S))
    # the planes go into gather_obs as sample_pxs hands them on (views, nothing converted)
    flatten = lambda t, C: t.view(B, C, S * S)
    inds = torch.arange(5, device="cuda").repeat(B, 1) * 7
    rays = pixel_sampling.gather_obs({}, inds, None, flatten(out["imgs"], 3), flatten(out["masks"], 1), flatten(out["vis2d"], 1),
                                     flatten(out["flow"], 2), flatten(out["occ"], 1), flatten(out["dp_feats_rsmp"], 16))
    assert torch.equal(rays["img_at_samp"][:, :, 0], out["imgs"].view(B, 3, -1)[:, 0][:, inds[0]])
    assert host(rays["obs_status"]).sum() == 0


def test_prepare_frame_pairs_graph_replay_follows_new_masks():
    h, w, S = 37, 65, 24
    rng = np.random.default_rng(21)
    raw = make_raw(rng, 2, h, w)
    d = {k: dev(v) for k, v in raw.items()}
    status = torch.zeros(2, device="cuda", dtype=torch.int32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        FP.prepare_frame_pairs(d, S, status=status)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = FP.prepare_frame_pairs(d, S, status=status)
    seen = []
    for i in range(3):
        raw["mask"] = np.stack([np.stack([blob(rng, h, w, 0.15 + 0.05 * i, 0.3), blob(rng, h, w)]) for _ in range(2)])
        if i == 2:
            raw["mask"][1, 0] = 0                                          # an empty mask arrives: counted, zeros, no error
        d["mask"].copy_(dev(raw["mask"]))
        status.zero_()
        graph.replay()
        want = check_prepared(out, raw, S)
        seen.append(want["kaug"].copy())
    assert not np.array_equal(seen[0], seen[1]) and want["status"].tolist() == [1, 0]
