"""GPU (-m gpu): novel-view frame rendering (moda_amd/nvs.py, csrc/nvs_kernels.hip) against torch's own indexing, against
moda_amd.raycast bit for bit, against the numpy oracle tests/nvs_numpy.py and the reference's record tests/golden/g37_nvs.npz,
and end to end against a per-frame loop written here."""
import types

import numpy as np
import pytest
import torch

import nvs_numpy as O
from helpers import golden, rel_err

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import moda_amd
    from moda_amd import synth, feeders as FD, nvs as NV
    from gpu_helpers import T, DEV, make_models, make_opts

TILE = 1024                                  # MODA_NVS_SCAN_TILE (test_nvs_oracle pins NV.SCAN_TILE to the header)
RAYCAST_BAR = 1e-5                           # test_gpu_feeders.test_raycast_matches_reference


def np_(t):
    return t.detach().cpu().numpy()


def rng_of(*key):
    return np.random.default_rng([37] + [int(k) for k in key])


def check_list(masks):
    """pix, frame == torch.nonzero(mask > 0), rank its inverse, offsets the frame boundaries."""
    B, S = masks.shape[0], masks.shape[1]
    offsets, pix, frame, rank = NV.mask_to_pixels(masks)
    want = torch.nonzero(masks.reshape(B, S * S) > 0)
    n = want.shape[0]
    assert pix.dtype == frame.dtype == rank.dtype == offsets.dtype == torch.int32
    assert pix.shape == frame.shape == (n,) and rank.shape == (B, S, S) and offsets.shape == (B + 1,)
    assert torch.equal(frame.long(), want[:, 0]) and torch.equal(pix.long(), want[:, 1])
    inv = torch.full((B * S * S,), -1, device=masks.device, dtype=torch.int32)
    inv[want[:, 0] * S * S + want[:, 1]] = torch.arange(n, device=masks.device, dtype=torch.int32)
    assert torch.equal(rank.reshape(-1), inv)
    counts = (masks.reshape(B, -1) > 0).sum(1)
    assert offsets.tolist() == [0] + torch.cumsum(counts, 0).tolist()
    return offsets, pix, frame, rank


def mask_kinds(B, S, rng):
    yy, xx = np.mgrid[:S, :S]
    first, last = np.zeros((B, S, S), np.float32), np.zeros((B, S, S), np.float32)
    first[:, 0, 0] = 1
    last[:, -1, -1] = 1
    return {"empty": np.zeros((B, S, S), np.float32), "full": np.ones((B, S, S), np.float32), "first": first, "last": last,
            "checker": np.broadcast_to(((xx + yy) % 2).astype(np.float32), (B, S, S)).copy(),
            "rand40": (rng.random((B, S, S)) < 0.4).astype(np.float32)}


@pytest.mark.parametrize("S", [1, 7, 16, 33, 65])
@pytest.mark.parametrize("B", [1, 3])
def test_compaction_matches_nonzero(S, B):
    for kind, m in mask_kinds(B, S, rng_of(S, B)).items():
        check_list(T(m * np.float32(0.25)))                                   # fp32, a value that is not 1
        check_list(T((m * 200).astype(np.uint8)))                             # uint8


@pytest.mark.parametrize("S", [33, 65])
@pytest.mark.parametrize("count", [TILE - 1, TILE, TILE + 1])
def test_compaction_at_the_scan_tile(S, count):
    """Per-frame counts of one scan tile, one less, one more: as the frame's first pixels (the count crosses the first tile's
    end where the frame has a second tile) and scattered."""
    rng = rng_of(S, count)
    P = S * S
    lead = np.zeros((3, P), np.float32)
    lead[:, :count] = 1
    scat = np.zeros((3, P), np.float32)
    for b in range(3):
        scat[b, rng.permutation(P)[:count]] = 1
    for m in (lead, scat):
        offsets, _, _, _ = check_list(T(m.reshape(3, S, S)))
        assert offsets.tolist() == [0, count, 2 * count, 3 * count]
        check_list(T(m.reshape(3, S, S).astype(np.uint8)))


def test_compaction_middle_frame_empty_and_non_numbers():
    rng = rng_of(5)
    m = (rng.random((3, 33, 33)) < 0.4).astype(np.float32)
    m[1] = 0
    offsets, _, _, _ = check_list(T(m))
    assert offsets[1] == offsets[2] and 0 < offsets[1] < offsets[3]
    v = rng.normal(size=(2, 65, 65)).astype(np.float32)                       # negatives are out
    v[rng.random(v.shape) < 0.2] = np.nan
    v[rng.random(v.shape) < 0.2] = -0.0
    v[rng.random(v.shape) < 0.1] = 0.0
    v[rng.random(v.shape) < 0.05] = np.inf
    v[rng.random(v.shape) < 0.05] = -np.inf
    v[0, 0, :4] = [np.nan, -0.0, -1.0, np.float32(1e-45)]                     # the smallest subnormal is > 0
    _, pix, frame, _ = check_list(T(v))
    o_off, o_pix, o_frame, _ = O.mask_to_pixels(v)
    assert np.array_equal(np_(pix), o_pix) and np.array_equal(np_(frame), o_frame)
    assert np_(pix)[0] == 3 and np_(frame)[0] == 0


def test_compaction_ten_repeats_give_identical_bits():
    m = T((rng_of(9).random((3, 65, 65)) < 0.4).astype(np.float32))
    first = [t.clone() for t in NV.mask_to_pixels(m)]
    for _ in range(9):
        again = NV.mask_to_pixels(m)
        assert all(torch.equal(a, b) for a, b in zip(first, again))


# ---- rays -----------------------------------------------------------------------------------------------------------------
def rays_by_raycast(S, rtks, near_far, masks):
    """moda_amd.raycast on EVERY pixel of every frame, then torch indexing with the mask."""
    B = rtks.shape[0]
    _, xys = FD.sample_xy(S, B, 0, DEV, return_all=True)
    full = FD.raycast(xys, rtks[:, :3, :3], rtks[:, :3, 3], moda_amd.geom_utils.K2inv(rtks[:, 3]), near_far)
    keep = masks.reshape(B, S * S) > 0
    return {k: full[k][keep] for k in ("rays_o", "rays_d", "near", "far", "rtk_vec", "xys")}


@pytest.mark.parametrize("tag", ["nf", "auto"])
def test_rays_meet_the_reference_record_and_raycast_bit_for_bit(tag):
    g = golden("g37_nvs")
    S = int(g["img_size"])
    nf = T(g["near_far"]) if tag == "nf" else None
    rays = NV.construct_rays_nvs(S, g["rtks"], nf, g["masks"], DEV)
    n = int(g["counts"].sum())
    assert rays["nsample"] == n and rays["bs"] == 1
    want = rays_by_raycast(S, T(g["rtks"]), nf, T(g["masks"]))
    for k in ("rays_o", "rays_d", "near", "far", "rtk_vec", "xys"):
        assert rays[k].shape == (1, n, g[f"{tag}/{k}"].shape[1]), k
        assert torch.equal(rays[k][0], want[k]), k                            # exact, rays_d and rays_o included
        if k in ("rays_o", "rays_d"):
            assert rel_err(np_(rays[k][0]), g[f"{tag}/{k}"]) < RAYCAST_BAR, k
        else:
            assert np.array_equal(np_(rays[k][0]), g[f"{tag}/{k}"]), k


def test_rays_and_code_rows_on_an_odd_batch():
    """Off the golden's size: 5 frames of 33 x 33 (two tiles a frame), one frame empty, one mask for all cameras, code rows."""
    S, B = 33, 5
    rng = rng_of(33, 5)
    cam = synth.make_cameras(21, B)
    rtks = np.zeros((B, 4, 4), np.float32)
    rtks[:, :3, :3], rtks[:, :3, 3] = cam["Rmat"], cam["Tmat"]
    rtks[:, 3] = np.stack([rng.uniform(25, 45, B), rng.uniform(25, 45, B), rng.uniform(14, 19, B), rng.uniform(14, 19, B)], 1)
    m = (rng.random((B, S, S)) < 0.4).astype(np.float32)
    m[3] = 0
    nf = T(cam["near_far"])
    rays = NV.construct_rays_nvs(S, rtks, nf, m, DEV)
    want = rays_by_raycast(S, T(rtks), nf, T(m))
    for k in want:
        assert torch.equal(rays[k][0], want[k]), k
    one = NV.construct_rays_nvs(S, rtks, nf, m[0], DEV)                       # the reference's xys[:, rndmask] over bs cameras
    want = rays_by_raycast(S, T(rtks), nf, T(np.broadcast_to(m[0], (B, S, S)).copy()))
    for k in want:
        assert torch.equal(one[k][0], want[k]), k
    lst = NV._compact("test", T(m))
    rows = {"env_code": T(rng.normal(size=(B, 64)).astype(np.float32)), "time_embedded": T(rng.normal(size=(B, 1, 128)).astype(np.float32)),
            "bone_rts": T(rng.normal(size=(B, 1, 8 * 25)).astype(np.float32))}
    src = {k: v.reshape(B, -1).clone() for k, v in rows.items()}
    got = NV._rays("test", lst, S, T(rtks)[:, :3, :3].contiguous(), T(rtks)[:, :3, 3].contiguous(),
                   moda_amd.geom_utils.K2inv(T(rtks)[:, 3]).contiguous(), nf, rows=dict(rows))
    for k, v in src.items():
        assert got[k].shape == (1, lst.pix.shape[0], v.shape[1]) and torch.equal(got[k][0], v[lst.frame.long()]), k
    assert torch.equal(got["rays_d"], rays["rays_d"])


def test_empty_list_launches_nothing_and_assembles_ones():
    S, B = 7, 2
    rtks = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    rtks[:, 3] = [10, 10, 3, 3]
    rays = NV.construct_rays_nvs(S, rtks, None, np.zeros((B, S, S)), DEV)
    assert rays["nsample"] == 0 and rays["rays_d"].shape == (1, 0, 3) and rays["rtk_vec"].shape == (1, 0, 21)
    _, _, _, rank = NV.mask_to_pixels(T(np.zeros((B, S, S), np.float32)))
    e = lambda c: torch.empty((0, c), device=DEV)
    fr = NV.assemble_frames(rank, e(3), e(1), e(1), e(1), to_uint8=True)
    assert all(bool((t == 1).all()) for t in (fr.rgb, fr.depth, fr.sil, fr.vis))
    assert all(bool((t == 255).all()) for t in (fr.rgb8, fr.sil8, fr.vis8)) and fr.rgb8.shape == (B, S, S, 3)


# ---- assembly -------------------------------------------------------------------------------------------------------------
def exact_halves():
    """fp32 values v with v * 255 == k + 0.5 exactly in fp32."""
    out = []
    for k in range(255):
        v = np.float32((k + 0.5) / 255)
        for c in (v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(1))):
            if np.float32(c) * np.float32(255) == np.float32(k + 0.5):
                out.append(c)
                break
    return np.asarray(out, np.float32)


def test_assembly_is_exact_against_the_oracle():
    S, B = 19, 3
    rng = rng_of(19, 3)
    m = (rng.random((B, S, S)) < 0.6).astype(np.float32)
    m[1] = 0
    n = int(m.sum())
    halves = exact_halves()
    assert len(halves) > 100 and {0.5, 1.5, 2.5} <= set((halves * np.float32(255)).tolist())
    sil = rng.random(n).astype(np.float32)
    sil[:4] = [0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nan, np.nextafter(np.float32(0.5), np.float32(1))]
    sil[4:4 + 60] = halves[rng.integers(128, len(halves), 60)]               # halves at or above 0.5: they survive the threshold
    rgb = rng.random((n, 3)).astype(np.float32) * np.float32(1.2) - np.float32(0.1)   # some below 0, some above 1
    rgb.reshape(-1)[:len(halves)] = halves
    rgb[-1] = [np.nan, np.inf, -np.inf]
    sil[-1] = 0.75
    dep = (rng.random(n) * 3).astype(np.float32)
    vis = rng.random(n).astype(np.float32)
    vis[:len(halves)] = halves[rng.permutation(len(halves))]
    vis[-2] = np.nan
    _, _, _, rank = NV.mask_to_pixels(T(m))
    fr = NV.assemble_frames(rank, T(rgb), T(dep), T(sil)[:, None], T(vis), to_uint8=True)
    want = O.assemble(m, rgb, dep, sil, vis)
    for name, got, w in zip(("rgb", "depth", "sil", "vis"), fr[:4], want):
        assert got.dtype == torch.float32 and np.array_equal(np_(got), w, equal_nan=True), name
    for name, got, w in zip(("rgb8", "sil8", "vis8"), fr[4:7], (want[0], want[2], want[3])):
        assert got.dtype == torch.uint8 and np.array_equal(np_(got), O.to_uint8(w)), name
    assert fr.offsets is None
    plain = NV.assemble_frames(rank, T(rgb), T(dep), T(sil), T(vis))
    assert plain.rgb8 is None and all(np.array_equal(np_(a), np_(b), equal_nan=True) for a, b in zip(plain[:4], fr[:4]))


# ---- end to end -----------------------------------------------------------------------------------------------------------
def mock_model(bones=25):
    """The model protocol of feeders.update_rays, as test_gpu_feeders builds it, with the visibility network."""
    models, emb = make_models(13, bones, with_skin=True, with_vis=True)
    model = types.SimpleNamespace(nerf_models=models, embeddings=emb, opts=make_opts(num_bones=bones, ndepth=16, chunk=100))
    model.pose_code = FD.FrameCode(6, 128, np.asarray([0, 50])).to(DEV)
    model.env_code = FD.FrameCode(6, 64, np.asarray([0, 50])).to(DEV)
    head = FD.DQ_RTHead(use_quat=True, in_channels_xyz=128, in_channels_dir=0, out_channels=7 * bones, raw_feat=True).to(DEV)
    with torch.no_grad():
        head.rgb[0].weight.mul_(0.05)
        head.rgb[0].bias.copy_(torch.tensor([0, 0, 0, 1, 0, 0, 0.0], device=DEV).repeat(bones))
    model.nerf_body_rts = torch.nn.Sequential(model.pose_code, head)
    model.rest_pose_code = models["rest_pose_code"]
    v = synth.uniform(13, "nvs/verts", (200, 3)) * np.float32(0.4) - np.float32(0.2)
    model.latest_vars = {"obj_bound": np.asarray([0.2, 0.2, 0.2], np.float32), "mesh_rest": types.SimpleNamespace(vertices=v)}
    return model


def scene(S, B):
    rng = rng_of(S, B, 77)
    cam = synth.make_cameras(13, B)
    rtks = np.zeros((B, 4, 4), np.float32)
    rtks[:, :3, :3], rtks[:, :3, 3] = cam["Rmat"], cam["Tmat"]
    rtks[:, 3] = [2.0 * S, 2.0 * S, S / 2, S / 2]
    yy, xx = np.mgrid[:S, :S]
    m = np.zeros((B, S, S), np.float32)
    m[0] = ((xx - S / 2 + 0.5) ** 2 + (yy - S / 2 + 0.5) ** 2 < (0.45 * S) ** 2)
    m[2] = rng.random((S, S)) < 0.7
    return rtks, m, torch.arange(B, device=DEV) * 7 + 3


def per_frame_loop(model, S, rtks, masks, embedid, near_far, ndepth):
    """nvs.py:109-174 one frame at a time: construct_rays_nvs, the codes repeated over the frame's rays, ONE render_rays call a
    frame, torch indexing into `ones` canvases."""
    B = rtks.shape[0]
    ones = lambda *s: torch.ones(s, device=DEV)
    rgbs, deps, sils, viss = ones(B, S, S, 3), ones(B, S, S), ones(B, S, S), ones(B, S, S)
    with torch.no_grad():
        for i in range(B):
            rays = NV.construct_rays_nvs(S, rtks[i:i + 1], near_far[i:i + 1], masks[i], DEV)
            n = rays["nsample"]
            if n == 0:
                continue
            rays["env_code"] = model.env_code(embedid[i:i + 1])[:, None].repeat(1, n, 1)
            rays["time_embedded"] = model.pose_code(embedid[i:i + 1])[:, None].repeat(1, n, 1)
            rays["bone_rts"] = model.nerf_body_rts(embedid[i:i + 1]).repeat(1, n, 1)
            FD.update_delta_rts(model, rays)
            out = moda_amd.render_rays(model.nerf_models, model.embeddings, FD.chunk_rays(rays, 0, n), N_samples=ndepth, perturb=0,
                                       noise_std=0, chunk=n, use_fine=True, img_size=S, obj_bound=model.latest_vars["obj_bound"],
                                       render_vis=True, opts=model.opts)
            rgb, dep = out["img_coarse"].reshape(n, 3).clone(), out["depth_rnd"].reshape(n)
            sil, vis = out["sil_coarse"].reshape(n).clone(), out["vis_pred"].reshape(n)
            sil[sil < 0.5] = 0
            rgb[sil < 0.5] = 1
            keep = torch.as_tensor(masks[i], device=DEV) > 0
            rgbs[i][keep], deps[i][keep], sils[i][keep], viss[i][keep] = rgb, dep, sil, vis
    return rgbs, deps, sils, viss


@pytest.mark.parametrize("precision", ["fp32"])
def test_render_nvs_equals_the_per_frame_loop_bit_for_bit(precision):
    """S = 16, ndepth = 16, 3 frames with the middle one empty, chunk = 100: chunks straddle frames, the loop renders a frame a
    call.  All four canvases bit-equal: the renderer is chunk-invariant in the exact-fp32 mode."""
    S, B = 16, 3
    prev = moda_amd.get_precision()
    moda_amd.set_precision(precision)
    try:
        model = mock_model()
        rtks, m, eid = scene(S, B)
        nf = T(np.asarray([[0.6, 1.4]] * B, np.float32))
        fr = NV.render_nvs(model, rtks, T(m), eid, near_far=nf, ndepth=16, chunk=100)
        want = per_frame_loop(model, S, rtks, m, eid, nf, 16)
    finally:
        moda_amd.set_precision(prev)
    counts = (m > 0).reshape(B, -1).sum(1)
    assert fr.offsets.tolist() == [0] + np.cumsum(counts).tolist() and counts[1] == 0
    assert counts[0] % 100 and counts.sum() > 200                             # a chunk straddles the frames 0 and 2
    for name, got, w in zip(("rgb", "depth", "sil", "vis"), fr[:4], want):
        print(name, "max |diff|", float((got - w).abs().max()), "inside-mask mean", float(got[T(m) > 0].mean()))
        assert torch.equal(got, w), name
        assert bool((got[T(m) <= 0] == 1).all()) and bool(torch.isfinite(got).all()), name
    assert bool((fr.depth[T(m) > 0] != 1).any())
    assert fr.rgb8 is None


def test_render_nvs_defaults_scale_near_far_and_uint8():
    """near_far=None is get_near_far over mesh_rest's vertices with every frame seen; scale multiplies the intrinsics row;
    ndepth and chunk default to the model's opts; to_uint8 adds the 8-bit images of the same canvases."""
    from moda_amd.frame_state import FrameState, get_near_far
    S, B = 16, 3
    prev = moda_amd.get_precision()
    moda_amd.set_precision("fp32")
    try:
        model = mock_model()
        rtks, m, eid = scene(S, B)
        big = rtks.copy()
        big[:, 3] *= 4
        fr = NV.render_nvs(model, big, T(m), eid, scale=0.25, to_uint8=True)
        state = FrameState(B, DEV)
        state["rtk"], state["idk"] = rtks, np.ones(B)
        nf = get_near_far(torch.zeros(B, 2, device=DEV), state, pts=model.latest_vars["mesh_rest"].vertices)
        want = NV.render_nvs(model, rtks, T((m * 255).astype(np.uint8)), eid, near_far=nf, ndepth=16, chunk=100)
    finally:
        moda_amd.set_precision(prev)
    assert bool((nf[:, 1] > nf[:, 0]).all())
    for name, got, w in zip(("rgb", "depth", "sil", "vis"), fr[:4], want[:4]):
        assert torch.equal(got, w), name
    for got, src in ((fr.rgb8, fr.rgb), (fr.sil8, fr.sil), (fr.vis8, fr.vis)):
        assert np.array_equal(np_(got), O.to_uint8(np_(src)))
    crop = NV.crop_short_edge(fr, 3, 4)
    assert crop.rgb.shape == (B, 12, S, 3) and crop.vis8.shape == (B, 12, S) and torch.equal(crop.sil, fr.sil[:, :12])
