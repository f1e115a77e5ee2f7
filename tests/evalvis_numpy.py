"""numpy restatement of moda_amd/eval_frames.py, float64 unless the input says otherwise: flow_to_image / compute_color /
make_color_wheel (third_party/ext_utils/flowlib.py:86-214), image_grid (nnutils/vis_utils.py:5-16), the canvas block of
v2s_trainer.eval() (nnutils/train_utils.py:496-520), add_image (:1493-1504) and save_vid's frames (utils/io.py:242-258).
flow_to_image and image_grid are pinned to the reference's own functions by tests/test_evalvis_oracle.py
(tests/golden/g39_evalvis.npz); the eval() block and save_vid are methods behind heavy imports: restated, unpinned."""
import numpy as np

FLOW_TAGS = ('flo_coarse', 'fdp_coarse', 'flo', 'fdp', 'flo_at_samp')
SCALED_TAGS = ('depth_rnd', 'occ', 'unc_pred', 'proj_err', 'feat_err')
UNKNOWN = 1e7
EPS = 2.220446049250313e-16


def color_wheel():
    """make_color_wheel, statement by statement."""
    RY, YG, GC, CB, BM, MR = 15, 6, 4, 11, 13, 6
    w = np.zeros((RY + YG + GC + CB + BM + MR, 3))
    c = 0
    w[0:RY, 0] = 255
    w[0:RY, 1] = np.floor(255 * np.arange(0, RY) / RY)
    c += RY
    w[c:c + YG, 0] = 255 - np.floor(255 * np.arange(0, YG) / YG)
    w[c:c + YG, 1] = 255
    c += YG
    w[c:c + GC, 1] = 255
    w[c:c + GC, 2] = np.floor(255 * np.arange(0, GC) / GC)
    c += GC
    w[c:c + CB, 1] = 255 - np.floor(255 * np.arange(0, CB) / CB)
    w[c:c + CB, 2] = 255
    c += CB
    w[c:c + BM, 2] = 255
    w[c:c + BM, 0] = np.floor(255 * np.arange(0, BM) / BM)
    c += BM
    w[c:c + MR, 2] = 255 - np.floor(255 * np.arange(0, MR) / MR)
    w[c:c + MR, 0] = 255
    return w


def flow_to_image(flow, after=np.float64):
    """One frame (H, W, C >= 2) -> (img uint8 (H, W, 3), pre (H, W, 3) float64 = 255 col before the floor, exact (H, W, 3) bool =
    channels exact by construction (both wheel entries 255 inside the unit circle, both 0 outside it, radius 0, or forced to
    0), top (H, W) bool = pixels of the frame's maximal radius, alt uint8 (H, W, 3) = what the other branch of `rad <= 1` gives).  The radius and its maximum are taken in
    flow.dtype; `after` is the dtype of u, v, radius, angle and fk after the division (float64: numpy >= 2 on any input and
    every numpy on a float64 input; float32: numpy < 2 on an fp32 input).  The caller's array is not written."""
    dt = flow.dtype.type
    u, v = flow[..., 0].copy(), flow[..., 1].copy()
    unknown = (np.abs(u) > dt(UNKNOWN)) | (np.abs(v) > dt(UNKNOWN))
    u[unknown] = 0
    v[unknown] = 0
    with np.errstate(invalid="ignore"):
        rad0 = np.sqrt(u * u + v * v)
        m = np.max(rad0)
        top = rad0 == m
        if m != m:                                             # max(-1, nan) returns its first argument
            den = after(-1) if after is np.float32 else np.float64(-1) + EPS
        elif after is np.float32:
            den = np.float32(m) + np.float32(EPS)
        else:
            den = np.float64(m) + EPS
        u, v = u.astype(after) / den, v.astype(after) / den
        nan = np.isnan(u) | np.isnan(v)
        u[nan] = 0
        v[nan] = 0
        wheel = color_wheel()
        rad = np.sqrt(u * u + v * v)
        a = np.arctan2(-v, -u) / after(np.pi)
        fk = (a + after(1)) / after(2) * after(54) + after(1)
        k0 = np.floor(fk).astype(int)
        k1 = k0 + 1
        k1[k1 == 56] = 1
        f = fk.astype(np.float64) - k0
    H, W = u.shape
    pre, alt, exact = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W, 3), bool)
    inside = rad <= 1
    for i in range(3):
        c0, c1 = wheel[k0 - 1, i] / 255, wheel[k1 - 1, i] / 255
        col = (1 - f) * c0 + f * c1
        near = 1 - rad.astype(np.float64) * (1 - col)
        far = col * 0.75
        keep = 1 - nan
        pre[..., i] = 255 * np.where(inside, near, far) * keep
        alt[..., i] = 255 * np.where(inside, far, near) * keep
        both = lambda val: (wheel[k0 - 1, i] == val) & (wheel[k1 - 1, i] == val)
        exact[..., i] = (both(255) & inside) | (both(0) & ~inside) | (rad == 0) | nan | unknown
    pre[unknown] = 0
    alt[unknown] = 0
    return np.uint8(np.floor(pre)), pre, exact, top & ~unknown & ~nan, np.uint8(np.clip(np.floor(alt), 0, 255))


def flow_to_images(flow, after=np.float64):
    """(N, H, W, C) -> the stacked fields of flow_to_image."""
    return tuple(np.stack(x) for x in zip(*(flow_to_image(f, after) for f in flow)))


def image_grid(img, row, col):
    bs, h, w, c = img.shape
    out = np.zeros((h * row, w * col, c), img.dtype)
    for i in range(row):
        for j in range(col):
            out[i * h:(i + 1) * h, j * w:(j + 1) * w] = img[i * col + j]
    return out


def nearest_resize(mask, S):
    """F.interpolate(mask[:, None], (S, S)) (mode 'nearest'): src = min(floor(dst * fp32(Sm / S)), Sm - 1), the product in fp32."""
    Sm = mask.shape[1]
    scale = np.float32(Sm) / np.float32(S)
    idx = np.minimum(np.floor(np.arange(S, dtype=np.float32) * scale).astype(int), Sm - 1)
    return mask[:, idx][:, :, idx]


def eval_canvases(rendered, masks, use_embed=True, use_proj=True, use_unc=True):
    """train_utils.py:496-520 on float64 copies -> {key: array} of the keys the block changes (the others pass through)."""
    r = {k: np.asarray(v, np.float64).copy() for k, v in rendered.items()}
    hbs, S = next(iter(r.values())).shape[:2]
    sil = nearest_resize(np.asarray(masks, np.float64)[:hbs], S)[..., None]
    out = {}
    with np.errstate(all="ignore"):
        out['flo_coarse'] = r['flo_coarse'] * sil
        out['img_loss_samp'] = r['img_loss_samp'] * sil
        if 'frame_cyc_dis' in r:
            out['frame_cyc_dis'] = r['frame_cyc_dis'] * (255 / r['frame_cyc_dis'].max())
        if use_embed:
            out['pts_pred'] = r['pts_pred'] * sil
            out['pts_exp'] = r['pts_exp'] * r['sil_coarse']
            e = r['feat_err'] * sil
            out['feat_err'] = e * (255 / e.max())
        if use_proj:
            e = r['proj_err'] * sil
            out['proj_err'] = e * (255 / e.max())
        if use_unc:
            e = r['unc_pred'] - r['unc_pred'].min()
            out['unc_pred'] = e * (255 / e.max())
    return out


def to_display(tag, grid):
    if tag in FLOW_TAGS:
        return flow_to_image(np.asarray(grid))[0]
    g = np.asarray(grid)
    with np.errstate(all="ignore"):
        if tag in SCALED_TAGS:
            return (g - g.min()) / (g.max() - g.min())
        return np.where(np.isnan(g), g, np.clip(g, 0, 1))


def to_u8(v):
    """The package's float -> uint8 rule: truncate toward zero, saturate to [0, 255], NaN -> 0 -> (uint8, #saturated, #NaN)."""
    v = np.asarray(v)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        sat = (v <= -1) | (v >= 256)
        out = np.trunc(np.clip(np.where(nan, 0, v), 0, 255)).astype(np.uint8)
    return out, int(sat.sum()), int(nan.sum())


def video_frames(frames, upsample_frame, is_flow, after=np.float64):
    """save_vid up to the uint8 frame, fp32 arithmetic where the reference's is (frame * 255) -> (frames, #saturated, #NaN)."""
    n = len(frames)
    if upsample_frame < 1:
        upsample_frame = n
    out, ns, nn = [], 0, 0
    for i in range(int(upsample_frame)):
        frame = frames[int(i / upsample_frame * n)]
        if is_flow:
            frame = flow_to_image(frame, after)[0].astype(np.float32)
        with np.errstate(invalid="ignore"):
            if frame.max() <= 1:
                frame = frame * np.float32(255)
        f8, s, m = to_u8(frame)
        out.append(f8)
        ns, nn = ns + s, nn + m
    return np.stack(out), ns, nn
