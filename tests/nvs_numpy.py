"""The numpy restatement of the two ends of scripts/visualize/nvs.py around render_rays: construct_rays_nvs (:41-55) and the
thresholding, the `ones` canvases and the crop (:160-185), plus the stated 8-bit rule.  Everything here selects, copies or does
a handful of fp32 operations, so the GPU tests hold the kernels to it exactly, except rays_d / rays_o, whose bar is raycast's."""
import numpy as np

F32 = np.float32


def mask_to_pixels(masks):
    """masks (B, S, S) -> offsets (B + 1), pix, frame (n), rank (B, S, S): `value > 0` decides (NaN, -0.0, negatives are out),
    frame-major and row-major, the order of xys[:, rndmask]."""
    masks = np.asarray(masks)
    B, S = masks.shape[0], masks.shape[1]
    with np.errstate(invalid="ignore"):
        keep = masks.reshape(B, S * S) > 0
    frame, pix = np.nonzero(keep)
    offsets = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int32)
    rank = np.full(B * S * S, -1, np.int32)
    rank[frame * S * S + pix] = np.arange(pix.size, dtype=np.int32)
    return offsets, pix.astype(np.int32), frame.astype(np.int32), rank.reshape(B, S, S)


def K2inv(K):
    """geom_utils.py:638-652 in fp32: quotients, not a matrix inverse."""
    K = np.asarray(K, F32).reshape(-1, 4)
    Kmat = np.zeros((K.shape[0], 3, 3), F32)
    Kmat[:, 0, 0] = F32(1) / K[:, 0]
    Kmat[:, 1, 1] = F32(1) / K[:, 1]
    Kmat[:, 0, 2] = -K[:, 2] / K[:, 0]
    Kmat[:, 1, 2] = -K[:, 3] / K[:, 1]
    Kmat[:, 2, 2] = 1
    return Kmat


def construct_rays_nvs(img_size, rtks, near_far, masks):
    """nvs.py:41-55 for a batch, flat layout: sample_xy(return_all)[:, mask] per frame, K2inv, raycast (float64 products rounded
    once: the bar against fp32 is raycast's 1e-5)."""
    rtks = np.asarray(rtks, F32)
    S = int(img_size)
    masks = np.asarray(masks).reshape(rtks.shape[0], S, S)
    _, pix, frame, _ = mask_to_pixels(masks)
    xys = np.stack([pix % S, pix // S], -1).astype(F32)
    Rmat, Tmat, Kinv = rtks[:, :3, :3], rtks[:, :3, 3], K2inv(rtks[:, 3])
    xy1 = np.concatenate([xys, np.ones_like(xys[:, :1])], 1).astype(np.float64)
    v = np.einsum("nj,nij->ni", xy1, Kinv[frame].astype(np.float64))            # xy1s.matmul(Kinv^T)
    rays_d = np.einsum("ni,nij->nj", v, Rmat[frame].astype(np.float64))          # .matmul(Rmat)
    rays_o = -np.einsum("ni,nij->nj", Tmat[frame].astype(np.float64), Rmat[frame].astype(np.float64))
    if near_far is None:
        z = Tmat[:, 2]
        near_far = np.stack([np.maximum(z - F32(1.5), F32(1e-5)), z + F32(1.5)], 1)
    near_far = np.asarray(near_far, F32)
    rtk_vec = np.concatenate([Rmat.reshape(-1, 9), Tmat, Kinv.reshape(-1, 9)], 1)
    n = pix.size
    return {"rays_o": rays_o.astype(F32)[None], "rays_d": rays_d.astype(F32)[None], "near": near_far[frame, 0].reshape(1, n, 1),
            "far": near_far[frame, 1].reshape(1, n, 1), "rtk_vec": rtk_vec[frame][None], "xys": xys[None], "nsample": n, "bs": 1}


def to_uint8(v):
    """clip(rint(v * 255), 0, 255): the product in fp32, round half to even, NaN -> 0."""
    with np.errstate(invalid="ignore"):
        t = np.asarray(v, F32) * F32(255)
        r = np.clip(np.rint(t), 0, 255)
    return np.where(np.isnan(t), 0, r).astype(np.uint8)


def assemble(masks, rgb, depth, sil, vis):
    """nvs.py:160-174 per frame with the reference's own statements, canvases in fp32: -> rgb (B,S,S,3), depth, sil, vis (B,S,S)."""
    masks = np.asarray(masks)
    B, S = masks.shape[0], masks.shape[1]
    offsets, _, _, _ = mask_to_pixels(masks)
    out = [np.ones((B, S, S, 3), F32), np.ones((B, S, S), F32), np.ones((B, S, S), F32), np.ones((B, S, S), F32)]
    for b in range(B):
        lo, hi = offsets[b], offsets[b + 1]
        r, d, s, v = (np.array(a, F32).reshape(len(a), -1)[lo:hi] for a in (rgb, depth, sil, vis))
        d, s, v = d[:, 0], s[:, 0], v[:, 0]
        with np.errstate(invalid="ignore"):
            s[s < 0.5] = 0
            r[s < 0.5] = 1
            m = masks[b] > 0
        out[0][b][m] = r
        out[1][b][m] = d
        out[2][b][m] = s
        out[3][b][m] = v
    return tuple(out)


def crop_short_edge(canvas, h, w, rgb=False):
    """nvs.py:176-185 on a (B, S, S[, 3]) canvas."""
    S = canvas.shape[1]
    if h > w:
        return canvas[:, :, :int(w * S / h)]
    return canvas[:, :int(h * S / w)]
