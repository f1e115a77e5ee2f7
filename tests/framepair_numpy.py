"""Float64 restatement of moda_amd/frame_pairs.py (the reference's compute_crop_params, the cv2.remap calls of read_raw,
flow_process / warp_flow, fb_flow_check and convert_batch_input's order), in the operation order include/moda_hip.h states for the
kernels, with the fp32 error bounds the tests hold the kernels to.  Every function returns (value, bound).

The sampler (cv2.remap with float maps, INTER_LINEAR / INTER_NEAREST, constant-zero border) is restated from OpenCV's source; it
has not been run against OpenCV.  Linear: sx = rne(fp32(x * 32)), cell sx >> 5, fraction sx & 31, weights the four products of
(1 - f/32, f/32), a tap outside the image contributes 0.  Nearest: rne(x), 0 outside.  A NaN / infinite coordinate samples 0.

Bounds (u = 2^-24, gamma_n = n u / (1 - n u); v = 2^-53 for float64):
  * box, crop parameters, crop coordinates, nearest planes: exact, bound 0.  The coordinate is one float64 multiply and one add
    and one rounding to fp32, which numpy's element-wise arithmetic reproduces bit for bit.
  * linear sample of fp32 planes.  The weights are exact; each product is rounded once and passes through at most three
    additions: |err| <= gamma_4 sum_i |v_i| w_i.  The uint8 image divides every tap by 255 first: gamma_5.
  * flow_process, flow.  fs = fp32(((flow + hp) - t') / a' - p) is four float64 operations on terms of size
    M = (|flow| + |hp| + |t'|) / |a'| + |p|, then one fp32 rounding.  The oracle rounds too (it restates the
    reference's fp32 storage), so two values each within u |fs| of nearly the same number are compared: e_fs = 8 v M + 2 u |fs|.  The 8 v M term also covers the
    reference's np.linalg.inv against the closed form used here.  out = 2 fp32(fs / S), again rounded on both sides: bound = 2 e_fs / S + 2 u |out|.
  * flow_process, occ.  The map m = fp32(fs + p) has error e_m = e_fs + u |m|.  When rne(32 m) does not flip (exemption (a):
    32 m within 32 e_m of a half-integer), cell and weights are the same, the tap values p_i + fs_i carry e_fs,i and the float64
    blend is exact to ~1e-15: e_dis <= sqrt(2) sum_i w_i max(e_fs,i) (the norm is 1-Lipschitz).  occ = exp(-50 dis / S) has
    |d occ / d dis| <= 50 / S: bound = 50 e_dis / S + 2 u occ + 1e-14.  Exemption (b): |occ - 0.25| <= bound (the zeroing flips).
  * remap / warp_flow / fb_flow_check through moda_remap are fp32 throughout: gamma_4 sum |v_i| w_i for the sample, plus, for
    warp_flow, the exemption (a) with e_m = u |m| + the caller's input error.
"""
import numpy as np

U32 = 2.0 ** -24
V64 = 2.0 ** -53


def gamma(n):
    return n * U32 / (1 - n * U32)


# ---- box and crop parameters ----------------------------------------------------------------------------------------------------
def mask_bbox(masks):
    """masks (B,h,w) -> (box (B,4) int32 = xmin, xmax, ymin, ymax; an empty mask: (w, -1, h, -1)), 0."""
    masks = np.asarray(masks)
    B, h, w = masks.shape
    box = np.empty((B, 4), np.int32)
    for b in range(B):
        with np.errstate(invalid="ignore"):
            ys, xs = np.where(masks[b] > 0)
        box[b] = (w, -1, h, -1) if len(xs) == 0 else (xs.min(), xs.max(), ys.min(), ys.max())
    return box, 0


def pair_major_rows(B):
    """Output row -> input frame for B = 2 bs frames given as (pair, k): row k bs + p holds frame 2 p + k."""
    bs = B // 2
    return np.asarray([(o % bs) * 2 + o // bs for o in range(B)])


def compute_crop_params(box, img_size, crop_factor=1.2, pair_major=False):
    """box (B,4) -> ((kaug (B,4) fp32, affine (B,4) float64, status [#empty, #zero-length]), 0); refused rows are NaN."""
    box = np.asarray(box, np.int64)
    B = box.shape[0]
    aff = np.full((B, 4), np.nan)
    status = np.zeros(2, np.int32)
    for f in range(B):
        x0, x1, y0, y1 = (int(v) for v in box[f])
        if x1 < x0 or y1 < y0:
            status[0] += 1
            continue
        center = ((x1 + x0) // 2, (y1 + y0) // 2)
        length = ((x1 - x0) // 2, (y1 - y0) // 2)
        length = (int(crop_factor * length[0]), int(crop_factor * length[1]))
        if length[0] == 0 or length[1] == 0:
            status[1] += 1
            continue
        aff[f] = (2 * length[0] / img_size, 2 * length[1] / img_size, float(center[0] - length[0]), float(center[1] - length[1]))
    if pair_major:
        aff = aff[pair_major_rows(B)]
    return (aff.astype(np.float32), aff, status), 0


def crop_coords(aff_row, S):
    """The fp32 source coordinates of an S x S crop: x (S,S), y (S,S), bit for bit."""
    ar = np.arange(S, dtype=np.float64)
    x = (ar * aff_row[0] + aff_row[2]).astype(np.float32)
    y = (ar * aff_row[1] + aff_row[3]).astype(np.float32)
    return np.broadcast_to(x[None, :], (S, S)), np.broadcast_to(y[:, None], (S, S))


# ---- the sampler ----------------------------------------------------------------------------------------------------------------
def _fixed5(x):
    """fp32 coordinate -> (cell, fraction, usable)."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.asarray(x, np.float32) * np.float32(32)
        ok = np.abs(s) < 2.0 ** 30
    i = np.rint(np.where(ok, s, 0)).astype(np.int64)                      # np.rint: round half to even
    return i >> 5, i & 31, ok


def linear_taps(x, y):
    """-> x0, y0 (int64), w (4, ...) float64 (exact in fp32) in the order (x0,y0), (x0+1,y0), (x0,y0+1), (x0+1,y0+1), usable."""
    x0, fx, okx = _fixed5(x)
    y0, fy, oky = _fixed5(y)
    ax, ay = fx / 32.0, fy / 32.0
    w = np.stack([(1 - ay) * (1 - ax), (1 - ay) * ax, ay * (1 - ax), ay * ax])
    return x0, y0, w, okx & oky


def _tap(plane, xi, yi):
    H, W = plane.shape
    inside = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
    return np.where(inside, plane[np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)], 0.0), inside


def sample_linear(plane, x, y, n_round=4):
    """plane (H,W) -> (value float64, bound) at fp32 coordinates x, y: ((v00 w00 + v01 w01) + v10 w10) + v11 w11."""
    plane = np.asarray(plane, np.float64)
    x0, y0, w, ok = linear_taps(x, y)
    val = np.zeros(np.shape(x))
    mag = np.zeros(np.shape(x))
    for k in range(4):
        v, _ = _tap(plane, x0 + (k & 1), y0 + (k >> 1))
        val = val + v * w[k]
        mag = mag + np.abs(v) * w[k]
    return np.where(ok, val, 0.0), np.where(ok, gamma(n_round) * mag, 0.0)


def sample_nearest(plane, x, y):
    """plane (H,W) -> ((value, inside), 0): the pixel (rne(x), rne(y)), 0 outside."""
    plane = np.asarray(plane)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(x) < 2.0 ** 30) & (np.abs(y) < 2.0 ** 30)
    xi = np.rint(np.where(ok, x, -1)).astype(np.int64)
    yi = np.rint(np.where(ok, y, -1)).astype(np.int64)
    v, inside = _tap(plane, xi, yi)
    return (np.where(ok, v, 0), inside & ok), 0


def remap(src, map_x, map_y, interpolation=1):
    """src (C,Hs,Ws) fp32 planes, maps (H,W) fp32 -> (value (C,H,W) float64, bound)."""
    src = np.asarray(src)
    mx, my = np.asarray(map_x, np.float32), np.asarray(map_y, np.float32)
    if interpolation == 0:
        return np.stack([sample_nearest(p, mx, my)[0][0] for p in src]).astype(np.float64), np.zeros((src.shape[0],) + mx.shape)
    parts = [sample_linear(p, mx, my) for p in src]
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])


def half_integer_risk(m64, e_m):
    """Exemption (a): 32 m within 32 e_m of a half-integer (the rne of the 1/32 lattice may flip); NaN never flips (it is 0)."""
    s = 32.0 * np.asarray(m64, np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(s - np.floor(s) - 0.5)
        return np.nan_to_num(d, nan=1.0, posinf=1.0) <= 32.0 * np.nan_to_num(e_m, nan=0.0, posinf=0.0)


def warp_flow(img, flow, normed=False, e_in=0.0):
    """img (C,h,w), flow (2,h,w) fp32 -> (value, bound, exempt (h,w)); e_in: the absolute error of `flow` as given."""
    flow = np.asarray(flow, np.float32)
    h, w = flow.shape[1:]
    fx, fy = flow[0], flow[1]
    if normed:
        fx, fy = fx * np.float32(w) / np.float32(2), fy * np.float32(h) / np.float32(2)
    mx = (fx + np.arange(w, dtype=np.float32)[None, :]).astype(np.float32)
    my = (fy + np.arange(h, dtype=np.float32)[:, None]).astype(np.float32)
    val, bound = remap(img, mx, my, 1)
    ex = half_integer_risk(mx, e_in + 3 * U32 * np.abs(mx)) | half_integer_risk(my, e_in + 3 * U32 * np.abs(my))
    return val, bound, ex


def fb_flow_check(flo_refr, flo_targ):
    """Two NDC flows (2,h,w) fp32 -> ((fberr_fw, fberr_bw), (bound_fw, bound_bw), (exempt_fw, exempt_bw)).  The image hp0 + flow
    is formed in fp32 by the product (u per tap, on values up to w + |flow|), the reference forms it in float64."""
    a, b = np.asarray(flo_refr, np.float32), np.asarray(flo_targ, np.float32)
    h, w = a.shape[1:]
    hp0 = np.stack(np.meshgrid(np.arange(w), np.arange(h))).astype(np.float64)
    vals, bounds, exs = [], [], []
    for p, q in ((a, b), (b, a)):
        p_px, q_px = (p * np.float32(w) / np.float32(2)).astype(np.float32), (q * np.float32(w) / np.float32(2)).astype(np.float32)
        img = (hp0 + q_px).astype(np.float32)
        res, bnd, ex = warp_flow(img, p_px, e_in=0.0)
        bnd = bnd + 2 * U32 * (np.abs(res) + 1)                           # the taps' own rounding, the subtraction
        fb = 2 * (res - hp0) / w
        err = np.sqrt(fb[0] ** 2 + fb[1] ** 2)
        ebound = 2 * np.sqrt(bnd[0] ** 2 + bnd[1] ** 2) / w + 6 * U32 * (err + np.abs(fb).sum(0))
        live = np.sqrt(p[0].astype(np.float64) ** 2 + p[1].astype(np.float64) ** 2) > 0
        vals.append(np.where(live, err, 0.0))
        bounds.append(np.where(live, ebound, 0.0))
        exs.append(ex & live)
    return tuple(vals), tuple(bounds), tuple(exs)


# ---- the crop -------------------------------------------------------------------------------------------------------------------
def crop_frames(affine, S, img=None, flow=None, occ=None, mask=None, dp=None, pair_major=False):
    """affine (B,4) in OUTPUT order; planes (B,h,w[,C]) in input order ((pair, k) flattened when pair_major) ->
    (dict of float64 arrays 'imgs' (B,3,S,S), 'flow' (B,2,S,S), 'occ', 'masks', 'dps', 'vis2d' (B,S,S), dict of bounds)."""
    B = affine.shape[0]
    src = pair_major_rows(B) if pair_major else np.arange(B)
    names = [n for n, t in (("imgs", img), ("flow", flow), ("occ", occ), ("masks", mask), ("dps", dp)) if t is not None] + ["vis2d"]
    ch = {"imgs": 3, "flow": 2}
    out = {n: np.zeros((B, ch[n], S, S) if n in ch else (B, S, S)) for n in names}
    bnd = {n: np.zeros_like(out[n]) for n in names}
    for o in range(B):
        if np.isnan(affine[o]).any():
            continue                                                       # a refused frame: zeros
        f = src[o]
        x, y = crop_coords(affine[o], S)
        if img is not None:
            for c in range(3):
                plane = (np.asarray(img[f][..., c], np.float32) / np.float32(255)).astype(np.float64)
                out["imgs"][o, c], bnd["imgs"][o, c] = sample_linear(plane, x, y, 5)
        if flow is not None:
            for c in range(2):
                out["flow"][o, c], bnd["flow"][o, c] = sample_linear(flow[f][..., c], x, y)
        if occ is not None:
            out["occ"][o], bnd["occ"][o] = sample_linear(occ[f], x, y)
        (_, inside), _ = sample_nearest(np.ones(_shape_of(img, flow, occ, mask, dp, f)), x, y)    # the all-ones plane
        out["vis2d"][o] = inside
        if mask is not None:
            with np.errstate(invalid="ignore"):
                (m, _), _ = sample_nearest(np.asarray(mask[f]) > 0, x, y)
            out["masks"][o] = (m.astype(np.float64) * inside) > 0
        if dp is not None:
            (d, _), _ = sample_nearest(dp[f], x, y)
            out["dps"][o] = d
    return out, bnd


def _shape_of(*planes_and_f):
    *planes, f = planes_and_f
    for p in planes:
        if p is not None:
            return np.asarray(p[f]).shape[:2]
    raise ValueError("no plane")


# ---- flow_process ---------------------------------------------------------------------------------------------------------------
def _screen_flow(fl, am, ao, S, e_in=None):
    """The cropped flow fl (2,S,S) fp32 of a frame with affine am, re-expressed in the crop of the frame with affine ao:
    fp32(((flow + hp) - t') / a' - p) -> (fs (2,S,S) fp32, e_fs (2,S,S)); e_in (2,S,S): the absolute error of fl as given."""
    col, row = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64))
    fs, e = [], []
    for c, p in ((0, col), (1, row)):
        hp = p * am[c] + am[2 + c]
        raw = ((fl[c].astype(np.float64) + hp) - ao[2 + c]) / ao[c] - p
        fs.append(raw.astype(np.float32))
        M = (np.abs(fl[c]) + np.abs(hp) + abs(ao[2 + c])) / abs(ao[c]) + p
        e.append(8 * V64 * M + 2 * U32 * np.abs(raw) + (0.0 if e_in is None else e_in[c] / abs(ao[c]) * (1 + 2 * U32)))
    return np.stack(fs), np.stack(e)


def flow_process(flow_c, affine, S, e_in=None):
    """flow_c (2 bs,2,S,S) fp32 pair-major, affine (2 bs,4) -> ((flow (2 bs,2,S,S), occ (2 bs,S,S)) float64, (bound_flow, bound_occ),
    exempt (2 bs,S,S) bool = (a) | (b)).  A pair with a refused frame: zeros, bound 0, nothing exempt.  e_in (2 bs,2,S,S): the
    absolute error of flow_c as given (a chain hands on the crop's bound); it enters e_fs divided by |a'|."""
    flow_c = np.asarray(flow_c, np.float32)
    B = flow_c.shape[0]
    bs = B // 2
    flow = np.zeros((B, 2, S, S))
    occ = np.zeros((B, S, S))
    b_flow, b_occ = np.zeros_like(flow), np.zeros_like(occ)
    exempt = np.zeros((B, S, S), bool)
    col, row = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64))
    cf, rf = col.astype(np.float32), row.astype(np.float32)
    for o in range(B):
        q = o + bs if o < bs else o - bs
        am, ao = affine[o], affine[q]
        if np.isnan(am).any() or np.isnan(ao).any():
            continue
        fs, e_fs = _screen_flow(flow_c[o], am, ao, S, None if e_in is None else e_in[o])
        gs, e_gs = _screen_flow(flow_c[q], ao, am, S, None if e_in is None else e_in[q])                      # the partner's, at every pixel: the taps read it
        mx, my = (fs[0] + cf).astype(np.float32), (fs[1] + rf).astype(np.float32)
        x0, y0, w, ok = linear_taps(mx, my)
        imgx, imgy = col + gs[0].astype(np.float64), row + gs[1].astype(np.float64)
        rx, ry, e_tap = np.zeros((S, S)), np.zeros((S, S)), np.zeros((S, S))
        for k in range(4):
            xi, yi = x0 + (k & 1), y0 + (k >> 1)
            vx, inside = _tap(imgx, xi, yi)
            vy, _ = _tap(imgy, xi, yi)
            ex, _ = _tap(np.maximum(e_gs[0], e_gs[1]), xi, yi)
            rx, ry = rx + vx * w[k], ry + vy * w[k]
            e_tap = e_tap + ex * w[k]
        rx, ry, e_tap = np.where(ok, rx, 0.0), np.where(ok, ry, 0.0), np.where(ok, e_tap, 0.0)
        dis = np.sqrt((rx - col) ** 2 + (ry - row) ** 2)
        oc = np.exp(-25 * (dis / S * 2))
        bo = 50 * (np.sqrt(2) * e_tap + 1e-13) / S + 2 * U32 * oc + 1e-14
        risk_a = half_integer_risk(mx, e_fs[0] + U32 * np.abs(mx)) | half_integer_risk(my, e_fs[1] + U32 * np.abs(my))
        risk_b = np.abs(oc - 0.25) <= bo
        occ[o] = np.where(oc < 0.25, 0.0, oc)
        b_occ[o] = bo
        exempt[o] = risk_a | risk_b
        fdiv = (fs / np.float32(S)).astype(np.float32)
        flow[o] = 2.0 * fdiv.astype(np.float64)
        b_flow[o] = 2 * e_fs / S + 2 * U32 * np.abs(flow[o])
    return (flow, occ), (b_flow, b_occ), exempt


# ---- the chain ------------------------------------------------------------------------------------------------------------------
def prepare_frame_pairs(raw, S, crop_factor=1.2):
    """raw: numpy arrays led by (bs, 2) -> (dict, dict of bounds, exempt): the planes of moda_amd.frame_pairs.prepare_frame_pairs
    that the frame-pair kernels produce (imgs, masks, vis2d, dps, flow, occ, kaug, status) and the pair-major ids."""
    bs = raw["mask"].shape[0]
    flat = {k: np.asarray(raw[k]).reshape((2 * bs,) + np.asarray(raw[k]).shape[2:]) for k in ("img", "mask", "flow", "dp")}
    box, _ = mask_bbox(flat["mask"])
    (kaug, aff, status), _ = compute_crop_params(box, S, crop_factor, pair_major=True)
    crop, cb = crop_frames(aff, S, img=flat["img"], flow=flat["flow"], mask=flat["mask"], dp=flat["dp"], pair_major=True)
    # the cropped flow handed on is the oracle's float64 value rounded to fp32; the product's differs from it by the crop's bound
    e_in = cb["flow"] + U32 * np.abs(crop["flow"])
    (flow, occ), (b_flow, b_occ), exempt = flow_process(crop["flow"].astype(np.float32), aff, S, e_in)
    rows = pair_major_rows(2 * bs)
    out = {"imgs": crop["imgs"], "masks": crop["masks"], "vis2d": crop["vis2d"], "dps": crop["dps"], "flow": flow, "occ": occ,
           "kaug": kaug, "affine": aff, "status": status, "rows": rows}
    bounds = {"imgs": cb["imgs"], "flow": b_flow, "occ": b_occ}
    return out, bounds, exempt
