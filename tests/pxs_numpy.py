"""A float64 / integer numpy restatement of the reference's pixel sampling (nnutils/moda.py:1048-1260, banmo.sample_pxs and
obs_to_rays[_line]), of the uncertainty head's ray inputs (:1316-1327) and of the ordering rule of moda_topk_rows.

UNPINNED: the reference's moda.py needs torchvision / pytorch3d at import and cannot run beside these tests, so nothing here is
checked against a reference run.  What pins it instead: tests/test_pxs_oracle.py replays the reference's literal
view(2,-1) / topk / stack / cat / view(-1) sequence in CPU torch and requires the closed-form ray order below to equal it."""
import numpy as np


def split_counts(nsample, nactive):
    """moda.py:1069-1070: (uniform, active) rays per line / frame, the reference's int() roundings."""
    return int(nsample * (1 - nactive)), int(nactive * nsample)


# ---- the ordering rule: descending key (-0 == +0, NaN one key above +inf), then ascending index ------------------------------------
def topk_rows(values, k):
    """-> (idx (rows, k) int64, vals (rows, k), number of NaNs): by a stable sort."""
    v = np.asarray(values, np.float32)
    rows, n = v.shape
    idx = np.empty((rows, k), np.int64)
    for r in range(rows):
        nan = np.isnan(v[r])
        key = np.where(nan, np.inf, v[r].astype(np.float64) + 0.0)          # -0 + 0 = +0; the NaNs are ordered by `nan` below
        order = np.lexsort((np.arange(n), -key, ~nan))                        # last key first: NaNs, then descending value, then index
        idx[r] = order[:k]
    return idx, np.take_along_axis(v, idx, 1), int(np.isnan(v).sum())


# ---- the ray order (closed form) -----------------------------------------------------------------------------------------------------
def line_ray_map(P, nsample, n_u, n_s, topk):
    """Line mode -> (b, slot) per ray: the line b = h P + l the ray comes from and its entry of rand_inds[b] (nsample uniform
    draws, then 4 nsample candidates).  topk (n_s P,) indexes the first half's (P, 4 nsample) candidates."""
    n_a, K = 4 * nsample, n_s * P
    b, slot = [], []
    for h in range(2):
        for l in range(P):
            for j in range(n_u):
                b.append(h * P + l)
                slot.append(j)
        for t in range(K):
            c = int(topk[t])
            b.append(h * P + c // n_a)
            slot.append(nsample + c % n_a)
    return np.asarray(b, np.int64), np.asarray(slot, np.int64)


def frame_ray_map(bs, nsample, n_u, n_s, topk):
    """Frame mode -> (b, slot) per ray (b, s); topk (bs, n_s) indexes each row's 4 nsample candidates."""
    b, slot = [], []
    for f in range(bs):
        for j in range(n_u):
            b.append(f)
            slot.append(j)
        for t in range(n_s):
            b.append(f)
            slot.append(nsample + int(topk[f][t]))
    return np.asarray(b, np.int64), np.asarray(slot, np.int64)


def assemble(rand_inds, nsample, n_u, n_s, line, img_size, lineid, frameid, frameid_sub, dataid, errid, topk, near_far, n_vid):
    """moda_pxs_assemble's outputs and status as a dict (integers int64, floats float32 exact values)."""
    rand_inds = np.asarray(rand_inds, np.int64)
    bs = rand_inds.shape[0]
    near_far = np.asarray(near_far, np.float32)
    if line:
        b, slot = line_ray_map(bs // 2, nsample, n_u, n_s, topk)
    else:
        b, slot = frame_ray_map(bs, nsample, n_u, n_s, topk)
    ind = rand_inds[b, slot]
    limit = img_size if line else img_size ** 2
    ok = (ind >= 0) & (ind < limit)
    xys = np.full((len(b), 2), np.nan, np.float32)
    if line:
        xys[ok, 0] = ind[ok]
        xys[ok, 1] = np.asarray(lineid, np.int64)[b[ok]]
    else:
        xys[ok, 0] = ind[ok] % img_size
        xys[ok, 1] = ind[ok] // img_size
    rows = b if line else np.arange(bs)
    f, d = np.asarray(frameid, np.int64)[rows], np.asarray(dataid, np.int64)[rows]
    f_ok = (f >= 0) & (f < len(near_far))
    nf = np.full((len(rows), 2), np.nan, np.float32)
    nf[f_ok] = near_far[f[f_ok]]
    bad_ids = int((~f_ok).sum()) + (int(((d < 0) | (d >= n_vid)).sum()) if n_vid > 0 else 0)
    return dict(rand_inds=ind, xys=xys, frameid=f, frameid_sub=np.asarray(frameid_sub, np.int64)[rows], dataid=d,
                errid=np.asarray(errid, np.int64)[rows], batch_map=rows.astype(np.int64), near_far=nf, ray_line=b,
                status=np.asarray([0, bad_ids, int((~ok).sum()), 0], np.int64))


def gather_obs(obs, row, col):
    """obs: name -> (B, C, W); ray r reads obs[row[r], :, col[r]] -> name -> (R, C) float32, NaN where row / col is out of range."""
    out = {}
    for name, t in obs.items():
        t = np.asarray(t, np.float32)
        B, C, W = t.shape
        ok = (row >= 0) & (row < B) & (col >= 0) & (col < W)
        o = np.full((len(row), C), np.nan, np.float32)
        o[ok] = t[row[ok], :, col[ok]]
        out[name] = o
    return out


# ---- float64 arithmetic ----------------------------------------------------------------------------------------------------------------
def raycast(xys, Rmat, Tmat, Kinv):
    """geom_utils.py:763-766, one pixel per row: rays_d = (Kinv [x, y, 1])^T R, rays_o = -T^T R (float64)."""
    p = np.concatenate([np.asarray(xys, np.float64), np.ones((len(xys), 1))], 1)
    cam = np.einsum('rij,rj->ri', np.asarray(Kinv, np.float64), p)
    d = np.einsum('ri,rij->rj', cam, np.asarray(Rmat, np.float64))
    o = -np.einsum('ri,rij->rj', np.asarray(Tmat, np.float64), np.asarray(Rmat, np.float64))
    return d, o


def unc_inputs(xys, Kinv, frameid_sub, dataid, vid_code, max_ts):
    """moda.py:1316-1327 per ray -> ts (R, 1), vid_code (R, C), xysn (R, 2) in float64."""
    p = np.concatenate([np.asarray(xys, np.float64), np.ones((len(xys), 1))], 1)
    xysn = np.einsum('rj,rij->ri', p, np.asarray(Kinv, np.float64))[:, :2]
    ts = np.asarray(frameid_sub, np.float64)[:, None] / max_ts * 2 - 1
    return ts, np.asarray(vid_code, np.float64)[np.asarray(dataid, np.int64)], xysn


def raycast_grads(xys, Rmat, Tmat, Kinv, g_d, g_o, g_xysn, ray_line, n_lines):
    """Gradients of sum(g_d * rays_d) + sum(g_o * rays_o) + sum(g_xysn * xysn) onto the per-LINE cameras, the rays' rows summed
    over the line they come from (float64) -> (d_Rmat, d_Tmat, d_Kinv), each (n_lines, ...)."""
    xys, Rmat, Tmat, Kinv = (np.asarray(t, np.float64) for t in (xys, Rmat, Tmat, Kinv))
    g_d, g_o, g_xysn = (np.asarray(t, np.float64) for t in (g_d, g_o, g_xysn))
    p = np.concatenate([xys, np.ones((len(xys), 1))], 1)
    cam = np.einsum('rij,rj->ri', Kinv, p)
    dR = np.einsum('ri,rj->rij', cam, g_d) - np.einsum('ri,rj->rij', Tmat, g_o)
    dT = -np.einsum('rij,rj->ri', Rmat, g_o)
    g_cam = np.einsum('rij,rj->ri', Rmat, g_d)
    g_cam[:, :2] += g_xysn
    dK = np.einsum('ri,rj->rij', g_cam, p)
    out = []
    for t in (dR, dT, dK):
        acc = np.zeros((n_lines,) + t.shape[1:])
        np.add.at(acc, ray_line, t)
        out.append(acc)
    return out
