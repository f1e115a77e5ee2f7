"""Which pixels a training step trains on, device-resident: banmo.sample_pxs (reference nnutils/moda.py:1048-1213) with its
uncertainty-driven active sampling (:1066-1177), the uncertainty head's per-ray inputs (:1316-1327) and the observation gathers
(:1215-1260).  The candidates' top-k, the per-ray assembly and the gathers are one HIP launch each (moda_topk_rows,
moda_pxs_assemble, moda_obs_gather, csrc/pixsample_kernels.hip); nothing is read back, so the stage can be captured.

Deviations from the reference, all deliberate:
  * `frameid` / `errid` come back as device tensors (the reference ends in two `.cpu()` calls; forward_loss takes device ids).
  * The selection follows a stated total order -- descending value with -0 == +0 and NaN above +inf, ties by ascending index --
    where torch.topk leaves ties unspecified.  It is exact on the values it is given; those are computed in the current
    inference precision (set_precision), and fp16 may order near-ties differently from fp32.
  * The uncertainty head is evaluated on the FIRST P lines' candidates only: the reference evaluates all 2P lines and reads row 0.
  * No parity with torch's random stream (`rand_inds=` injects the draws).
  * Bad ids do not raise: a column outside the line / frame, a frame id outside `near_far` or a data id outside `vid_code` gives
    NaN rows and is counted in rays['pxs_status'] (device int32 [#NaN predictions, #ids refused, #columns refused, 0]).
"""
import torch
from torch.autograd import Function

from . import _lib as L
from . import abi
from . import feeders as FD

TOPK_MAX_N = abi.CONSTANTS["MODA_TOPK_MAX_N"]
_SHORT_N = 256              # rows up to this length share a workgroup; longer rows are one grid row each (at most 65535)


def topk_rows(values, k, return_values=False, status=None):
    """values (rows, n) fp32 -> (idx (rows, k) int32, status (4,) int32): the k first of every row in descending order, -0 as +0,
    NaN above +inf, ties by ascending index (moda_topk_rows).  status[0] counts the NaNs seen.  return_values: (idx, values,
    status)."""
    if not torch.is_tensor(values) or values.dim() != 2:
        raise ValueError("topk_rows: expected a (rows, n) tensor")
    v = L.dev(values)
    rows, n = v.shape
    k = int(k)
    if n > TOPK_MAX_N:
        raise ValueError(f"topk_rows: rows of {n} values, the kernel takes at most {TOPK_MAX_N} (MODA_TOPK_MAX_N)")
    if n < 1 or rows * n >= 2 ** 31 or (n > _SHORT_N and rows > 65535):
        raise ValueError(f"topk_rows: shape {(rows, n)} is outside what the kernel takes (MODA_ESHAPE)")
    if k < 1 or k > n:
        raise ValueError(f"topk_rows: k = {k} outside 1..{n}")
    idx = torch.empty((rows, k), device=v.device, dtype=torch.int32)
    vals = torch.empty((rows, k), device=v.device) if return_values else None
    if status is None:
        status = torch.zeros((4,), device=v.device, dtype=torch.int32)
    L.call("moda_topk_rows", L.ptr(v), rows, n, k, L.ptr(idx), L.ptr(vals), L.ptr(status), L.stream())
    return (idx, vals, status) if return_values else (idx, status)


def _obs(t, C, B, what):
    """An observation tensor (B, C, W[, 1]) as the kernel reads it, or an error: fp32, contiguous, on the device."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError("gather_obs: observations must be CUDA (ROCm) tensors; the HIP library is the only compute path")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"gather_obs: {what} must be contiguous fp32, got {t.dtype}, contiguous={t.is_contiguous()}")
    if t.dim() == 4 and t.shape[-1] == 1:
        t = t[..., 0]
    if t.dim() != 3 or t.shape[0] != B or t.shape[1] != C:
        raise ValueError(f"gather_obs: {what} must be ({B}, {C}, W[, 1]), got {tuple(t.shape)}")
    return t


def gather_obs(rays, rand_inds, batch_map, imgs, masks, vis2d, flow, occ, dp_feats=None, status=None):
    """obs_to_rays_line (batch_map (R,) given, rand_inds (R, 1)) / obs_to_rays (batch_map None, rand_inds (bs, ns)) of
    moda.py:1215-1260 in one launch: rays['img_at_samp'] ... ['feats_at_samp'] in the reference's shapes, (R, 1, C) / (bs, ns, C),
    without forming t[batch_map].  A column or a row out of range gives NaN values, counted in rays['obs_status'] (`status`, or a
    fresh (4,) int32: [0, #rows refused, #columns refused, 0])."""
    B = imgs.shape[0]
    obs = [_obs(imgs, 3, B, "imgs"), _obs(masks, 1, B, "masks"), _obs(vis2d, 1, B, "vis2d"), _obs(flow, 2, B, "flow"),
           _obs(occ, 1, B, "occ"), None if dp_feats is None else _obs(dp_feats, 16, B, "dp_feats")]
    W = obs[0].shape[2]
    if any(t is not None and t.shape[2] != W for t in obs):
        raise ValueError("gather_obs: the observations differ in their pixel count")
    cols = L.dev(rand_inds, torch.int64)
    if cols.dim() != 2:
        raise ValueError(f"gather_obs: rand_inds must be (R, 1) or (bs, ns), got {tuple(cols.shape)}")
    lead, ns = cols.shape
    bm = None
    if batch_map is not None:
        bm = L.dev(batch_map, torch.int64).reshape(-1)
        if ns != 1 or bm.shape[0] != lead:
            raise ValueError(f"gather_obs: with a batch_map, rand_inds is (R, 1) and batch_map (R,); got {tuple(cols.shape)}, {tuple(bm.shape)}")
    elif lead != B:
        raise ValueError(f"gather_obs: rand_inds has {lead} rows for {B} frames")
    R = lead * ns
    dev = cols.device
    out = [torch.empty((lead, ns, C), device=dev) for C in (3, 1, 1, 2, 1)]
    feats = torch.empty((lead, ns, 16), device=dev) if dp_feats is not None else None
    if status is None:
        status = torch.zeros((4,), device=dev, dtype=torch.int32)
    L.call("moda_obs_gather", *(L.ptr(t) for t in obs), B, W, L.ptr(bm), L.ptr(cols), R, ns, *(L.ptr(t) for t in out), L.ptr(feats),
           L.ptr(status), L.stream())
    for key, t in zip(('img_at_samp', 'sil_at_samp', 'vis_at_samp', 'flo_at_samp', 'cfd_at_samp'), out):
        rays[key] = t
    if feats is not None:
        rays['feats_at_samp'] = feats
    rays['obs_status'] = status
    return rays


class GatherRowsFn(Function):
    """table (T, C)[ids] whose backward is the deterministic row sum moda_id_rows_sum (8 columns a launch): repeated ids add in
    increasing ray order, the same bits on every run.  An id outside [0, T) is not followed: a NaN row, no gradient."""

    @staticmethod
    def forward(ctx, table, ids):
        T = table.shape[0]
        ok = (ids >= 0) & (ids < T)
        rows = table.index_select(0, ids.clamp(0, T - 1))
        ctx.save_for_backward(ids)
        ctx.T = T
        return torch.where(ok[:, None], rows, torch.full_like(rows, float('nan')))

    @staticmethod
    def backward(ctx, g):
        (ids,) = ctx.saved_tensors
        g = L.dev(g)
        parts = [FD.id_rows_sum(g[:, c:c + 8], ids, ctx.T) for c in range(0, g.shape[1], 8)]
        return (parts[0] if len(parts) == 1 else torch.cat(parts, 1)), None


def gather_rows(table, ids):
    """table (T, ...) -> (len(ids), ...) through GatherRowsFn."""
    t = L.dev(table)
    flat = GatherRowsFn.apply(t.reshape(t.shape[0], -1), L.dev(ids, torch.int64).reshape(-1))
    return flat.view((flat.shape[0],) + tuple(t.shape[1:]))


def _eye_rows(n, device):
    return (L.const_tensor(("pxs_eye", n), device, lambda: torch.eye(3).repeat(n, 1, 1)),
            L.const_tensor(("pxs_zero3", n), device, lambda: torch.zeros(n, 3)))


def _unc_inputs(model, dataid, frameid_sub, xys, Kinv):
    """moda.py:1316-1327 for (bs, ns) pixels: ts (bs, ns, 1), vid_code (bs, ns, C), xysn (bs, ns, 2).  xysn = (Kinv [x, y, 1])[:2]
    is moda_raycast with the identity for a rotation, so its gradient reaches Kinv through that kernel's backward; the code rows
    come through GatherRowsFn, so vid_code.weight's gradient is a fixed-order sum."""
    xys = L.dev(xys)
    bs, ns, _ = xys.shape
    dev = xys.device
    ts = frameid_sub.to(dev).float() / float(model.max_ts) * 2 - 1                                # :1317
    ts = ts.reshape(bs, 1, 1).expand(bs, ns, 1)
    code = gather_rows(model.vid_code.weight, dataid.to(dev).long())                              # :1321-1322
    eye, zero = _eye_rows(bs, dev)
    xysn = FD.RaycastFn.apply(xys, eye, zero, L.dev(Kinv).reshape(bs, 3, 3))[0][..., :2]          # :1325-1326
    return ts, code[:, None].expand(bs, ns, code.shape[-1]), xysn


def unc_ray_inputs(model, rays, dataid, frameid_sub, xys, Kinv):
    """The uncertainty head's inputs of moda.update_rays (moda.py:1316-1327): rays['ts'], ['vid_code'], ['xysn'] for the rays'
    (bs, nsample) pixels.  Gradients reach model.vid_code.weight and Kinv."""
    rays['ts'], rays['vid_code'], rays['xysn'] = _unc_inputs(model, dataid, frameid_sub, xys, Kinv)
    return rays


def _predict_unc(model, dataid, frameid_sub, xys_a, Kinv):
    """nerf_unc on candidate pixels xys_a (rows, n, 2) under no_grad (moda.py:1102-1116) -> (rows, n)."""
    with torch.no_grad():
        ts, code, xysn = _unc_inputs(model, dataid, frameid_sub, xys_a, Kinv.detach())
        rows, n, _ = xysn.shape
        xyt = torch.cat([xysn, ts], -1).reshape(rows * n, 3)
        x = torch.cat([model.embedding_xyz(xyt), code.reshape(rows * n, -1)], -1)
        return model.nerf_models['nerf_unc'](x)[..., 0].reshape(rows, n)


def _ids_common(*ids):
    """The five id arrays as the kernel reads them: contiguous device tensors of ONE integer type -> (tensors, is-int64)."""
    out = []
    for t in ids:
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("sample_pxs: ids must be CUDA (ROCm) tensors; the HIP library is the only compute path")
        if t.dtype not in (torch.int32, torch.int64):
            t = t.long()
        out.append(t.reshape(-1).contiguous())
    if len({t.dtype for t in out}) > 1:
        out = [t.long() for t in out]
    return out, int(out[0].dtype == torch.int64)


ASSEMBLED = ('rand_inds', 'xys', 'frameid', 'frameid_sub', 'dataid', 'errid', 'batch_map', 'near_far')


def assemble_rays(rand_inds, nsample, n_u, n_s, line, img_size, lineid, frameid, frameid_sub, dataid, errid, topk, near_far, n_vid=0,
                  status=None):
    """moda_pxs_assemble: the split / select / stack / cat / view(-1) of moda.py:1075-1191 in one launch -> dict of ASSEMBLED (flat:
    rand_inds (R,), xys (R, 2); the ids, batch_map and near_far rows per ray in line mode, per frame in frame mode) + 'status'.
    n_s == 0: active sampling off, topk unused."""
    rand_inds = L.dev(rand_inds, torch.int64)
    bs = rand_inds.shape[0]
    dev = rand_inds.device
    ids, i64 = _ids_common(frameid, frameid_sub, dataid, errid, lineid if line else frameid)
    fid, fsub, did, eid, lid = ids
    near_far = L.dev(near_far).reshape(-1, 2)
    if n_s:
        topk = L.dev(topk, torch.int32).reshape(-1)
        if topk.shape[0] != (n_s * (bs // 2) if line else n_s * bs):
            raise ValueError(f"assemble_rays: {topk.shape[0]} top-k entries for n_s = {n_s}, bs = {bs}")
    R = bs * (n_u + n_s)
    n_id = R if line else bs
    i8 = lambda n: torch.empty((n,), device=dev, dtype=torch.int64)
    out = dict(rand_inds=i8(R), xys=torch.empty((R, 2), device=dev), frameid=i8(n_id), frameid_sub=i8(n_id), dataid=i8(n_id),
               errid=i8(n_id), batch_map=i8(n_id), near_far=torch.empty((n_id, 2), device=dev))
    if status is None:
        status = torch.zeros((4,), device=dev, dtype=torch.int32)
    L.call("moda_pxs_assemble", L.ptr(rand_inds), bs, nsample, n_u, n_s, int(bool(line)), int(img_size), L.ptr(lid), L.ptr(fid),
           L.ptr(fsub), L.ptr(did), L.ptr(eid), i64, L.ptr(topk if n_s else None), L.ptr(near_far), near_far.shape[0], int(n_vid),
           *(L.ptr(out[k]) for k in ASSEMBLED), L.ptr(status), L.stream())
    out['status'] = status
    return out


def split_counts(nsample, nactive):
    """(n_u, n_s) of moda.py:1069-1070: uniform and active rays per line / frame, with the reference's int() roundings."""
    return int(nsample * (1 - nactive)), int(nactive * nsample)


def sample_pxs(model, bs, nsample, Rmat, Tmat, Kinv, dataid, frameid, frameid_sub, embedid, lineid, errid, imgs, masks, vis2d,
               flow, occ, dp_feats, *, rand_inds=None, generator=None, return_unc=False):
    """banmo.sample_pxs (moda.py:1048-1213) -> (rand_inds, rays, frameid, errid), the ids as DEVICE int64 tensors.

    Read off `model`: opts.lineload / use_unc / nactive / warmup_steps / use_embed, training, progress, img_size, max_ts, vid_code,
    embedding_xyz, nerf_models, near_far, and what update_rays / update_delta_rts read (pose_code, nerf_body_rts, ...).
    rand_inds (bs, 5 nsample) int64 injects the draws (columns of the line, or pixel indices of the frame; nsample uniform, then
    4 nsample candidates); otherwise they are drawn with sample_xy (`generator` is torch's, there is no parity with the reference's
    stream).  `embedid` is accepted and unused, as in the reference (:1195-1196 passes frameid).  return_unc: rays['unc_candidates']
    holds the predictions the selection was made from.  rays['pxs_status']: device int32 [#NaN predictions, #ids refused, #columns
    refused, 0]."""
    opts = model.opts
    for flag in ("flowbw", "lbs"):
        if getattr(opts, flag, False):
            raise NotImplementedError(f"sample_pxs: opts.{flag} is not implemented (update_rays runs the neudbs configuration)")
    dp = dp_feats if getattr(opts, "use_embed", True) else None
    if not model.training:
        return _sample_all(model, bs, nsample, Rmat, Tmat, Kinv, dataid, frameid, frameid_sub, errid, imgs, masks, vis2d, flow, occ, dp)
    line = bool(opts.lineload)
    active = bool(opts.use_unc) and model.progress >= opts.warmup_steps
    n_u, n_s = split_counts(nsample, opts.nactive) if active else (nsample, 0)
    if line and bs % 2:
        raise ValueError(f"sample_pxs: line loading pairs the lines h * P + l, bs = {bs} is odd")
    if n_u + n_s == 0:
        raise ValueError(f"sample_pxs: nsample = {nsample} with nactive = {opts.nactive} leaves no ray (n_u + n_s == 0)")
    P = bs // 2
    n_a = 4 * nsample
    n_top = (P if line else 1) * n_a
    if n_s and n_top > TOPK_MAX_N:
        raise ValueError(f"sample_pxs: {n_top} candidates a row, the top-k kernel takes at most {TOPK_MAX_N} (MODA_TOPK_MAX_N)")
    for t, what in ((imgs, "imgs"), (masks, "masks"), (vis2d, "vis2d"), (flow, "flow"), (occ, "occ"), (dp, "dp_feats")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError(f"sample_pxs: {what} must be contiguous fp32")
    dev = imgs.device
    img_size = int(model.img_size)
    if line and lineid is None:
        raise ValueError("sample_pxs: line loading needs lineid")
    # 1. the draws (:1062-1064)
    if rand_inds is None:
        ones = torch.ones(img_size if line else img_size ** 2, device=dev)
        rand_inds = torch.multinomial(ones, bs * (nsample + n_a), replacement=line, generator=generator).view(bs, nsample + n_a)
    rand_inds = L.dev(rand_inds, torch.int64)
    if tuple(rand_inds.shape) != (bs, nsample + n_a):
        raise ValueError(f"sample_pxs: rand_inds must be ({bs}, {nsample + n_a}), got {tuple(rand_inds.shape)}")
    ids, i64 = _ids_common(frameid, frameid_sub, dataid, errid, lineid if line else frameid)
    fid, fsub, did, eid, lid = ids
    if any(t.shape[0] != bs for t in ids):
        raise ValueError(f"sample_pxs: the id arrays must hold {bs} entries")
    near_far = L.dev(model.near_far).reshape(-1, 2)
    n_vid = model.vid_code.weight.shape[0] if getattr(opts, "use_unc", False) else 0
    status = torch.zeros((4,), device=dev, dtype=torch.int32)
    rays_extra = {}
    topk = None
    if n_s:
        # 2. the uncertainty head on the candidates, the first P lines only in line mode (:1102-1116, 1149)
        rows = P if line else bs
        cand = rand_inds[:rows, nsample:]
        if line:
            xys_a = torch.stack([cand.float(), lid[:rows, None].float().expand(rows, n_a)], -1)
        else:
            yy = torch.div(cand, img_size, rounding_mode='floor')
            xys_a = torch.stack([(cand - yy * img_size).float(), yy.float()], -1)
        unc = _predict_unc(model, did[:rows], fsub[:rows], xys_a, L.dev(Kinv).reshape(bs, 3, 3)[:rows])
        if return_unc:
            rays_extra['unc_candidates'] = unc
        # 3. the selection (:1146 / :1171)
        topk, _ = topk_rows(unc.reshape(1, -1) if line else unc, n_s * P if line else n_s, status=status)
    # 4. the per-ray assembly (:1075-1191)
    per = n_u + n_s
    R = bs * per
    asm = assemble_rays(rand_inds, nsample, n_u, n_s, line, img_size, lid, fid, fsub, did, eid, topk, near_far, n_vid, status=status)
    rand_out, xys_o, fid_o, fsub_o, did_o, eid_o, bm_o, nf_o = (asm[k] for k in ASSEMBLED)
    if line:
        # 5. the cameras of every ray's line: one gather of the 21-float row, its backward a fixed-order sum over repeated lines
        rtk = torch.cat([L.dev(Rmat).reshape(bs, 9), L.dev(Tmat).reshape(bs, 3), L.dev(Kinv).reshape(bs, 9)], 1)
        rtk = GatherRowsFn.apply(rtk, bm_o)
        Rm, Tm, Ki = rtk[:, :9].reshape(R, 3, 3), rtk[:, 9:12], rtk[:, 12:].reshape(R, 3, 3)
        xys, rand_ret = xys_o.view(R, 1, 2), rand_out.view(R, 1)
        pair_bs = 2 if n_s else bs
    else:
        Rm, Tm, Ki = Rmat, Tmat, Kinv
        xys, rand_ret = xys_o.view(bs, per, 2), rand_out.view(bs, per)
        pair_bs = bs
    # 6.-9. rays, the per-frame codes and poses, the uncertainty head's inputs, the rest-pose correction (:1193-1200)
    rays = FD.raycast(xys, Rm, Tm, Ki, nf_o)
    rays.update(rays_extra)
    rays['pxs_status'] = status
    FD.update_rays(model, rays, pair_bs > 1, fid_o.clamp(0, near_far.shape[0] - 1))     # a refused id is not followed: its rays are NaN
    if getattr(opts, "use_unc", False):
        unc_ray_inputs(model, rays, did_o, fsub_o, xys, Ki)
    if 'bones' in model.nerf_models:
        FD.update_delta_rts(model, rays)
    # 10. the observations (:1205-1211)
    gather_obs(rays, rand_ret, bm_o if line else None, imgs, masks, vis2d, flow, occ, dp)     # (columns were counted by the assembly)
    return rand_ret, rays, fid_o, eid_o


def _sample_all(model, bs, nsample, Rmat, Tmat, Kinv, dataid, frameid, frameid_sub, errid, imgs, masks, vis2d, flow, occ, dp):
    """training == False: every pixel of every frame (sample_xy(return_all=True), moda.py:1063-1064), no split, through the
    existing pieces."""
    from . import pixel_lines as PL
    dev = imgs.device
    rand_inds, xys = FD.sample_xy(int(model.img_size), bs, nsample + 4 * nsample, dev, return_all=True)
    fid = frameid.to(dev).long()
    near_far = L.dev(model.near_far).reshape(-1, 2)
    rays = FD.raycast(xys, Rmat, Tmat, Kinv, near_far[fid])
    FD.update_rays(model, rays, bs > 1, fid)
    if getattr(model.opts, "use_unc", False):
        unc_ray_inputs(model, rays, dataid, frameid_sub, xys, Kinv)
    if 'bones' in model.nerf_models:
        FD.update_delta_rts(model, rays)
    PL.obs_to_rays(rays, rand_inds, imgs, masks, vis2d, flow, occ, dp)
    return rand_inds, rays, fid, errid
