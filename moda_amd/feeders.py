"""The per-frame feeders immediately before the rendering path, with the reference's names and
argument meaning: ray construction (`raycast`, `sample_xy`, `chunk_rays`, nnutils/geom_utils.py:746-838), the frame codes
(`FrameCode`, nnutils/nerf.py:346-380), the body-pose head (`DQ_RTHead`, nerf.py:239-279), the rest-pose correction
(`correct_bones`, `correct_rest_pose`, geom_utils.py:933-972, composed by `update_delta_rts`, moda.py:1262-1279) and the
per-ray expansion `update_rays` performs (nnutils/moda.py:1281-1327).  Arithmetic runs in HIP kernels behind autograd Functions; gradients reach the camera
(`Rmat`, `Tmat`, `Kinv`), the code tables and the pose head's parameters as they do in the reference."""
import numpy as np
import torch
from torch import nn
from torch.autograd import Function

from . import _lib as L
from . import abi
from . import autograd as A
from .dual_quat import dq_inverse, dq_mul
from .geom_utils import bone_transform
from .nerf import Embedding, NeRF


class RaycastFn(Function):
    """geom_utils.py:763-766: rays_d = (Kinv [x,y,1])^T R, rays_o = -T^T R."""

    @staticmethod
    def forward(ctx, xys, Rmat, Tmat, Kinv):
        xy, R, T, K = (L.dev(t) for t in (xys, Rmat, Tmat, Kinv))
        bs, ns, _ = xy.shape
        d = torch.empty((bs, ns, 3), device=xy.device)
        o = torch.empty((bs, ns, 3), device=xy.device)
        L.call("moda_raycast", L.ptr(xy), L.ptr(R), L.ptr(T), L.ptr(K), bs, ns, L.ptr(d), L.ptr(o), None, None, None, None,
               None, L.stream())
        ctx.save_for_backward(xy, R, T, K)
        return d, o

    @staticmethod
    def backward(ctx, g_d, g_o):
        xy, R, T, K = ctx.saved_tensors
        bs, ns, _ = xy.shape
        gd = torch.zeros((bs, ns, 3), device=xy.device) if g_d is None else L.dev(g_d)
        go = None if g_o is None else L.dev(g_o)
        dR, dT, dK = torch.empty_like(R), torch.empty_like(T), torch.empty_like(K)
        L.call("moda_raycast", L.ptr(xy), L.ptr(R), L.ptr(T), L.ptr(K), bs, ns, None, None, L.ptr(gd), L.ptr(go), L.ptr(dR),
               L.ptr(dT), L.ptr(dK), L.stream())
        return None, dR, dT, dK


def raycast(xys, Rmat, Tmat, Kinv, near_far):
    """geom_utils.py:746-794 -> rays dict (rays_o, rays_d, near, far, rtk_vec, xys, nsample, bs), tensors (bs, ns, .)."""
    xys = L.dev(xys)
    bs, nsample, _ = xys.shape
    Rmat = L.dev(Rmat).reshape(-1, 3, 3)
    Tmat = L.dev(Tmat).reshape(-1, 3)
    Kinv = L.dev(Kinv).reshape(-1, 3, 3)
    rays_d, rays_o = RaycastFn.apply(xys, Rmat, Tmat, Kinv)
    if near_far is not None:
        nf = L.dev(near_far)
        znear = nf[:, 0, None, None].expand(bs, nsample, 1).contiguous()           # :769-770
        zfar = nf[:, 1, None, None].expand(bs, nsample, 1).contiguous()
    else:                                                                         # :772-776
        z = Tmat[:, None, 2:3].expand(bs, nsample, 1)
        znear = (z - 1.5).clamp_min(1e-5)
        zfar = z + 1.5
    rtk_vec = torch.cat([Rmat.reshape(-1, 1, 9), Tmat.reshape(-1, 1, 3), Kinv.reshape(-1, 1, 9)], -1)   # :780-784
    return {'rays_o': rays_o, 'rays_d': rays_d, 'near': znear, 'far': zfar,
            'rtk_vec': rtk_vec.expand(bs, nsample, 21).contiguous(), 'xys': xys, 'nsample': nsample, 'bs': bs}


def sample_xy(img_size, bs, nsample, device, return_all=False, lineid=None):
    """geom_utils.py:796-827: pixel indices and coordinates (index logic and torch's own sampler; no arithmetic)."""
    ar = torch.arange(img_size, device=device, dtype=torch.float32)
    xygrid = torch.stack([ar[None, :].expand(img_size, img_size), ar[:, None].expand(img_size, img_size)], -1).reshape(1, -1, 2)
    if return_all:
        xys = xygrid.repeat(bs, 1, 1)
        rand_inds = torch.arange(xys.shape[1], dtype=torch.float32)[None].repeat(bs, 1)
    elif lineid is None:
        rand_inds = torch.multinomial(torch.ones(img_size ** 2, device=device), bs * nsample, replacement=False).view(bs, nsample)
        xys = xygrid[0][rand_inds]
    else:
        rand_inds = torch.multinomial(torch.ones(img_size, device=device), bs * nsample, replacement=True).view(bs, nsample)
        xys = xygrid[0][rand_inds].clone()
        xys[..., 1] = xys[..., 1] + lineid[:, None]
    return rand_inds.long(), xys


def chunk_rays(rays, start, delta):
    """geom_utils.py:829-838: rays [start, start+delta) of the flattened (bs*nsample, C) tensors.  In the frame-grouped
    layout (`rays_per_frame` set by update_rays(frame_layout=True)) the rendering.FRAME_KEYS tensors hold one row per
    frame; the chunk must then cover whole frames and keeps the layout."""
    k = rays.get('rays_per_frame', None)
    if k is None:
        return {key: v.view(-1, v.shape[-1])[start:start + delta] for key, v in rays.items() if torch.is_tensor(v)}
    if start % k or delta % k:
        raise ValueError(f"frame-grouped rays: chunks must cover whole frames of {k} rays")
    from .rendering import FRAME_KEYS
    n_rays = rays['rays_d'].reshape(-1, 3).shape[0]
    out = {'rays_per_frame': k}
    for key, v in rays.items():
        if not torch.is_tensor(v):
            continue
        v2 = v.reshape(-1, v.shape[-1])
        if key in FRAME_KEYS and v2.shape[0] * k == n_rays:
            out[key] = v2[start // k:(start + delta) // k]
        else:
            out[key] = v2[start:start + delta]
    return out


def fid_reindex(fid, num_vids, vid_offset):
    """geom_utils.py:1759-1778: absolute frame id -> (video id, relative time in [-1, 1])."""
    vid_offset = np.asarray(vid_offset)
    tid = torch.zeros_like(fid).float()
    vid = torch.zeros_like(fid)
    max_ts = float((vid_offset[1:] - vid_offset[:-1]).max())
    for i in range(num_vids):
        assign = torch.logical_and(fid >= int(vid_offset[i]), fid < int(vid_offset[i + 1]))
        vid[assign] = i
        doffset = float(vid_offset[i + 1] - vid_offset[i])
        tid[assign] = (fid[assign].float() - float(vid_offset[i]) - doffset / 2) / max_ts * 2
    return vid, tid


class FrameCode(nn.Module):
    """nerf.py:346-380: frame index -> code = Linear(one-hot(video) (x) Fourier(t))."""

    def __init__(self, num_freq, embedding_dim, vid_offset, scale=1):
        super().__init__()
        self.vid_offset = np.asarray(vid_offset)
        self.num_vids = len(vid_offset) - 1
        max_ts = (self.vid_offset[1:] - self.vid_offset[:-1]).max()
        self.num_freq = 2 * int(np.log2(max_ts)) - 2
        self.fourier_embed = Embedding(1, num_freq, alpha=num_freq)
        self.basis_mlp = nn.Linear(self.num_vids * self.fourier_embed.out_channels, embedding_dim)
        self.scale = scale

    def forward(self, fid):
        bs = fid.shape[0]
        vid, tid = fid_reindex(fid, self.num_vids, self.vid_offset)
        coeff = self.fourier_embed(L.dev(tid * self.scale).view(bs, 1))                      # (bs, C), HIP
        C = coeff.shape[1]
        # coeff[..., None] * one_hot(vid): each row's C coefficients land in its video's column of a (C, num_vids) grid
        wide = torch.zeros((bs, C, self.num_vids), device=coeff.device)
        wide.scatter_(2, L.dev(vid, torch.int64).view(bs, 1, 1).expand(bs, C, 1), coeff[..., None])
        return A.LinearFn.apply(wide.view(bs, -1), self.basis_mlp.weight, self.basis_mlp.bias, 0)


class RtToDqFn(Function):
    @staticmethod
    def forward(ctx, rts):
        r = L.dev(rts)
        out = torch.empty((r.shape[0], 8), device=r.device)
        L.call("moda_rt_to_dq", L.ptr(r), r.shape[0], L.ptr(out), None, None, L.stream())
        ctx.save_for_backward(r)
        return out

    @staticmethod
    def backward(ctx, g):
        (r,) = ctx.saved_tensors
        d = torch.empty_like(r)
        L.call("moda_rt_to_dq", L.ptr(r), r.shape[0], None, L.ptr(L.dev(g)), L.ptr(d), L.stream())
        return d


class DQ_RTHead(NeRF):
    """nerf.py:239-279: code (bs, C) -> unit dual quaternions of the B bones, (bs, 1, 8B)."""

    def __init__(self, use_quat, **kwargs):
        super().__init__(**kwargs)
        if not use_quat:
            raise NotImplementedError("DQ_RTHead is built with use_quat=True (moda.py:314-319)")
        self.use_quat = use_quat
        self.num_output = 7
        for m in self.modules():
            if isinstance(m, nn.Linear) and m.bias is not None:
                m.bias.data.zero_()

    def forward(self, x):
        y = super().forward(x)
        bs = y.shape[0]
        return RtToDqFn.apply(y.reshape(-1, self.num_output)).view(bs, 1, -1)


# ---- root (camera) poses: RTHead, RTExplicit, RTExpMLP (nerf.py:307-344, 382-470) on moda_root_pose ----------------------------------
RAW_NONE, RAW_BASE, RAW_ROWS, RAW_BY_ID = (abi.CONSTANTS["MODA_ROOT_RAW_" + k] for k in ("NONE", "BASE", "ROWS", "BY_ID"))


def _ids(t):
    """Frame / data ids as the kernels read them: a contiguous device int32 or int64 tensor, and the is-int64 flag."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError("root poses: ids must be a CUDA (ROCm) tensor; the HIP library is the only compute path")
    if t.dtype not in (torch.int32, torch.int64):
        t = t.long()
    return t.reshape(-1).contiguous(), int(t.dtype == torch.int64)


def id_rows_sum(rows, ids, T, lanes=0):
    """The backward of `table[ids]`: (T, C) = sum of rows[i] over ids[i] == t in increasing i (moda_id_rows_sum): no atomics, the
    same bits on every run and for every `lanes` (lanes per workgroup, 0 = the default)."""
    r = L.dev(rows)
    ids, i64 = _ids(ids)
    if r.dim() != 2 or not 1 <= r.shape[1] <= 8 or ids.shape[0] != r.shape[0]:
        raise ValueError(f"id_rows_sum: expected rows (n, C <= 8) and n ids, got {tuple(r.shape)} and {ids.shape[0]} ids")
    out = torch.empty((T, r.shape[1]), device=r.device)
    L.call("moda_id_rows_sum", L.ptr(r), L.ptr(ids), i64, r.shape[0], T, r.shape[1], L.ptr(out), lanes, L.stream())
    return out


class RootPoseFn(Function):
    """moda_root_pose: base rows se3[ids] (or None), the MLP's rows `delta` (or None), refine_rt against `rt_raw` and the K row
    ks[dataid] -> (rtk (n, out_rows, 4), status (4,) int32 = [#frame ids refused, #data ids refused, 0, 0]).  One launch forward;
    backward one launch plus one deterministic row sum per table (se3, ks)."""

    @staticmethod
    def forward(ctx, se3, ids, delta, rt_raw, raw_mode, obj_scale, ks, dataid, out_rows):
        se3 = None if se3 is None else L.dev(se3)
        delta = None if delta is None else L.dev(delta)
        rt_raw = None if rt_raw is None else L.dev(rt_raw)
        ks = None if ks is None else L.dev(ks).reshape(-1, 4)
        ids, i64 = (None, 0) if ids is None else _ids(ids)
        dataid, d64 = (None, 0) if dataid is None else _ids(dataid)
        for t, what in ((se3, "se3"), (delta, "delta")):
            if t is not None and (t.dim() != 2 or t.shape[1] not in (6, 7)):
                raise ValueError(f"root poses: {what} must be (rows, 6 | 7), got {tuple(t.shape)}")
        if rt_raw is not None and (rt_raw.dim() != 3 or rt_raw.shape[1] not in (3, 4) or rt_raw.shape[2] != 4):
            raise ValueError(f"root poses: rt_raw must be (rows, 3 | 4, 4), got {tuple(rt_raw.shape)}")
        if (raw_mode in (RAW_ROWS, RAW_BY_ID)) != (rt_raw is not None):
            raise ValueError("root poses: rt_raw goes with RAW_ROWS / RAW_BY_ID and with nothing else")
        if delta is None and ids is None:
            raise ValueError("root poses: neither ids nor delta rows")
        n = delta.shape[0] if delta is not None else ids.shape[0]
        for t, what in ((ids, "ids"), (dataid, "dataid")):
            if t is not None and t.shape[0] != n:
                raise ValueError(f"root poses: {what} has {t.shape[0]} rows, expected {n}")
        if raw_mode == RAW_ROWS and rt_raw.shape[0] != n:
            raise ValueError(f"root poses: rt_raw has {rt_raw.shape[0]} rows, expected {n}")
        if raw_mode == RAW_BY_ID and se3 is not None and rt_raw.shape[0] != se3.shape[0]:
            raise ValueError(f"root poses: the rt_raw table has {rt_raw.shape[0]} frames, se3 {se3.shape[0]}")
        dev = (delta if delta is not None else ids).device
        T = se3.shape[0] if se3 is not None else (rt_raw.shape[0] if raw_mode == RAW_BY_ID else 0)
        rtk = torch.empty((n, out_rows, 4), device=dev)
        status = torch.zeros((4,), device=dev, dtype=torch.int32)
        ctx.args = (T, 0 if se3 is None else se3.shape[1], i64, n, 0 if delta is None else delta.shape[1], raw_mode,
                    0 if rt_raw is None else rt_raw.shape[1], float(obj_scale), d64, 0 if ks is None else ks.shape[0], out_rows)
        ctx.save_for_backward(se3, ids, delta, rt_raw, ks, dataid, status)
        RootPoseFn._call(ctx.args, se3, ids, delta, rt_raw, ks, dataid, rtk, None, None, None, None, status)
        ctx.mark_non_differentiable(status)
        return rtk, status

    @staticmethod
    def _call(args, se3, ids, delta, rt_raw, ks, dataid, rtk, g, d_rows, d_delta, d_ks, status):
        T, cols, i64, n, dcols, raw_mode, raw_rows, obj_scale, d64, n_ks, out_rows = args
        L.call("moda_root_pose", L.ptr(se3), T, cols, L.ptr(ids), i64, n, L.ptr(delta), dcols, L.ptr(rt_raw), raw_mode, raw_rows,
               obj_scale, L.ptr(ks), L.ptr(dataid), d64, n_ks, out_rows, L.ptr(rtk), L.ptr(g), L.ptr(d_rows), L.ptr(d_delta),
               L.ptr(d_ks), L.ptr(status), L.stream())

    @staticmethod
    def backward(ctx, g, _g_status):
        se3, ids, delta, rt_raw, ks, dataid, status = ctx.saved_tensors
        n, dev = ctx.args[3], g.device
        need_ks = ks is not None and ctx.needs_input_grad[6]
        d_rows = None if se3 is None else torch.empty((n, se3.shape[1]), device=dev)
        d_delta = None if delta is None else torch.empty_like(delta)
        d_ks_rows = torch.empty((n, 4), device=dev) if need_ks else None
        RootPoseFn._call(ctx.args, se3, ids, delta, rt_raw, ks, dataid, None, L.dev(g), d_rows, d_delta, d_ks_rows, status)
        d_se3 = id_rows_sum(d_rows, ids, se3.shape[0]) if se3 is not None and ctx.needs_input_grad[0] else None
        d_ks = id_rows_sum(d_ks_rows, dataid, ks.shape[0]) if need_ks else None
        return d_se3, None, d_delta if ctx.needs_input_grad[2] else None, None, None, None, d_ks, None, None


def _rts12(rtk, bs):
    """(n, 3, 4) -> the reference modules' (bs, 1, 12) = [R (9) | t (3)] (data movement only)."""
    return torch.cat([rtk[:, :, :3].reshape(-1, 9), rtk[:, :, 3]], -1).view(bs, 1, 12)


class RTHead(NeRF):
    """nerf.py:307-344: code (bs, C) -> rigid transforms (bs, 1, 12) = [R | t]; a quaternion (use_quat) or a rotation vector."""

    def __init__(self, use_quat, **kwargs):
        super().__init__(**kwargs)
        self.use_quat = use_quat
        self.num_output = 7 if use_quat else 6
        for m in self.modules():
            if isinstance(m, nn.Linear) and m.bias is not None:
                m.bias.data.zero_()
        self.id_status = None

    def raw(self, x):
        """The MLP's own output rows (n, num_output), before the tail."""
        return NeRF.forward(self, x).reshape(-1, self.num_output)

    def forward(self, x):
        rts = self.raw(x)
        rtk, self.id_status = RootPoseFn.apply(None, None, rts, None, RAW_NONE, 1.0, None, None, 3)
        return _rts12(rtk, x.shape[0])


class RTExplicit(nn.Module):
    """nerf.py:382-427: frame ids -> rigid transforms (bs, 1, 12) read from the table `se3` (max_t, 7 | 6 with delta)."""

    def __init__(self, max_t, delta=False, rand=True):
        super().__init__()
        self.max_t = max_t
        self.delta = delta
        trans = torch.zeros(max_t, 3)
        if delta:
            rot = torch.zeros(max_t, 3)
        elif rand:
            rot = torch.rand(max_t, 4) * 2 - 1
        else:
            rot = torch.zeros(max_t, 4)
            rot[:, 0] = 1
        se3 = torch.cat([trans, rot], -1)
        self.se3 = nn.Parameter(se3)
        self.num_output = se3.shape[-1]
        self.id_status = None

    def forward(self, x):
        rtk, self.id_status = RootPoseFn.apply(self.se3, x, None, None, RAW_NONE, 1.0, None, None, 3)
        return _rts12(rtk, x.shape[0])


class FrameCodeTable(FrameCode):
    """FrameCode whose Fourier coefficients -- a function of the frame id and the video layout alone -- are tabulated once per
    device for the frames 0 .. max_t - 1 (by FrameCode's own arithmetic, so the code has the same bits) and then gathered: the
    per-step work is one index_select and the Linear, nothing is read back, and the call can be captured.  The first call on a
    device builds the table and must therefore happen outside a capture.  The table depends on the constructor's arguments only
    (max_t, the video layout, scale, the number of frequencies), none of which is a parameter or changes afterwards, so it is never
    rebuilt.  An id outside [0, max_t) is clamped FOR THE LOOKUP ONLY, so that nothing is read out of bounds; the pose tail that
    consumes the code refuses the same id (NaN row, counted in its status word), so the clamped code never reaches a result."""

    def __init__(self, max_t, num_freq, embedding_dim, vid_offset, scale=1):
        super().__init__(num_freq, embedding_dim, vid_offset, scale=scale)
        self.max_t = max_t
        self._tables = {}

    def coefficients(self, device):
        tab = self._tables.get(str(device))
        if tab is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FrameCodeTable: the coefficient table is built on the first call -- call once before capture")
            with torch.no_grad():
                fid = torch.arange(self.max_t, device=device)
                vid, tid = fid_reindex(fid, self.num_vids, self.vid_offset)
                coeff = self.fourier_embed(L.dev(tid * self.scale).view(-1, 1))
                C = coeff.shape[1]
                wide = torch.zeros((self.max_t, C, self.num_vids), device=device)
                wide.scatter_(2, L.dev(vid, torch.int64).view(-1, 1, 1).expand(-1, C, 1), coeff[..., None])
                tab = wide.view(self.max_t, -1).contiguous()
            self._tables[str(device)] = tab
        return tab

    def forward(self, fid):
        tab = self.coefficients(fid.device)
        # a refused id (outside the table) is clamped for this lookup only: the tail writes NaN for its row and counts it
        rows = tab.index_select(0, fid.reshape(-1).long().clamp(0, self.max_t - 1))
        return A.LinearFn.apply(rows, self.basis_mlp.weight, self.basis_mlp.bias, 0)


class RTExpMLP(nn.Module):
    """nerf.py:429-470: the explicit table `base_rt` composed with the MLP delta `mlp_rt(root_code(id))`, the base's gradient
    magnified 10x.  State-dict keys as the reference's, the `delta_rt.0.*` / `delta_rt.1.*` aliases included."""

    def __init__(self, max_t, num_freqs, t_embed_dim, data_offset, delta=False):
        super().__init__()
        self.root_code = FrameCodeTable(max_t, num_freqs, t_embed_dim, data_offset, scale=0.1)
        self.base_rt = RTExplicit(max_t, delta=delta, rand=False)
        self.mlp_rt = RTHead(use_quat=False, in_channels_xyz=t_embed_dim, in_channels_dir=0, out_channels=6, raw_feat=True)
        self.delta_rt = nn.Sequential(self.root_code, self.mlp_rt)
        self.id_status = None

    def delta_rows(self, x):
        """The MLP's rows (n, 6) for the frame ids x."""
        return self.mlp_rt.raw(self.root_code(x))

    def forward(self, x):
        rtk, self.id_status = RootPoseFn.apply(self.base_rt.se3, x, self.delta_rows(x), None, RAW_NONE, 1.0, None, None, 3)
        return _rts12(rtk, x.shape[0])


def correct_bones(model, bones_rst, inverse=False, neudbs=True):
    """geom_utils.py:933-951: rest bones moved by the rest pose's transforms -> (bones_rst (B,10), bone_rts_rst (1, 8B))."""
    if not neudbs:
        raise NotImplementedError("linear blend skinning: MoDA runs neudbs (moda.py:72-73)")
    code = model.rest_pose_code.weight[:1]
    bone_rts_rst = model.nerf_body_rts[1](code)[0]
    B = bones_rst.shape[-2]
    if inverse:
        bone_rts_rst = dq_inverse(bone_rts_rst.view(-1, B, 8)).view(bone_rts_rst.shape)
    return bone_transform(bones_rst, bone_rts_rst, neudbs, is_vec=True)[0], bone_rts_rst


def reinit_bones(model, mesh, num_bones, neudbs):
    """geom_utils.py:857-903: a fresh pose-head output layer for `num_bones` bones and bones placed at the k-means centres of
    the mesh vertices, written into the existing parameters (none is added).  `mesh`: a TriMesh (its device vertices are used
    as they are) or anything with `.vertices`."""
    if not neudbs:
        raise NotImplementedError("linear blend skinning: MoDA runs neudbs (moda.py:72-73)")
    from .bones import kmeans
    device = model.device
    points = getattr(mesh, "vertices_t", None)
    if points is None:
        points = torch.as_tensor(np.asarray(mesh.vertices), dtype=torch.float32)
    points = points.detach().to(device=device, dtype=torch.float32)                   # :867
    rthead = model.nerf_body_rts[1].rgb
    num_in = rthead[0].weight.shape[1]                                                # :871
    rthead = nn.Sequential(nn.Linear(num_in, 7 * num_bones)).to(device)               # :873
    torch.nn.init.xavier_uniform_(rthead[0].weight, gain=0.5)
    torch.nn.init.zeros_(rthead[0].bias)
    if points.shape[0] < 100:                                                         # :880-883
        bound = torch.Tensor(np.asarray(model.latest_vars['obj_bound'], np.float32))[None]
        center = torch.rand(num_bones, 3) * bound * 2 - bound
    else:
        _, center = kmeans(X=points, num_clusters=num_bones, iter_limit=100, tqdm_flag=False, distance='euclidean',
                           device=device)                                             # :885-886
    center = center.to(device)
    orient = torch.Tensor([[1, 0, 0, 0]]).to(device)
    orient = orient.repeat(num_bones, 1)
    scale = torch.zeros(num_bones, 3).to(device)
    bones = torch.cat([center, orient, scale], -1)                                    # :891

    model.num_bones = num_bones
    num_output = model.nerf_body_rts[1].num_output
    bias_reinit = rthead[0].bias.data
    weight_reinit = rthead[0].weight.data
    model.nerf_body_rts[1].rgb[0].bias.data[:num_bones * num_output] = bias_reinit
    model.nerf_body_rts[1].rgb[0].weight.data[:num_bones * num_output] = weight_reinit

    bones, _ = correct_bones(model, bones, inverse=True, neudbs=neudbs)               # :900
    model.bones.data[:num_bones] = bones.detach()
    model.nerf_models['bones'] = model.bones
    return


def correct_rest_pose(opts, bone_rts_fw, bone_rts_rst, neudbs):
    """geom_utils.py:953-972: delta(J_b) = (J_b*)^-1 J_b for every frame's bone transforms."""
    if not neudbs:
        raise NotImplementedError("linear blend skinning: MoDA runs neudbs (moda.py:72-73)")
    shape = bone_rts_fw.shape
    B = opts.num_bones
    inv = dq_inverse(bone_rts_rst.view(-1, B, 8))
    fw = bone_rts_fw.reshape(-1, B, 8)
    return dq_mul(inv.expand(fw.shape[0], B, 8).contiguous(), fw.contiguous()).view(shape)


def update_delta_rts(model, rays):
    """moda.update_delta_rts (moda.py:1262-1279): the rest bones moved by the rest pose (kept in nerf_models['bones_rst'])
    and every bone_rts* entry of `rays` re-expressed relative to the rest pose."""
    opts = model.opts
    bones_rst, bone_rts_rst = correct_bones(model, model.nerf_models['bones'], neudbs=opts.neudbs)
    model.nerf_models['bones_rst'] = bones_rst
    for k in ('bone_rts', 'bone_rts_target', 'bone_rts_dentrg'):
        if k in rays:
            rays[k] = correct_rest_pose(opts, rays[k], bone_rts_rst, opts.neudbs)
    return rays


def update_rays(model, rays, is_pair, embedid, frame_layout=False):
    """The per-ray expansion of moda.update_rays (moda.py:1281-1311) for the neudbs configuration: frame codes and body
    poses evaluated once per frame, then repeated over the frame's `nsample` pixels (the layout render_rays takes).
    frame_layout=True keeps them as ONE row per frame, (bs, C), and records rays['rays_per_frame'] = nsample: render_rays
    then reads 8B + 128 + 64 floats per frame instead of per ray (the frame-grouped layout, rendering.FRAME_KEYS)."""
    ns = rays['nsample']
    embedid = embedid.long()
    if frame_layout:
        rep = lambda t: t
        rays['rays_per_frame'] = ns
        rays['rtk_vec'] = rays['rtk_vec'][:, 0]
    else:
        rep = lambda t: t[:, None].expand(t.shape[0], ns, t.shape[-1])
    if is_pair:
        rv = rays['rtk_vec']
        rays['rtk_vec_target'] = rv.reshape((2, rv.shape[0] // 2) + tuple(rv.shape[1:])).flip(0).reshape(rv.shape)
        target = embedid.view(2, -1).flip(0).reshape(-1)
        rays['bone_rts_target'] = rep(model.nerf_body_rts(target)[:, 0])
    rays['time_embedded'] = rep(model.pose_code(embedid))
    rays['bone_rts'] = rep(model.nerf_body_rts(embedid)[:, 0])
    if getattr(model, 'env_code', None) is not None:
        rays['env_code'] = rep(model.env_code(embedid))
    if getattr(model, 'appearance_code', None) is not None:
        rays['appearance_code'] = rep(model.appearance_code(embedid))
    return rays
