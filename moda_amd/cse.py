"""DensePose-CSE observations, device-resident: the reference's resample_dp / bbox_dp2rnd (nnutils/geom_utils.py:1665-1701, called
from banmo.set_input, moda.py:1515-1543), ood_check_cse (:1610-1663, called per video from eval_cam, train_utils.py:393-453) and
compute_flow_cse / match2flo / match2coords (:1207-1247, scripts/visualize/match.py), with the reference's names and argument
order.  The work is three HIP entries (csrc/cse_kernels.hip): moda_feat_argmax -- for every 16-channel query row the candidate
row with the largest dot product, the score matrix never written -- moda_grid_resample and moda_ood_error.  Nothing is read back,
so every call here can be captured into a graph.

Deviations from the reference, all deliberate:
  * ood_check_cse returns DEVICE tensors (bool valid_list, fp32 error_list); the whole batch is one arg-max launch.
  * The arg-max order is stated where torch's CUDA argmax leaves ties open: the larger score, then the lowest index; a NaN score
    beats every number (lowest NaN index); -0 == +0.  The score is the fp32 fma chain over the 16 channels in ascending order.
  * A dp_idx value outside [0, N) is not read through: it contributes nothing and is counted (`return_status=True`).
  * resample_dp's test `dp_bbox.abs().sum() == 0` is evaluated on the device; a batch row whose box is degenerate while another
    row's is not gives zeros (its coordinates are not numbers), not an error.
  * Inputs that require grad are refused: every call site of the reference is under no_grad or in the data loader.
"""
import torch

from . import _lib as L
from . import abi
from .geom_utils import K2inv, K2mat, Kmatinv

CHANNELS = abi.CONSTANTS["MODA_CSE_CHANNELS"]
QUERY_TILE = abi.CONSTANTS["MODA_CSE_QUERY_TILE"]
CAND_TILE = abi.CONSTANTS["MODA_CSE_CAND_TILE"]
OOD_MAX_BLOCKS = abi.CONSTANTS["MODA_OOD_MAX_BLOCKS"]
OOD_THRESHOLD = 12.0        # ood_check_cse's err_threshold
_GRID, _DP, _INTERP = abi.CONSTANTS["MODA_RESAMPLE_GRID"], abi.CONSTANTS["MODA_RESAMPLE_DP"], abi.CONSTANTS["MODA_RESAMPLE_INTERP"]


def _no_grad(what, *tensors):
    if any(torch.is_tensor(t) and t.requires_grad for t in tensors):
        raise NotImplementedError(f"{what}: inputs that require grad are not implemented (the CSE kernels have no backward; the "
                                  "reference calls this under no_grad or in the data loader); pass them detached")


def _feats(what, t, dims, square=False):
    """A feature image: fp32, contiguous, (…,16,h,w); checked before the device so that the refusals do not need a GPU."""
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: expected a tensor, got {type(t)}")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{what}: features must be contiguous fp32, got {t.dtype}, contiguous={t.is_contiguous()}")
    if t.dim() != dims:
        raise ValueError(f"{what}: expected {dims} dimensions, got shape {tuple(t.shape)}")
    if t.shape[-3] != CHANNELS:
        raise NotImplementedError(f"{what}: C = {t.shape[-3]} channels; the kernels are built for C = {CHANNELS}")
    if square and t.shape[-1] != t.shape[-2]:
        raise ValueError(f"{what}: feature images must be square (the reference's sample_xy(w, ...).view(h, w, 2) needs it), "
                         f"got {t.shape[-2]} x {t.shape[-1]}")
    return t


def _cuda(what, *tensors):
    for t in tensors:
        if torch.is_tensor(t) and not t.is_cuda:
            raise RuntimeError(f"{what} takes CUDA (ROCm) tensors; the HIP library is the only compute path")


def argmax_splits(B, N, M, splits=0):
    """(number of candidate ranges, their length) moda_feat_argmax uses; splits = 0: the library's choice."""
    rng = L._I64(0)
    n = L.load().moda_feat_argmax_splits(int(B), int(N), int(M), int(splits), L._c.byref(rng))
    return int(n), int(rng.value)


def _argmax(q, q_str, c, c_str, B, N, M, splits):
    idx = torch.empty((B, N), device=c.device, dtype=torch.int32)
    if N == 0:
        return idx
    n, _ = argmax_splits(B, N, M, splits)
    keys = torch.empty((B * N,), device=c.device, dtype=torch.int64) if n > 1 else None
    L.call("moda_feat_argmax", L.ptr(q), *q_str, L.ptr(c), *c_str, B, N, M, int(splits) if n > 1 else 1, L.ptr(idx), L.ptr(keys),
           L.stream())
    return idx


def feat_argmax(queries, candidates, *, splits=0):
    """queries (N,16) | (B,N,16) | (1,N,16), candidates (M,16) | (B,M,16), fp32 device tensors of ANY strides (a transposed view of
    a (16,h,w) image is read in place) -> idx (N,) | (B,N) int64: per query the candidate with the largest dot product, in the
    order stated in the module docstring.  splits: 0 lets the library cut the candidates into ranges, > 0 forces that many."""
    _no_grad("feat_argmax", queries, candidates)
    for name, t in (("queries", queries), ("candidates", candidates)):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError(f"feat_argmax: {name} must be an fp32 tensor")
        if t.dim() not in (2, 3):
            raise ValueError(f"feat_argmax: {name} must be (rows, 16) or (B, rows, 16), got {tuple(t.shape)}")
        if t.shape[-1] != CHANNELS:
            raise NotImplementedError(f"feat_argmax: C = {t.shape[-1]} channels; the kernel is built for C = {CHANNELS}")
    _cuda("feat_argmax", queries, candidates)
    batched = candidates.dim() == 3 or queries.dim() == 3
    q = queries if queries.dim() == 3 else queries[None]
    c = candidates if candidates.dim() == 3 else candidates[None]
    B = max(q.shape[0], c.shape[0])
    if c.shape[0] not in (1, B) or q.shape[0] not in (1, B) or c.shape[1] < 1:
        raise ValueError(f"feat_argmax: queries {tuple(queries.shape)} against candidates {tuple(candidates.shape)}")
    q_str = (q.stride(0) if q.shape[0] == B and B > 1 else 0, q.stride(1), q.stride(2))
    c_str = (c.stride(0) if c.shape[0] == B and B > 1 else 0, c.stride(1), c.stride(2))
    idx = _argmax(q, q_str, c, c_str, B, q.shape[1], c.shape[1], splits).long()
    return idx if batched else idx[0]


def bbox_dp2rnd(bbox, kaug):
    """geom_utils.bbox_dp2rnd: bbox (bs,4), kaug (bs,4) -> (bs,3,3), the map from DensePose-box to rendered-box coordinates."""
    cropa2im = torch.cat([(bbox[:, 2:] - bbox[:, :2]) / 112., bbox[:, :2]], -1)
    return K2inv(kaug).matmul(K2mat(cropa2im))


def _resample(src, Hd, Wd, mode, affine=None, dp_bbox=None, kaug=None, normalize=False):
    B, C, Hs, Ws = src.shape
    dst = torch.empty((B, C, Hd, Wd), device=src.device, dtype=torch.float32)
    L.call("moda_grid_resample", L.ptr(src), B, C, Hs, Ws, Hd, Wd, mode, L.ptr(affine), L.ptr(dp_bbox), L.ptr(kaug),
           1 if normalize else 0, L.ptr(dst), L.stream())
    return dst


def resample_dp(dp_feats, dp_bbox, kaug, target_size, *, normalize=False):
    """geom_utils.resample_dp: dp_feats (bs,16,h,w), dp_bbox (bs,4), kaug (bs,4) -> (bs,16,target_size,target_size) in one launch:
    F.interpolate(bilinear) when dp_bbox is all zero, F.grid_sample through Kmatinv(bbox_dp2rnd(dp_bbox, kaug)) otherwise (the
    test and the affine are evaluated inside the kernel).  normalize=True fuses the F.normalize(., 2, 1) both call sites apply."""
    _no_grad("resample_dp", dp_feats, dp_bbox, kaug)
    _feats("resample_dp", dp_feats, 4)
    _cuda("resample_dp", dp_feats, dp_bbox, kaug)
    bs = dp_feats.shape[0]
    dp_bbox, kaug = L.dev(dp_bbox).reshape(-1, 4), L.dev(kaug).reshape(-1, 4)
    if dp_bbox.shape[0] != bs or kaug.shape[0] != bs or int(target_size) < 1:
        raise ValueError(f"resample_dp: dp_feats, dp_bbox, kaug hold {bs}, {dp_bbox.shape[0]}, {kaug.shape[0]} entries, "
                         f"target_size = {target_size}")
    return _resample(dp_feats, int(target_size), int(target_size), _DP, dp_bbox=dp_bbox, kaug=kaug, normalize=normalize)


def ood_check_cse(dp_feats, dp_embed, dp_idx, *, return_status=False, splits=0):
    """geom_utils.ood_check_cse: dp_feats (bs,16,h,w), dp_embed (N,16), dp_idx (bs,H,W) integer-valued ->
    (valid_list (bs,) bool, error_list (bs,) fp32), device tensors; with return_status also the int32 counter (1,) of dp_idx values
    outside [0, N).  Per frame: every embedding row is matched to its best pixel (ONE arg-max launch for the batch), and the mean
    distance between a pixel and the match of its dp_idx, over the pixels with dp_idx != 0, is compared with 12."""
    _no_grad("ood_check_cse", dp_feats, dp_embed, dp_idx)
    _feats("ood_check_cse", dp_feats, 4, square=True)
    if not torch.is_tensor(dp_embed) or dp_embed.dtype != torch.float32 or not dp_embed.is_contiguous() or dp_embed.dim() != 2:
        raise ValueError("ood_check_cse: dp_embed must be a contiguous fp32 (N, 16) tensor")
    if dp_embed.shape[1] != CHANNELS:
        raise NotImplementedError(f"ood_check_cse: C = {dp_embed.shape[1]} channels; the kernels are built for C = {CHANNELS}")
    _cuda("ood_check_cse", dp_feats, dp_embed, dp_idx)
    bs, _, h, w = dp_feats.shape
    N = dp_embed.shape[0]
    if dp_idx.dim() != 3 or dp_idx.shape[0] != bs or N < 1:
        raise ValueError(f"ood_check_cse: dp_idx {tuple(dp_idx.shape)} for {bs} frames, N = {N}")
    dp_idx = dp_idx.to(torch.int32).contiguous()                          # the reference: .float() ... .long()
    img = dp_feats.view(bs, CHANNELS, h * w)
    idx = _argmax(dp_embed, (0, CHANNELS, 1), img, (img.stride(0), 1, h * w), bs, N, h * w, splits)
    partials = torch.empty((bs * OOD_MAX_BLOCKS * 2,), device=img.device, dtype=torch.float64)
    error = torch.empty((bs,), device=img.device, dtype=torch.float32)
    valid = torch.empty((bs,), device=img.device, dtype=torch.bool)
    status = torch.zeros((1,), device=img.device, dtype=torch.int32)
    L.call("moda_ood_error", L.ptr(idx), L.ptr(dp_idx), bs, N, h, w, dp_idx.shape[1], dp_idx.shape[2], OOD_THRESHOLD, L.ptr(partials),
           L.ptr(error), L.ptr(valid), L.ptr(status), L.stream())
    return (valid, error, status) if return_status else (valid, error)


def match2coords(match, w_rszd):
    """geom_utils.match2coords: pixel indices (P,) -> (P,2) fp32 (x, y)."""
    return torch.cat([match[:, None] % w_rszd, match[:, None] // w_rszd], -1).float()


def match2flo(match, w_rszd, img_size, warp_r, warp_t, device=None):
    """geom_utils.match2flo: the matches (w*w,) of a w x w feature image -> flow (2,w,w) in the reference frame's crop; the final
    F.grid_sample is the resample kernel in grid mode on the 2-channel image."""
    _no_grad("match2flo", match, warp_r, warp_t)
    _cuda("match2flo", match, warp_r, warp_t)
    w = int(w_rszd)
    warp_r, warp_t = L.dev(warp_r), L.dev(warp_t)
    ar = torch.arange(w, device=match.device, dtype=torch.float32)
    xy = torch.stack([ar[None, :].expand(w, w), ar[:, None].expand(w, w)], -1).reshape(-1, 2)
    ref_coord = xy.matmul(warp_r[:2, :2]) + warp_r[None, :2, 2]
    tar_coord = match2coords(match, w).matmul(warp_t[:2, :2]) + warp_t[None, :2, 2]
    flo_dp = ((tar_coord - ref_coord) / img_size * 2).view(w, w, 2).permute(2, 0, 1).contiguous()
    inv = Kmatinv(warp_r[None])[0]
    sc = float(img_size / w)
    affine = torch.stack([inv[0, 0] * sc, inv[1, 0] * sc, inv[0, 2], inv[0, 1] * sc, inv[1, 1] * sc, inv[1, 2]]).reshape(1, 6).contiguous()
    return _resample(flo_dp[None], w, w, _GRID, affine=affine)[0]


def compute_flow_cse(cse_a, cse_b, warp_a, warp_b, img_size, *, splits=0):
    """geom_utils.compute_flow_cse: two (16,w,w) feature images -> (flo_a, flo_b), each (2,w,w).  Two arg-max launches with the
    operands swapped: cost.max(1) and cost.max(0) of the (w*w)^2 volume, which is never formed."""
    _no_grad("compute_flow_cse", cse_a, cse_b, warp_a, warp_b)
    _feats("compute_flow_cse", cse_a, 3, square=True)
    _feats("compute_flow_cse", cse_b, 3, square=True)
    if cse_a.shape != cse_b.shape:
        raise ValueError(f"compute_flow_cse: feature images of {tuple(cse_a.shape)} and {tuple(cse_b.shape)}")
    _cuda("compute_flow_cse", cse_a, cse_b, warp_a, warp_b)
    w = cse_a.shape[-1]
    P = w * w
    st = (0, 1, P)
    match_a = _argmax(cse_a, st, cse_b, st, 1, P, P, splits)[0].long()
    match_b = _argmax(cse_b, st, cse_a, st, 1, P, P, splits)[0].long()
    flo_a = match2flo(match_a, w, img_size, warp_a, warp_b, cse_a.device)
    flo_b = match2flo(match_b, w, img_size, warp_b, warp_a, cse_a.device)
    return flo_a, flo_b
