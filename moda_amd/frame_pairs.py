"""Frame-pair preparation, device-resident: what the reference's data loader does between decoded arrays and the batch
(dataloader/vidbase.py:142-246 -- compute_crop_params, the six cv2.remap calls of read_raw, flow_process with
ext_utils/flowlib.warp_flow) and banmo.convert_batch_input's reordering (nnutils/moda.py:1362-1417), plus fb_flow_check
(nnutils/geom_utils.py:1313-1342), with the reference's names.  The work is five HIP entries (csrc/framepair_kernels.hip):
moda_mask_bbox, moda_crop_params, moda_crop_remap, moda_flow_process, moda_remap.  Nothing is read back, so every call here can
be captured into a graph, and a captured call follows new masks.

The sampler restates cv2.remap (float maps, constant-zero border) from OpenCV's source; the restatement has not been run against
OpenCV.  Deviations from the reference, all deliberate:
  * Arrays are device tensors; images and planes passed to remap / warp_flow are channel-FIRST (C, H, W), not (H, W, C).
  * compute_crop_params raises on an empty mask and flow_process meets a singular matrix on a box of half-length 0.  Here both
    are counted in a device status word [#empty, #zero-length]; such a frame's kaug is NaN and its image outputs are 0, and the
    flow and occ of BOTH frames of its pair are 0.
  * A map coordinate that is NaN or infinite samples 0 (cv2 does the same through its saturating casts).
  * img is uint8 and each tap is divided by 255 in fp32 (the reference divides in float64 before the remap).
  * dps is fp32 (convert_batch_input's .float()).
  * flow_process uses the closed-form inverse of the diagonal-plus-translation crop matrix, not np.linalg.inv.
  * Inputs that require grad are refused: all of this is data loading."""
import torch

from . import _lib as L
from . import abi
from . import cse

INTER_NEAREST, INTER_LINEAR = abi.CONSTANTS["MODA_REMAP_NEAREST"], abi.CONSTANTS["MODA_REMAP_LINEAR"]       # cv2's values
CROP_FACTOR = 1.2                        # BaseDataset.crop_factor
MAX_SIDE = 32767                         # frames: pixels a side


def _no_grad(what, *tensors):
    if any(torch.is_tensor(t) and t.requires_grad for t in tensors):
        raise NotImplementedError(f"{what}: inputs that require grad are not implemented (frame preparation is data loading and "
                                  "has no backward); pass them detached")


def _cuda(what, *tensors):
    for t in tensors:
        if torch.is_tensor(t) and not t.is_cuda:
            raise RuntimeError(f"{what} takes CUDA (ROCm) tensors; the HIP library is the only compute path")


def _plane(what, name, t, dtypes, tail, lead=None):
    """A decoded array: a tensor of one of `dtypes`, contiguous, its trailing dimensions `tail` (None: any size); checked before
    the device so that the refusals need no GPU."""
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: {name} must be a tensor, got {type(t)}")
    if t.dtype not in dtypes or not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous {' or '.join(str(d) for d in dtypes)}, got {t.dtype}, "
                         f"contiguous={t.is_contiguous()}")
    if t.dim() < len(tail) or any(w is not None and s != w for s, w in zip(t.shape[t.dim() - len(tail):], tail)):
        raise ValueError(f"{what}: {name} must end in {tuple('*' if w is None else w for w in tail)}, got {tuple(t.shape)}")
    if lead is not None and tuple(t.shape[:t.dim() - len(tail)]) != tuple(lead):
        raise ValueError(f"{what}: {name} must lead with {tuple(lead)}, got {tuple(t.shape)}")
    return t


def _size(what, img_size):
    if int(img_size) != img_size or not 1 <= int(img_size) <= 16384:
        raise ValueError(f"{what}: img_size = {img_size} outside 1..16384")
    return int(img_size)


def mask_bbox(masks):
    """masks (..., h, w), fp32 or uint8, the object wherever the value is > 0 -> int32 (..., 4) = xmin, xmax, ymin, ymax
    (np.where(mask > 0) and its min / max).  An empty mask gives (w, -1, h, -1)."""
    _no_grad("mask_bbox", masks)
    _plane("mask_bbox", "masks", masks, (torch.float32, torch.uint8), (None, None))
    if masks.dim() < 2 or masks.numel() == 0 or max(masks.shape[-2:]) > MAX_SIDE:
        raise ValueError(f"mask_bbox: masks must be (..., h, w) with 1 <= h, w <= {MAX_SIDE}, got {tuple(masks.shape)}")
    _cuda("mask_bbox", masks)
    h, w = masks.shape[-2:]
    B = masks.numel() // (h * w)
    box = torch.empty(tuple(masks.shape[:-2]) + (4,), device=masks.device, dtype=torch.int32)
    L.call("moda_mask_bbox", L.ptr(masks), 1 if masks.dtype == torch.uint8 else 0, B, h, w, L.ptr(box), L.stream())
    return box


def _crop_params(box, B, bs, img_size, crop_factor, status):
    kaug = torch.empty((B, 4), device=box.device, dtype=torch.float32)
    affine = torch.empty((B, 4), device=box.device, dtype=torch.float64)
    if status is None:
        status = torch.zeros((2,), device=box.device, dtype=torch.int32)
    L.call("moda_crop_params", L.ptr(box), B, bs, img_size, float(crop_factor), L.ptr(kaug), L.ptr(affine), L.ptr(status), L.stream())
    return kaug, affine, status


def compute_crop_params(masks, img_size, crop_factor=CROP_FACTOR, *, pair_major=False, status=None):
    """BaseDataset.compute_crop_params for every frame of masks (B, h, w) | (bs, 2, h, w) -> (kaug (B,4) fp32, affine (B,4)
    float64, status (2,) int32).  kaug = [alp0, alp1, cx - lx, cy - ly]; affine holds the same values unrounded: the reference's
    hp0 is (col * alp0 + tx, row * alp1 + ty) and its B matrix is diag(alp) with that translation.  pair_major (masks
    (bs, 2, h, w)): the rows come out as convert_batch_input orders them, all first frames then all second frames.
    status counts [empty masks, boxes of half-length 0]; those rows are NaN."""
    _no_grad("compute_crop_params", masks)
    img_size = _size("compute_crop_params", img_size)
    if not 0 < float(crop_factor) < 1024:
        raise ValueError(f"compute_crop_params: crop_factor = {crop_factor}")
    if torch.is_tensor(masks) and pair_major and (masks.dim() != 4 or masks.shape[1] != 2):
        raise ValueError(f"compute_crop_params: pair_major takes masks (bs, 2, h, w), got {tuple(masks.shape)}")
    box = mask_bbox(masks).reshape(-1, 4)
    B = box.shape[0]
    return _crop_params(box, B, B // 2 if pair_major else 0, img_size, crop_factor, status)


def remap(src, map_x, map_y, interpolation=INTER_LINEAR):
    """cv2.remap(src, map_x, map_y, interpolation) with the constant-zero border: src (C, Hs, Ws) | (Hs, Ws) fp32 planes, maps
    (H, W) fp32 -> (C, H, W) | (H, W).  A NaN or infinite coordinate samples 0."""
    _no_grad("remap", src, map_x, map_y)
    _plane("remap", "src", src, (torch.float32,), (None, None))
    _plane("remap", "map_x", map_x, (torch.float32,), (None, None))
    _plane("remap", "map_y", map_y, (torch.float32,), (None, None))
    if src.dim() not in (2, 3) or map_x.dim() != 2 or map_x.shape != map_y.shape or src.numel() == 0 or map_x.numel() == 0:
        raise ValueError(f"remap: src {tuple(src.shape)} must be (C, Hs, Ws) or (Hs, Ws), the maps {tuple(map_x.shape)} and "
                         f"{tuple(map_y.shape)} one (H, W)")
    if max(src.shape[-2:]) > MAX_SIDE:
        raise ValueError(f"remap: src of {tuple(src.shape)} has more than {MAX_SIDE} pixels a side")
    if interpolation not in (INTER_NEAREST, INTER_LINEAR):
        raise ValueError(f"remap: interpolation = {interpolation}; INTER_NEAREST (0) and INTER_LINEAR (1) are implemented")
    _cuda("remap", src, map_x, map_y)
    C = src.shape[0] if src.dim() == 3 else 1
    H, W = map_x.shape
    dst = torch.empty((C, H, W) if src.dim() == 3 else (H, W), device=src.device, dtype=torch.float32)
    L.call("moda_remap", L.ptr(src), C, src.shape[-2], src.shape[-1], L.ptr(map_x), L.ptr(map_y), H, W, int(interpolation), L.ptr(dst),
           L.stream())
    return dst


def warp_flow(img, flow, normed=False):
    """flowlib.warp_flow: img (C, h, w) fp32 sampled linearly at pixel + flow, flow (2, h, w) fp32 in pixels, or in NDC when
    `normed` (then scaled by w / 2, h / 2).  The map is formed in fp32 as the reference does."""
    _no_grad("warp_flow", img, flow)
    _plane("warp_flow", "img", img, (torch.float32,), (None, None))
    _plane("warp_flow", "flow", flow, (torch.float32,), (2, None, None))
    if flow.dim() != 3:
        raise ValueError(f"warp_flow: flow must be (2, h, w), got {tuple(flow.shape)}")
    _cuda("warp_flow", img, flow)
    h, w = flow.shape[1:]
    fx, fy = flow[0], flow[1]
    if normed:
        fx, fy = fx * w / 2., fy * h / 2.
    map_x = (fx + torch.arange(w, device=flow.device, dtype=torch.float32)[None, :]).contiguous()
    map_y = (fy + torch.arange(h, device=flow.device, dtype=torch.float32)[:, None]).contiguous()
    return remap(img, map_x, map_y, INTER_LINEAR)


def fb_flow_check(flo_refr, flo_targ):
    """geom_utils.fb_flow_check without its image-saving branch: two NDC flows (2, h, w) fp32 -> (fberr_fw, fberr_bw), each
    (h, w) fp32, the forward-backward error in NDC, 0 where the flow itself is 0.  (The reference scales both axes by the width.)"""
    _no_grad("fb_flow_check", flo_refr, flo_targ)
    for n, t in (("flo_refr", flo_refr), ("flo_targ", flo_targ)):
        _plane("fb_flow_check", n, t, (torch.float32,), (2, None, None))
    if flo_refr.dim() != 3 or flo_refr.shape != flo_targ.shape:
        raise ValueError(f"fb_flow_check: flows of {tuple(flo_refr.shape)} and {tuple(flo_targ.shape)}")
    _cuda("fb_flow_check", flo_refr, flo_targ)
    h, w = flo_refr.shape[1:]
    dev = flo_refr.device
    hp0 = torch.stack([torch.arange(w, device=dev, dtype=torch.float32)[None, :].expand(h, w),
                       torch.arange(h, device=dev, dtype=torch.float32)[:, None].expand(h, w)])
    out = []
    for a, b in ((flo_refr, flo_targ), (flo_targ, flo_refr)):
        a_px, b_px = a * w / 2, b * w / 2
        fb = 2 * (warp_flow((hp0 + b_px).contiguous(), a_px.contiguous()) - hp0) / w
        err = torch.sqrt(fb[0] * fb[0] + fb[1] * fb[1])
        out.append(torch.where(torch.sqrt(a[0] * a[0] + a[1] * a[1]) > 0, err, torch.zeros_like(err)))
    return out[0], out[1]


def _frames(what, planes, lead=None):
    """Validate the decoded planes of one call (shared (h, w)); returns (lead, h, w)."""
    specs = {"img": ((torch.uint8,), 3), "flow": ((torch.float32,), 2), "occ": ((torch.float32,), None),
             "mask": ((torch.float32, torch.uint8), None), "dp": ((torch.int32,), None)}
    hw = None
    for name, t in planes.items():
        if t is None:
            continue
        dtypes, ch = specs[name]
        tail = (None, None) if ch is None else (None, None, ch)
        _plane(what, name, t, dtypes, tail)
        this_lead, this_hw = tuple(t.shape[:t.dim() - len(tail)]), tuple(t.shape[t.dim() - len(tail):][:2])
        if lead is None:
            lead = this_lead
        if this_lead != tuple(lead):
            raise ValueError(f"{what}: {name} must lead with {tuple(lead)}, got {tuple(t.shape)}")
        if hw is None:
            hw = this_hw
        if this_hw != hw:
            raise ValueError(f"{what}: the frames of one call share (h, w); {name} is {this_hw}, another plane {hw} (a flow stored at "
                             "another resolution is not resized here)")
    if hw is None or min(hw) < 1 or max(hw) > MAX_SIDE or len(lead) == 0 or min(lead) < 1:
        raise ValueError(f"{what}: frames {tuple(lead)} x {hw}")
    return tuple(lead), hw[0], hw[1]


def crop_frames(affine, img_size, *, img=None, flow=None, occ=None, mask=None, dp=None, pair_major=False):
    """The six cv2.remap calls of read_raw for every frame at once: affine (B,4) float64 from compute_crop_params (in OUTPUT
    order), planes led by (B,) or, with pair_major, by (bs, 2): img (...,h,w,3) uint8, flow (...,h,w,2) fp32, occ (...,h,w) fp32,
    mask (...,h,w) fp32 | uint8, dp (...,h,w) int32; a plane left None is skipped.  Returns a dict of fp32 tensors: 'imgs'
    (B,3,S,S), 'flow' (B,2,S,S) (still in source pixels: flow_process comes next), 'occ', 'masks' ((mask * vis2d) > 0), 'dps',
    'vis2d' (B,S,S).  pair_major: output row k bs + p holds frame (p, k)."""
    planes = {"img": img, "flow": flow, "occ": occ, "mask": mask, "dp": dp}
    _no_grad("crop_frames", affine, *planes.values())
    S = _size("crop_frames", img_size)
    lead, h, w = _frames("crop_frames", planes)
    _plane("crop_frames", "affine", affine, (torch.float64,), (4,))
    if pair_major and (len(lead) != 2 or lead[1] != 2):
        raise ValueError(f"crop_frames: pair_major takes planes led by (bs, 2), got {lead}")
    B = 1
    for n in lead:
        B *= n
    if affine.numel() != 4 * B:
        raise ValueError(f"crop_frames: affine holds {affine.numel() // 4} rows for {B} frames")
    _cuda("crop_frames", affine, *planes.values())
    dev = affine.device

    def new(C=None):
        return torch.empty((B, S, S) if C is None else (B, C, S, S), device=dev, dtype=torch.float32)

    out = {"imgs": new(3) if img is not None else None, "flow": new(2) if flow is not None else None,
           "occ": new() if occ is not None else None, "masks": new() if mask is not None else None,
           "dps": new() if dp is not None else None, "vis2d": new()}
    L.call("moda_crop_remap", L.ptr(img), L.ptr(flow), L.ptr(occ), L.ptr(mask), 1 if mask is not None and mask.dtype == torch.uint8 else 0,
           L.ptr(dp), L.ptr(affine), B, B // 2 if pair_major else 0, h, w, S, L.ptr(out["imgs"]), L.ptr(out["flow"]), L.ptr(out["occ"]),
           L.ptr(out["masks"]), L.ptr(out["dps"]), L.ptr(out["vis2d"]), L.stream())
    return {k: v for k, v in out.items() if v is not None}


def flow_process(flow, affine, img_size):
    """BaseDataset.flow_process for bs pairs in one launch: flow (2 bs,2,S,S) fp32, the cropped flows in source pixels, pair-major
    (row p and row bs + p are a pair: flow and flown); affine (2 bs,4) float64 in the same order -> (flow (2 bs,2,S,S) in NDC of
    the other frame's crop, occ (2 bs,S,S) = exp(-25 * 2 |dis| / S), 0 below 0.25).  The incoming occ planes are not needed: the
    reference overwrites them."""
    _no_grad("flow_process", flow, affine)
    S = _size("flow_process", img_size)
    _plane("flow_process", "flow", flow, (torch.float32,), (2, S, S))
    _plane("flow_process", "affine", affine, (torch.float64,), (4,))
    if flow.dim() != 4 or flow.shape[0] % 2 or flow.shape[0] < 2 or affine.numel() != 4 * flow.shape[0]:
        raise ValueError(f"flow_process: flow {tuple(flow.shape)} must be (2 bs, 2, {S}, {S}) with affine (2 bs, 4), got "
                         f"{tuple(affine.shape)}")
    _cuda("flow_process", flow, affine)
    out = torch.empty_like(flow)
    occ = torch.empty((flow.shape[0], S, S), device=flow.device, dtype=torch.float32)
    L.call("moda_flow_process", L.ptr(flow), L.ptr(affine), flow.shape[0] // 2, S, L.ptr(out), L.ptr(occ), L.stream())
    return out, occ


RAW_KEYS = ("img", "mask", "flow", "occ", "dp", "dp_feat", "dp_bbox", "rtk", "dataid", "frameid")


def _pair_major(t, bs):
    return t.reshape(bs, 2, *t.shape[2:]).transpose(0, 1).reshape(2 * bs, *t.shape[2:])


def prepare_frame_pairs(raw, img_size, *, crop_factor=CROP_FACTOR, status=None):
    """Decoded device arrays of bs frame pairs -> the attributes convert_batch_input sets and sample_pxs consumes.

    raw: img (bs,2,h,w,3) uint8; mask (bs,2,h,w) fp32 | uint8; flow (bs,2,h,w,2) fp32; occ (bs,2,h,w) fp32 (validated, not read:
    flow_process replaces it); dp (bs,2,h,w) int32; dp_feat (bs,2,16,hf,wf) fp32; dp_bbox (bs,2,4); rtk (bs,2,4,4); dataid,
    frameid (bs,2).  Returns a dict, every frame-indexed entry pair-major (2 bs rows): imgs (.,3,S,S), masks, vis2d, dps, occ
    (.,S,S), flow (.,2,S,S), rtk (.,4,4), rt_raw (.,3,4), kaug (.,4), dp_bbox (.,4), dp_feats (.,16,hf,wf) L2-normalised,
    dp_feats_rsmp (.,16,S,S) (cse.resample_dp of the normalised features, as read_raw computes it), dataid, frameid (int64),
    and 'status' (2,) int32 [#empty masks, #zero-length boxes].  No host read-back: the call can be captured."""
    missing = [k for k in RAW_KEYS if k not in raw]
    if missing:
        raise ValueError(f"prepare_frame_pairs: raw lacks {missing}")
    _no_grad("prepare_frame_pairs", *(raw[k] for k in RAW_KEYS))
    S = _size("prepare_frame_pairs", img_size)
    planes = {k: raw[k] for k in ("img", "flow", "occ", "mask", "dp")}
    lead, h, w = _frames("prepare_frame_pairs", planes)
    if len(lead) != 2 or lead[1] != 2:
        raise ValueError(f"prepare_frame_pairs: every key leads with (bs, 2), img leads with {lead}")
    bs = lead[0]
    _plane("prepare_frame_pairs", "dp_feat", raw["dp_feat"], (torch.float32,), (cse.CHANNELS, None, None), lead)
    for k, tail in (("dp_bbox", (4,)), ("rtk", (4, 4)), ("dataid", ()), ("frameid", ())):
        t = raw[k]
        if not torch.is_tensor(t) or tuple(t.shape) != lead + tail:
            raise ValueError(f"prepare_frame_pairs: {k} must be a tensor of shape {lead + tail}")
    _cuda("prepare_frame_pairs", *(raw[k] for k in RAW_KEYS))
    kaug, affine, status = compute_crop_params(raw["mask"], S, crop_factor, pair_major=True, status=status)
    crop = crop_frames(affine, S, img=raw["img"], flow=raw["flow"], mask=raw["mask"], dp=raw["dp"], pair_major=True)
    flow, occ = flow_process(crop["flow"], affine, S)
    rtk = _pair_major(raw["rtk"].float(), bs).contiguous()
    dp_bbox = _pair_major(raw["dp_bbox"].float(), bs).contiguous()
    feats = _pair_major(raw["dp_feat"], bs).contiguous()
    dp_feats = torch.nn.functional.normalize(feats, 2, 1)
    return {"imgs": crop["imgs"], "masks": crop["masks"], "vis2d": crop["vis2d"], "dps": crop["dps"], "flow": flow, "occ": occ,
            "rtk": rtk, "rt_raw": rtk[:, :3].clone(), "kaug": kaug, "dp_bbox": dp_bbox, "dp_feats": dp_feats,
            "dp_feats_rsmp": cse.resample_dp(dp_feats, dp_bbox, kaug, S),
            "dataid": _pair_major(raw["dataid"], bs).long(), "frameid": _pair_major(raw["frameid"], bs).long(), "status": status}
