"""Evaluation-frame rendering, device-resident: the image half of v2s_trainer.eval() (nnutils/train_utils.py:455-624) -- what the
trainer runs after every epoch and what extract.py writes.  render_vid -> nerf_render in evaluation mode over whole observed
frames (train_utils.py:1345-1362, moda.py:850-928), the per-key masking and normalisation of train_utils.py:496-520,
add_image_grid / image_grid / add_image (train_utils.py:1482-1504, vis_utils.py:5-16), flow_to_image
(third_party/ext_utils/flowlib.py:86-214) and save_vid's frame preparation (utils/io.py:242-258).  The mesh half of eval() is
animate.py / mesh.py.

Everything from the chunk loop outwards runs on the device: five HIP entries (include/moda_hip_vis.h,
csrc/evalvis_kernels.hip) replace the reference's `.max()` / `.min()` read per key and chunk and its numpy pass over every frame.
Inference only: inputs that require grad raise NotImplementedError; lbs and the flow warps are refused, as everywhere in this
package.  Nothing is read back by any function here, and every function can be captured in a HIP graph after one eager warm-up
call (which builds the cached op tables and the colour wheel).

Deviations from the reference, all deliberate:
  * flow_to_image does not zero the unknown pixels of the caller's array (the reference writes u[idxUnknow] = 0 through a view).
  * An fp32 flow is coloured as numpy >= 2 colours it by default: `maxrad + np.finfo(float).eps` is a float64 scalar, which NEP 50
    no longer demotes, so u, v, the radius, the angle and fk are float64 after the division.  numpy < 2 kept them fp32 (the sum
    then being fp32 as well); f64_after_norm=False gives that arithmetic.  The two differ by one level on about 1.5 % of the
    channels and by whole branches of `rad <= 1` on the frame's longest vectors.
  * A frame with a NaN radius is normalised by -1, as the reference's `max(-1, np.max(rad))` returns its first argument then.
  * numpy's float -> uint8 cast is undefined outside [0, 256).  The rule here: truncate toward zero, saturate to [0, 255],
    NaN -> 0; in-range values equal numpy's.  Saturations and NaNs are counted in the status word.
  * Masks are square (the kernels resize (Sm, Sm) -> (S, S)); the reference's F.interpolate takes any rectangle.
Out of scope: reading and decoding files, imageio, cv2.resize (the gif downscale of save_vid), draw_cams / save_cams,
TensorBoard, the arrows of cat_imgflo / point_vec, any backward pass.  The eval() block and save_vid are methods behind heavy
imports: they are restated (tests/evalvis_numpy.py) and not pinned to a reference run; flow_to_image and image_grid are."""
import collections

import numpy as np
import torch

from . import _lib as L
from . import abi

C = abi.VIS_CONSTANTS
TILE = C["MODA_VIS_TILE"]
OP_MASK, OP_MUL, OP_SUBMIN, OP_SCALE255 = (C["MODA_VIS_OP_" + k] for k in ("MASK", "MUL", "SUBMIN", "SCALE255"))
OP_UNIT, OP_CLAMP01, OP_RAD = (C["MODA_VIS_OP_" + k] for k in ("UNIT", "CLAMP01", "RAD"))
STATUS_FIELDS = ("zero_div", "nan_ext", "saturated", "nan_u8")

FLOW_TAGS = ('flo_coarse', 'fdp_coarse', 'flo', 'fdp', 'flo_at_samp')                # v2s_trainer.isflow
SCALED_TAGS = ('depth_rnd', 'occ', 'unc_pred', 'proj_err', 'feat_err')               # add_image_grid's scale=True
VIS_KEYS = ('xyz_camera_vis', 'xyz_canonical_vis', 'pts_exp_vis', 'pts_pred_vis')    # render_vid drops these
_RAY_SKIP = ('unc_candidates', 'pxs_status', 'obs_status')


def _no_grad(what, *tensors):
    if any(torch.is_tensor(t) and t.requires_grad for t in tensors):
        raise NotImplementedError(f"{what}: inputs that require grad are not implemented (evaluation frames have no backward); "
                                  "pass them detached")


def _refuse_warps(what, model):
    opts = model.opts
    if getattr(opts, 'lbs', False) or getattr(opts, 'flowbw', False) or any(k in model.nerf_models for k in ('flowbw', 'flowfw')):
        raise NotImplementedError(f"{what}: linear blend skinning and the flow warps are not implemented (MoDA runs neudbs)")


def _f32(what, t):
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: expected a tensor, got {type(t)}")
    _no_grad(what, t)
    if not t.is_cuda:
        raise RuntimeError(f"{what} takes CUDA (ROCm) tensors; the HIP library is the only compute path")
    return L.dev(t.detach())


def new_status(device):
    """The device status word: int32 [keys with a zero divisor, keys with a NaN extremum, saturated 8-bit values, NaNs -> 0]."""
    return torch.zeros((4,), device=device, dtype=torch.int32)


_TABLES = {}


def _cached(key, device, make, dtype):
    k = (key, str(device))
    t = _TABLES.get(k)
    if t is None:
        t = _TABLES[k] = torch.as_tensor(make(), dtype=dtype).to(device).contiguous()
    return t


def _op_table(rows, device):
    """rows: ((off, n, C, flags, mul_off), ...) -> the cached (nkeys, 8) int64 device table (values depend on shapes only)."""
    return _cached(("ops", rows), device, lambda: np.asarray([list(r) + [0, 0, 0] for r in rows], np.int64), torch.int64)


def _run_table(x, rows, mask, S, status, reduce=True, apply=True):
    """moda_vis_minmax [+ moda_vis_apply] over the packed fp32 buffer x -> (mm (nkeys, 2), out or None)."""
    dev = x.device
    nkeys, max_n, total = len(rows), max(r[1] for r in rows), x.numel()
    ops = _op_table(tuple(rows), dev)
    margs = (None, 0, 1, 1) if mask is None else (L.ptr(mask), mask.shape[0], mask.shape[1], S)
    if reduce:
        mm = torch.empty((nkeys, 2), device=dev, dtype=torch.float32)
        part = torch.empty((nkeys, (max_n + TILE - 1) // TILE, 2), device=dev, dtype=torch.int32)
        L.call("moda_vis_minmax", L.ptr(x), total, L.ptr(ops), nkeys, max_n, *margs, L.ptr(part), L.ptr(mm), L.ptr(status), L.stream())
    else:
        mm = torch.zeros((nkeys, 2), device=dev, dtype=torch.float32)
    out = None
    if apply:
        out = torch.empty_like(x)
        L.call("moda_vis_apply", L.ptr(x), total, L.ptr(ops), nkeys, max_n, *margs, L.ptr(mm), L.ptr(out), L.stream())
    return mm, out


# ---- flow_to_image ------------------------------------------------------------------------------------------------------------
def color_wheel():
    """The 55-entry Middlebury wheel (Baker et al., "A Database and Evaluation Methodology for Optical Flow"): six ramps of
    15, 6, 4, 11, 13 and 6 steps between red, yellow, green, cyan, blue, magenta and red; one channel of a ramp is 255, one
    rises as floor(255 i / n) or falls as 255 - floor(255 i / n), one is 0.  (55, 3) float64."""
    ramps = ((15, 0, 1, +1), (6, 1, 0, -1), (4, 1, 2, +1), (11, 2, 1, -1), (13, 2, 0, +1), (6, 0, 2, -1))   # (n, full, moving, sign)
    rows = []
    for n, full, moving, sign in ramps:
        for i in range(n):
            c = [0.0, 0.0, 0.0]
            c[full] = 255.0
            c[moving] = float(255 * i // n) if sign > 0 else 255.0 - float(255 * i // n)
            rows.append(c)
    return np.asarray(rows, np.float64)


def flow_to_image(flow, f64_after_norm=True, status=None):
    """flowlib.flow_to_image for a batch: flow (N, H, W, 2 or more) fp32 (or one (H, W, C) frame) -> (N, H, W, 3) uint8.  The
    maximum radius is taken per frame; |u| or |v| > 1e7 is unknown flow and gives 0; NaN pixels give 0; channels past the second
    are ignored.  The caller's tensor is not written (the reference zeroes its unknown pixels).  f64_after_norm: see the
    module docstring.  Two launches for the maxima, one for the colours."""
    x = _f32("flow_to_image", flow)
    single = x.dim() == 3
    if single:
        x = x[None]
    if x.dim() != 4 or x.shape[-1] < 2 or min(x.shape) < 1:
        raise ValueError(f"flow_to_image: flow must be (N, H, W, C >= 2), got {tuple(flow.shape)}")
    N, H, W, Cn = (int(s) for s in x.shape)
    HW = H * W
    if N * HW * Cn >= 2 ** 31:
        raise ValueError(f"flow_to_image: {N * HW * Cn} floats, the limit is 2^31 - 1 a call")
    rows = tuple((i * HW * Cn, HW, Cn, OP_RAD, 0) for i in range(N))
    st = new_status(x.device) if status is None else status
    mm, _ = _run_table(x.reshape(-1), rows, None, 1, st, apply=False)
    maxrad = mm[:, 1].contiguous()
    wheel = _cached("wheel", x.device, color_wheel, torch.float32)
    out = torch.empty((N, H, W, 3), device=x.device, dtype=torch.uint8)
    L.call("moda_flow_color", L.ptr(x), N, HW, Cn, L.ptr(maxrad), L.ptr(wheel), 1 if f64_after_norm else 0, L.ptr(out), L.stream())
    return out[0] if single else out


# ---- canvases -----------------------------------------------------------------------------------------------------------------
def _get(src, name):
    return src.get(name) if isinstance(src, dict) else getattr(src, name, None)


def eval_canvases(rendered, model_or_tensors, opts, status=None):
    """train_utils.py:496-520 for one chunk of frames.  rendered: render_vid's dict, every key (hbs, S, S, C) with
    S == opts.render_size.  model_or_tensors: a model, or a dict, with the observations of the chunk as set_input leaves them --
    masks (bs, Sm, Sm), imgs (bs, 3, H, W), flow (bs, 2, H, W), occ (bs, H, W), dp_feats (bs, 16, h, w) and, for 'dpc', dps
    (bs, H, W) with dp_vis (n, 3); an observation that is missing leaves its key out.  -> (canvases, status): a new dict (the
    input's tensors are not written) with
      flo_coarse, img_loss_samp, pts_pred, feat_err, proj_err   *= the masks, nearest-resized to S (torch's legacy `nearest`:
                                              src = floor(dst * (float) Sm / S))
      pts_exp                                 *= sil_coarse
      feat_err, proj_err, frame_cyc_dis       *= 255 / max, the max taken after the masking
      unc_pred                                -= min; *= 255 / max
    gated by opts.use_embed / use_proj / use_unc as in the reference, normalised over the chunk; dis_reg and dis_reg_forward are
    dropped; img, sil, flo, dpc, occ, feat are the first hbs observed frames.  A maximum of 0 gives what IEEE gives (255 / 0 =
    inf, 0 * inf = NaN) and is counted in status[0]; a NaN makes its key's extremum NaN (status[1]).  Three launches for all
    keys together."""
    what = "eval_canvases"
    keys = [k for k in rendered if k not in ('dis_reg', 'dis_reg_forward')]
    if not keys:
        raise ValueError(f"{what}: nothing rendered")
    first = rendered[keys[0]]
    hbs, S = int(first.shape[0]), int(first.shape[1])
    if S != int(opts.render_size):
        raise ValueError(f"{what}: frames of {S} pixels, opts.render_size = {opts.render_size}")
    masks = _get(model_or_tensors, 'masks')
    if masks is None:
        raise ValueError(f"{what}: the observations hold no masks")
    if masks.dim() != 3 or masks.shape[1] != masks.shape[2] or masks.shape[0] < hbs:
        raise ValueError(f"{what}: masks must be (bs >= {hbs}, Sm, Sm), got {tuple(masks.shape)}")
    mask = _f32(what, masks)[:hbs]
    plan = [('flo_coarse', OP_MASK), ('img_loss_samp', OP_MASK), ('frame_cyc_dis', OP_SCALE255)]
    if getattr(opts, 'use_embed', False):
        plan += [('pts_pred', OP_MASK), ('pts_exp', OP_MUL), ('feat_err', OP_MASK | OP_SCALE255)]
    if getattr(opts, 'use_proj', False):
        plan += [('proj_err', OP_MASK | OP_SCALE255)]
    if getattr(opts, 'use_unc', False):
        plan += [('unc_pred', OP_SUBMIN | OP_SCALE255)]
    for k, _ in plan:
        if k not in rendered and k != 'frame_cyc_dis':
            raise KeyError(f"{what}: opts ask for '{k}', which was not rendered")
    plan = [(k, f) for k, f in plan if k in rendered]
    if any(f & OP_MUL for _, f in plan):
        if 'sil_coarse' not in rendered:
            raise KeyError(f"{what}: 'pts_exp' is multiplied by 'sil_coarse', which was not rendered")
        plan.append(('sil_coarse', 0))
    st = new_status(mask.device) if status is None else status
    out = {k: rendered[k] for k in keys}
    if plan:
        parts, rows, off = [], [], 0
        for k, f in plan:
            t = _f32(what, rendered[k])
            if t.dim() != 4 or tuple(t.shape[:3]) != (hbs, S, S):
                raise ValueError(f"{what}: '{k}' must be ({hbs}, {S}, {S}, C), got {tuple(t.shape)}")
            parts.append(t.reshape(-1))
            rows.append([off, t.numel(), int(t.shape[3]), f, 0])
            off += t.numel()
        if off >= 2 ** 31:
            raise ValueError(f"{what}: {off} floats in the chunk's canvases, the limit is 2^31 - 1 a call")
        sil_off = rows[-1][0]
        for r in rows:
            if r[3] & OP_MUL:
                r[4] = sil_off
        x = torch.cat(parts)
        _, y = _run_table(x, tuple(tuple(r) for r in rows), mask, S, st)
        for (k, f), r in zip(plan, rows):
            if f:
                out[k] = y[r[0]:r[0] + r[1]].view(rendered[k].shape)
    # the observed frames (:498-503), as the reference adds them
    obs = {n: _get(model_or_tensors, n) for n in ('imgs', 'flow', 'occ', 'dp_feats', 'dps', 'dp_vis')}
    if obs['imgs'] is not None:
        out['img'] = obs['imgs'].permute(0, 2, 3, 1)[:hbs]
    out['sil'] = masks[..., None][:hbs]
    if obs['flow'] is not None:
        out['flo'] = obs['flow'].permute(0, 2, 3, 1)[:hbs]
    if obs['dps'] is not None and obs['dp_vis'] is not None:
        out['dpc'] = obs['dp_vis'][obs['dps'].long()][:hbs]
    if obs['occ'] is not None:
        out['occ'] = obs['occ'][..., None][:hbs]
    if obs['dp_feats'] is not None:
        out['feat'] = obs['dp_feats'].std(1)[..., None][:hbs]
    return out, st


# ---- grid, display, video -----------------------------------------------------------------------------------------------------
def image_grid(img, row, col):
    """vis_utils.image_grid: img (N, h, w, c) -> (row h, col w, c), cell (i, j) holding img[i col + j].  One gather launch."""
    x = _f32("image_grid", img)
    if x.dim() != 4 or min(x.shape) < 1:
        raise ValueError(f"image_grid: img must be (N, h, w, c), got {tuple(img.shape)}")
    N, h, w, c = (int(s) for s in x.shape)
    row, col = int(row), int(col)
    if row < 1 or col < 1 or N < row * col:
        raise ValueError(f"image_grid: {N} frames for a {row} x {col} grid (the reference indexes img[i * col + j])")
    if row * h * col * w * c >= 2 ** 31:
        raise ValueError("image_grid: the collage holds 2^31 floats or more")
    out = torch.empty((row * h, col * w, c), device=x.device, dtype=torch.float32)
    L.call("moda_vis_grid", L.ptr(x), N, h, w, c, row, col, L.ptr(out), L.stream())
    return out


def to_display(tag, grid, status=None):
    """add_image (train_utils.py:1493-1504) up to what is handed to the log: a flow tag (FLOW_TAGS) -> flow_to_image's (H, W, 3)
    uint8; a scaled tag (SCALED_TAGS) -> (x - min) / (max - min), extrema over the whole grid; any other -> clamped to [0, 1]."""
    x = _f32("to_display", grid)
    if tag in FLOW_TAGS:
        return flow_to_image(x, status=status)
    if x.numel() < 1 or x.numel() >= 2 ** 31:
        raise ValueError(f"to_display: a grid of {x.numel()} elements")
    st = new_status(x.device) if status is None else status
    scaled = tag in SCALED_TAGS
    _, y = _run_table(x.reshape(-1), ((0, x.numel(), 1, OP_UNIT if scaled else OP_CLAMP01, 0),), None, 1, st, reduce=scaled)
    return y.view(x.shape)


def video_frames(frames, upsample_frame=150., is_flow=False, status=None):
    """save_vid (utils/io.py:242-258) up to the uint8 frame: frames (N, h, w[, c]) fp32 -> (int(upsample_frame), h, w[, c]) uint8
    (flow: (.., h, w, 3)).  Output frame i is input frame int(i / upsample_frame * N); upsample_frame < 1 stands for N.  Flow
    frames are coloured first.  A frame whose maximum is <= 1 is multiplied by 255 -- decided per frame on the device -- then
    converted by the rule of the module docstring.  The gif's cv2.resize and imageio stay outside."""
    x = _f32("video_frames", frames)
    if x.dim() < 2 or min(x.shape) < 1:
        raise ValueError(f"video_frames: frames must be (N, ...), got {tuple(frames.shape)}")
    if is_flow:
        x = flow_to_image(x, status=status).float()
    N = int(x.shape[0])
    E = x[0].numel()
    if N * E >= 2 ** 31:
        raise ValueError("video_frames: 2^31 values or more")
    if upsample_frame < 1:
        upsample_frame = N
    P = int(upsample_frame)
    if P * E >= 2 ** 31:
        raise ValueError("video_frames: 2^31 output values or more")
    pick = _cached(("pick", float(upsample_frame), N), x.device, lambda: [int(i / upsample_frame * N) for i in range(P)], torch.int32)
    st = new_status(x.device) if status is None else status
    mm, _ = _run_table(x.reshape(-1), tuple((i * E, E, 1, 0, 0) for i in range(N)), None, 1, st, apply=False)
    out = torch.empty((P,) + tuple(x.shape[1:]), device=x.device, dtype=torch.uint8)
    L.call("moda_vis_to_u8", L.ptr(x), N, E, L.ptr(pick), P, L.ptr(mm), L.ptr(out), L.ptr(st), L.stream())
    return out


# ---- rendering ----------------------------------------------------------------------------------------------------------------
def nerf_render_eval(model, rtk, kaug, embedid, ndepth=None, chunk=None):
    """banmo.nerf_render (moda.py:850-928) with self.training == False: prepare_ray_cams, sample_pxs over every pixel of every
    frame, render_rays over chunk_rays, the per-key concatenation viewed as (bs, S, S, -1) (zero-dimensional results stacked and
    averaged), and pts_pred / pts_exp mapped through (x - vis_min) / vis_len and clamped to [0, 1] -> (results, rand_inds).

    Read off `model`: opts (ndepth, chunk, perturb, noise_std, fine_steps, use_embed, and what sample_pxs reads), training
    (must be False), progress, img_size, nerf_models, embeddings, latest_vars['obj_bound'], vis_min / vis_len (use_embed), the
    batch as set_input leaves it -- dataid, frameid, frameid_sub, embedid, lineid, errid, imgs, masks, vis2d, flow, occ,
    dp_feats -- and what sample_pxs reads (near_far, pose_code, nerf_body_rts, ...).  As in the reference, model.frameid and
    model.errid are replaced by what sample_pxs returns.  `embedid` is accepted and unused, as there.  Nothing is read back."""
    from .feeders import chunk_rays
    from .geom_utils import prepare_ray_cams
    from .pixel_sampling import sample_pxs
    from .rendering import render_rays
    what = "nerf_render_eval"
    opts = model.opts
    _refuse_warps(what, model)
    if model.training:
        raise ValueError(f"{what}: the model is in training mode (nerf_render's training route is the training step's)")
    _no_grad(what, rtk, kaug)
    ndepth = int(opts.ndepth if ndepth is None else ndepth)
    chunk = int(opts.chunk if chunk is None else chunk)
    if chunk < 1:
        raise ValueError(f"{what}: chunk = {chunk}")
    S = int(model.img_size)
    with torch.no_grad():
        Rmat, Tmat, Kinv = prepare_ray_cams(rtk, kaug)
        bs = Kinv.shape[0]
        rand_inds, rays, frameid, errid = sample_pxs(model, bs, 256, Rmat, Tmat, Kinv, model.dataid, model.frameid, model.frameid_sub,
                                                     model.embedid, getattr(model, 'lineid', None), model.errid, model.imgs, model.masks,
                                                     model.vis2d, model.flow, model.occ, model.dp_feats)
        model.frameid, model.errid = frameid, errid                                  # moda.py:866-867
        # (the observations come back as permuted views, which chunk_rays cannot view as rows: one copy each, once a call)
        rays = {k: v.contiguous() if torch.is_tensor(v) else v for k, v in rays.items() if k not in _RAY_SKIP}
        n = rays['bs'] * rays['nsample']
        use_fine = model.progress > opts.fine_steps                                  # moda.py:879-883
        results = collections.defaultdict(list)
        for i in range(0, n, chunk):
            out = render_rays(model.nerf_models, model.embeddings, chunk_rays(rays, i, chunk), N_samples=ndepth, use_disp=False,
                              perturb=opts.perturb, noise_std=opts.noise_std, chunk=chunk, obj_bound=model.latest_vars['obj_bound'],
                              use_fine=use_fine, img_size=S, progress=model.progress, opts=opts)
            for k, v in out.items():
                if torch.is_tensor(v):
                    results[k].append(v)
        results = {k: torch.stack(v).mean() if v[0].dim() == 0 else torch.cat(v, 0).view(bs, S, S, -1) for k, v in results.items()}
        if getattr(opts, 'use_embed', False):                                        # moda.py:917-923
            dev = results['pts_pred'].device
            vmin = L.const_tensor(("vis_min", np.asarray(model.vis_min, np.float32).tobytes()), dev, lambda: np.asarray(model.vis_min, np.float32)[None])
            vlen = L.const_tensor(("vis_len", np.asarray(model.vis_len, np.float32).tobytes()), dev, lambda: np.asarray(model.vis_len, np.float32)[None])
            for k in ('pts_pred', 'pts_exp'):
                results[k] = ((results[k] - vmin) / vlen).clamp(0, 1)
    return results, rand_inds


def render_vid(model, ndepth=None, chunk=None):
    """v2s_trainer.render_vid (train_utils.py:1345-1362) after model.set_input(batch): nerf_render_eval on model.rtk, a clone of
    model.kaug and model.embedid, the four *_vis keys dropped, and the first bs // 2 rows of every key that has rows (the second
    half of the batch are the paired frames; zero-dimensional results are dropped)."""
    rendered, _ = nerf_render_eval(model, model.rtk, model.kaug.clone(), model.embedid, ndepth=ndepth, chunk=chunk)
    return {k: v[:v.shape[0] // 2] for k, v in rendered.items() if k not in VIS_KEYS and v.dim() > 0}


class EvalFrames:
    """What eval_frames returns: rendered_seq {key: (frames, S, S, C)}, concatenated over the chunks, and the status word."""

    def __init__(self, rendered_seq, status):
        self.rendered_seq, self.status = rendered_seq, status

    def grid(self, k, row=3, col=3):
        """add_image_grid's picture of key k: image_grid(., 3, 3) in its display form (to_display)."""
        return to_display(k, image_grid(self.rendered_seq[k], row, col), status=self.status)

    def video(self, k, upsample_frame=None):
        """save_vid's frames of key k as eval() asks for them: upsample_frame = min(30, frames)."""
        v = self.rendered_seq[k]
        return video_frames(v, min(30, len(v)) if upsample_frame is None else upsample_frame, is_flow=k in FLOW_TAGS, status=self.status)


def eval_frames(model, frames, set_input, ndepth=None, chunk=None):
    """The loop of eval() (train_utils.py:480-520) over chunks of opts.rnd_frame_chunk frames.  frames: the frame indices to
    render; set_input(model, idx_chunk): the caller's counterpart of evalloader.collate_fn + model.set_input, which leaves the
    chunk's batch (frames and their pairs) on the model.  Per chunk: render_vid, then eval_canvases on the chunk's observations.
    -> EvalFrames with rendered_seq concatenated per key.  The host reads nothing back inside the loop (nor after it)."""
    opts = model.opts
    _refuse_warps("eval_frames", model)
    step = int(opts.rnd_frame_chunk)
    if step < 1 or len(frames) < 1:
        raise ValueError(f"eval_frames: {len(frames)} frames in chunks of {step}")
    seq = collections.defaultdict(list)
    status = None
    for j in range(0, len(frames), step):
        idx = frames[j:j + step]
        set_input(model, idx)
        rendered = render_vid(model, ndepth=ndepth, chunk=chunk)
        rendered = {k: v[:len(idx)] for k, v in rendered.items()}
        status = new_status(model.masks.device) if status is None else status
        canv, _ = eval_canvases(rendered, model, opts, status=status)
        for k, v in canv.items():
            seq[k].append(v)
    return EvalFrames({k: torch.cat(v, 0) for k, v in seq.items()}, status)
