"""Camera tools, device-resident: what the reference does with the pose CNN's cameras after extract_cams, and its camera
yardstick.

  save_cams, fill_invalid_rotations   v2s_trainer.save_cams (nnutils/train_utils.py:744-791) without the files: rotations of
                                      rejected frames replaced by the closest valid frame's of the same video, translations
                                      scaled by obj_scale, the frame table's rt_raw and rotation rows written, each video's last
                                      row duplicated.  ONE launch (moda_cam_fill).
  align_sim3, eval_root, load_root    geom_utils.align_sim3 (nnutils/geom_utils.py:1463-1514) and scripts/eval/eval_root.py's
                                      main: mean-rotation / mean-scale alignment and the rotation error in degrees as max, median,
                                      mean and std.  ONE launch (moda_cam_sim3).
  visual_hull_align, align_sfm_sim3   geom_utils.py:1552-1608 and :1516-1550: prior cameras centred by voting G^3 lattice points
                                      against every view's silhouette.  Two launches (moda_cam_hull_vote, moda_cam_hull_apply).
  draw_cams, draw_cams_pair,          utils/io.py:147-153, :190-240: camera glyphs as one instancing launch after the launch
  render_root_txt                     that takes the median translation norm.

Seven HIP entries (include/moda_hip_cams.h, csrc/cams_kernels.hip).  Nothing is read back by any function here except
CamInit.save (and the host file helpers load_root / render_root_txt); every device function can be captured with
torch.cuda.graph after one eager warm-up call (which uploads the cached offset tables and glyph templates).  Inputs that require
grad raise NotImplementedError, CPU tensors RuntimeError, wrong shapes ValueError naming the argument.

Pinned and unpinned.  align_sim3, visual_hull_align, rtk_invert, rtk_compose and rot_angle are pinned to runs of the reference's
own functions (tests/golden/g40_cams.npz) through the float64 restatement tests/cams_numpy.py.  save_cams is a method of
v2s_trainer, which does not import without absl flags, the data loaders and cv2: it is RESTATED and unpinned (its fill rule is
tested against a literal transcription of the reference's loop).  eval_root.py's main and draw_cams are restated too.

Deviations from the reference, all deliberate:
  * align_sim3 does not modify its inputs (the reference writes rootlist_b and is_inlier in place): the aligned cameras and the
    inliers used are returned.  A NaN err_valid is never the fallback frame (np.argmin would take the first NaN).
  * scipy's Rotation.from_matrix first projects a matrix that is not orthogonal onto the nearest rotation (an SVD); that step is
    not restated: for fp32-rounded rotations it moves a quaternion entry by about 3e-9, far below fp32 resolution.
  * align_sim3's rotation errors are float64 up to the final fp32 value (the reference takes acos in fp32); their mean and std
    are float64 sums of those fp32 values; the median of an even count is the float64 mean of the two middle values.
  * visual_hull_align projects and samples in float64 from the reference's fp32 camera rows, bound and lattice (the reference
    stays fp32).  A non-finite sample coordinate contributes 0 and is counted in status[0]; an empty selection sets status[1] and
    leaves the translations unchanged (the reference returns NaN).  `bound` is a float64 sum rounded once, not torch's fp32 mean.
  * draw_cams' glyph is this module's own -- a box of side `radius` at the origin and three bars of length 5 radius and
    half-width 0.1 radius along x (red), y (green), z (blue): 32 vertices and 48 faces a camera, NOT trimesh.creation.axis'
    vertex counts.  `cool` and `gray` are the closed forms (x, 1 - x, 1) and (x, x, x), not matplotlib's 256-entry tables.
    draw_cams_pair's segments are boxes of half-width 0.001 (the reference: 5-sided cylinders of radius 0.001).
  * save_cams does not edit the data sets' rtklist (there are no files until CamInit.save).
Out of scope: process_so3_seq (it needs pydensecrf and the ScoreHead), editing the data sets' rtklist, lbs, any backward pass,
and eval_root.py's umeyama_alignment, which is dead code there."""
import glob
import os

import numpy as np
import torch

from . import _lib as L
from . import abi
from .mesh import TriMesh

C = abi.CAM_CONSTANTS
BLOCK = C["MODA_CAM_BLOCK"]
PART_FIELDS = C["MODA_CAM_PART_FIELDS"]
FIT_FIELDS = C["MODA_CAM_FIT_FIELDS"]
MAX_GRID = C["MODA_CAM_MAX_GRID"]
SIM3_STATUS = ("zero_norm", "fallback", "used", "sweeps")
HULL_STATUS = ("nonfinite", "empty", "selected", "reserved")
GLYPH_VERTS, GLYPH_FACES = 32, 48


# ---- argument checks: type, grad, shape, device -- in this order, so that every refusal can be met without a GPU --------------
def _arg(what, name, t, shape_txt, ok_shape, dtypes=None):
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: {name}: expected a tensor, got {type(t).__name__}")
    if t.requires_grad:
        raise NotImplementedError(f"{what}: inputs that require grad are not implemented (the camera tools have no backward); "
                                  "pass them detached")
    if not ok_shape(tuple(t.shape)) or (dtypes is not None and t.dtype not in dtypes):
        raise ValueError(f"{what}: {name} must be {shape_txt}, got {t.dtype} {tuple(t.shape)}")
    return t


def _on_device(what, *tensors):
    """After every argument's shape has been checked: CPU tensors are refused."""
    if any(t is not None and not t.is_cuda for t in tensors):
        raise RuntimeError(f"{what} takes CUDA (ROCm) tensors; the HIP library is the only compute path")


def _cams(what, name, t, n=None, at_least=False):
    ok = lambda s: len(s) == 3 and s[1:] == (4, 4) and s[0] >= 1 and (n is None or (s[0] >= n if at_least else s[0] == n))
    txt = "(n, 4, 4)" if n is None else (f"(>= {n}, 4, 4)" if at_least else f"({n}, 4, 4)")
    return _arg(what, name, t, txt, ok)


def _flags(what, name, t, n):
    t = _arg(what, name, t, f"({n},) bool or uint8", lambda s: s == (n,), (torch.bool, torch.uint8))
    return t.contiguous().view(torch.uint8)


_OFFSETS = {}


def _offsets(what, name, off, total, device):
    """(n_videos + 1,) offsets -> (device int32 table, host tuple | None).  Host data (a sequence, numpy, a CPU tensor) is checked
    and uploaded once per distinct tuple; a device tensor is taken as it is (the kernel skips a video whose range is not inside
    the table)."""
    if torch.is_tensor(off) and off.is_cuda:
        if off.dim() != 1 or off.shape[0] < 2 or off.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{what}: {name} must be (n_videos + 1,) int, got {off.dtype} {tuple(off.shape)}")
        return off.to(torch.int32).contiguous(), None
    host = tuple(int(v) for v in (off.tolist() if hasattr(off, "tolist") else off))
    if len(host) < 2 or host[0] != 0 or any(b < a for a, b in zip(host, host[1:])) or (total is not None and host[-1] != total):
        raise ValueError(f"{what}: {name} = {host}: expected non-decreasing offsets from 0 to {total}")
    if device is None:                                                           # the checks only
        return None, host
    key = (host, str(device))
    t = _OFFSETS.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{what}: a new {name} is uploaded from the host -- call once before capture")
        t = _OFFSETS[key] = torch.tensor(host, dtype=torch.int32).to(device)
    return t, host


# ---- save_cams ----------------------------------------------------------------------------------------------------------------
class CamInit:
    """What save_cams returns: rtk (N,4,4) fp32 with the filled rotations and scaled translations, src (N,) int32 (the frame each
    rotation came from), n_valid (n_videos,) int32, rows (N,) int32 (each frame's row in the frame table); device tensors."""

    def __init__(self, rtk, src, n_valid, rows, frame_offset):
        self.rtk, self.src, self.n_valid, self.rows, self.frame_offset = rtk, src, n_valid, rows, frame_offset

    def save(self, prefix, seqnames, frame_numbers=None):
        """The reference's files (train_utils.py:766-768, :778-782): `<prefix>/<seq>-%05d.txt` per frame in np.savetxt's default
        format, and each video's last camera a second time under the next number.  seqnames: one name a video; frame_numbers
        (N,): the number in each frame's file name (None: its index inside the video).  The one read-back of this module.
        -> the paths written."""
        rtk = self.rtk.detach().cpu().numpy()
        off = [int(v) for v in self.frame_offset.cpu().tolist()]
        if len(seqnames) != len(off) - 1:
            raise ValueError(f"CamInit.save: {len(seqnames)} names for {len(off) - 1} videos")
        if frame_numbers is not None and len(frame_numbers) != len(rtk):
            raise ValueError(f"CamInit.save: {len(frame_numbers)} frame numbers for {len(rtk)} frames")
        os.makedirs(prefix, exist_ok=True)
        paths = []
        for v, name in enumerate(seqnames):
            for i in range(off[v], off[v + 1]):
                idx = i - off[v] if frame_numbers is None else int(frame_numbers[i])
                for number in (idx, idx + 1) if i == off[v + 1] - 1 else (idx,):
                    paths.append('%s/%s-%05d.txt' % (prefix, name, number))
                    np.savetxt(paths[-1], rtk[i])
        return paths


def _fill(what, rtk, is_valid, offs, fill, scale, state=None):
    N = rtk.shape[0]
    dev = rtk.device
    nv = offs.shape[0] - 1
    out = torch.empty_like(rtk)
    src = torch.empty((N,), device=dev, dtype=torch.int32)
    n_valid = torch.zeros((nv,), device=dev, dtype=torch.int32)
    rows = torch.empty((N,), device=dev, dtype=torch.int32)
    tabs = (None, None, 0) if state is None else (L.ptr(state.rtk), L.ptr(state.rt_raw), state.num_frames)
    L.call("moda_cam_fill", L.ptr(rtk), L.ptr(is_valid), L.ptr(offs), nv, N, 1 if fill else 0, float(scale), L.ptr(out), L.ptr(src),
           L.ptr(n_valid), L.ptr(rows), *tabs, L.stream())
    return out, src, n_valid, rows


def fill_invalid_rotations(rtk, is_valid, frame_offset):
    """The unc_filter block of save_cams (train_utils.py:752-761): rtk (N,4,4), is_valid (N,) bool, frame_offset (n_videos + 1,)
    int, video v holding frames [frame_offset[v], frame_offset[v+1]) -> (rtk_filled (N,4,4), src (N,) int32).  An invalid frame i
    of a video with a valid frame takes the rotation of the valid frame j of that video that minimises |i - j| (the lower j on a
    tie, np.argmin's choice); valid frames and videos without a valid frame are untouched; src[i] is the frame the rotation came
    from, or i.  One launch; a video may be of any length."""
    what = "fill_invalid_rotations"
    r = _cams(what, "rtk", rtk)
    N = r.shape[0]
    val = _flags(what, "is_valid", is_valid, N)
    if not (torch.is_tensor(frame_offset) and frame_offset.is_cuda):
        _offsets(what, "frame_offset", frame_offset, N, None)
    _on_device(what, r, val)
    offs, _ = _offsets(what, "frame_offset", frame_offset, N, r.device)
    out, src, _, _ = _fill(what, L.dev(r), val, offs, True, 1.0)
    return out, src


def save_cams(rtk, is_valid, data_offset, obj_scale, state, *, unc_filter=True):
    """v2s_trainer.save_cams (train_utils.py:744-791) without the files, restated (see the module docstring): rtk (N,4,4) and
    is_valid (N,) as extract_cams returns them, data_offset (n_videos + 1,) the frame TABLE's offsets (what
    loss_utils.compute_root_sm_2nd_loss takes): video v has n_v table rows and n_v - 1 evaluated frames, N = data_offset[-1] -
    n_videos.  In order: the rotations are filled (unc_filter), t *= obj_scale, state.rt_raw[row] = rtk[:3,:4] and
    state.rtk[row,:3,:3] = R (the table's translation and K row stay), and each video's last evaluated frame is written a second
    time into the video's last table row.  state: a FrameState with data_offset[-1] frames, updated in place.  -> CamInit.  One
    launch."""
    from .frame_state import FrameState
    what = "save_cams"
    r = _cams(what, "rtk", rtk)
    N = r.shape[0]
    val = _flags(what, "is_valid", is_valid, N)
    if not isinstance(state, FrameState):
        raise TypeError(f"{what}: state must be a moda_amd.FrameState, got {type(state).__name__}")
    _on_device(what, r, val)
    r = L.dev(r)
    doff, host = _offsets(what, "data_offset", data_offset, None, r.device)
    nv = doff.shape[0] - 1
    if host is not None:
        if host[-1] - nv != N or any(b - a < 1 for a, b in zip(host, host[1:])) or host[-1] != state.num_frames:
            raise ValueError(f"{what}: data_offset = {host} describes {host[-1] - nv} evaluated frames in a table of {host[-1]} rows; "
                             f"rtk holds {N} and state {state.num_frames}")
        offs, _ = _offsets(what, "data_offset", tuple(o - v for v, o in enumerate(host)), N, r.device)
    else:
        offs = doff - torch.arange(nv + 1, device=r.device, dtype=torch.int32)
    out, src, n_valid, rows = _fill(what, r, val, offs, unc_filter, obj_scale, state)
    return CamInit(out, src, n_valid, rows, offs)


# ---- align_sim3 ---------------------------------------------------------------------------------------------------------------
class Sim3Fit:
    """align_sim3's fit, device tensors: rotation (3,3) float64 (the mean of Rb^T Ra), scale () float64 (the mean of |ta| / |tb|),
    so3_err (n,) fp32 degrees, stats (4,) float64 = max, median, mean, unbiased std of so3_err, inlier_used (n,) bool, status (4,)
    int32 = [frames with a zero-norm second translation, 1 when no inlier was given and the fallback frame was taken, frames used,
    Jacobi sweeps], eig (2,) float64: the two largest eigenvalues of sum q q^T (their gap says how well the mean is defined)."""

    def __init__(self, fit, so3_err, stats, inlier_used, status):
        self.rotation, self.scale, self.eig = fit[:9].view(3, 3), fit[9], fit[10:12]
        self.so3_err, self.stats, self.inlier_used, self.status = so3_err, stats, inlier_used, status


def align_sim3(rootlist_a, rootlist_b, is_inlier=None, err_valid=None):
    """geom_utils.align_sim3: rootlist_a, rootlist_b (n,4,4); is_inlier (n,) bool and err_valid (n,) select the frames the fit
    uses (None: all; no inlier set: the frame of smallest err_valid) -> (rootlist_b_aligned (n,4,4), Sim3Fit).  Rb' = Rb mean(Rb^T
    Ra) with scipy's Rotation.mean, tb' = tb mean(|ta| / |tb|).  The inputs are not modified.  One launch."""
    what = "align_sim3"
    a = _cams(what, "rootlist_a", rootlist_a)
    n = a.shape[0]
    b = _cams(what, "rootlist_b", rootlist_b, n)
    inl = err = None
    if is_inlier is not None:
        if err_valid is None:
            raise ValueError(f"{what}: err_valid must be given with is_inlier (it chooses the frame when no inlier is set)")
        inl = _flags(what, "is_inlier", is_inlier, n)
        err = _arg(what, "err_valid", err_valid, f"({n},)", lambda s: s == (n,))
    _on_device(what, a, b, inl, err)
    a, b, err = L.dev(a), L.dev(b), None if err is None else L.dev(err)
    dev = a.device
    out = torch.empty_like(b)
    fit = torch.empty((FIT_FIELDS,), device=dev, dtype=torch.float64)
    so3 = torch.empty((n,), device=dev, dtype=torch.float32)
    stats = torch.empty((4,), device=dev, dtype=torch.float64)
    used = torch.empty((n,), device=dev, dtype=torch.uint8)
    status = torch.empty((4,), device=dev, dtype=torch.int32)
    L.call("moda_cam_sim3", L.ptr(a), L.ptr(b), L.ptr(inl), L.ptr(err), n, L.ptr(out), L.ptr(fit), L.ptr(so3), L.ptr(stats),
           L.ptr(used), L.ptr(status), L.stream())
    return out, Sim3Fit(fit, so3, stats, used.view(torch.bool), status)


def load_root(root_dir, cap_frame):
    """utils/io.py:173-188, a host function: every `<root_dir>*.txt` in sorted order (the first cap_frame of them when
    cap_frame > 0) through np.loadtxt -> (n,4,4) float64 numpy."""
    paths = sorted(glob.glob('%s*.txt' % root_dir))
    if cap_frame > 0:
        paths = paths[:cap_frame]
    return np.asarray([np.loadtxt(p) for p in paths])


def eval_root(rootlist_a, rootlist_b):
    """scripts/eval/eval_root.py's main without the file reading: -> (aligned_b, Sim3Fit, TriMesh), the mesh being
    draw_cams(rootlist_a, color='gray') concatenated with draw_cams(aligned_b)."""
    aligned, fit = align_sim3(rootlist_a, rootlist_b)
    return aligned, fit, concatenate([draw_cams(rootlist_a, color='gray'), draw_cams(aligned)])


# ---- visual hull --------------------------------------------------------------------------------------------------------------
def visual_hull_align(rtk, kaug, masks, *, grid_size=64, return_scores=False):
    """geom_utils.visual_hull_align: rtk (>= V,4,4) (trimmed to V rows, as there), kaug (V,4), masks (V,h,w) fp32, uint8 or bool
    -> (rtk_out (V,4,4), status (4,) int32[, scores (grid_size^3,) fp32]).  grid_size^3 lattice points in [-bound, bound]^3,
    bound = the mean of |(-R^T t)| over all 3 V entries, are projected into every view (obj_to_cam, pinhole_cam with
    mat2K(K2inv(kaug) K2mat(rtk[:,3])), the 1e-6 + z kept) and sample its mask (grid_sample: bilinear, align_corners=False, zero
    padding); a point whose summed score exceeds 0.8 V is selected, and t_out = -R (c - centre) with c = -R^T t and centre the
    mean of the selected points.  status = [non-finite samples, 1 when nothing was selected (translations unchanged), points
    selected, 0].  Two launches."""
    what = "visual_hull_align"
    if not torch.is_tensor(masks):
        raise TypeError(f"{what}: masks: expected a tensor, got {type(masks).__name__}")
    m = _arg(what, "masks", masks, "(V, h, w) fp32, uint8 or bool", lambda s: len(s) == 3 and min(s) >= 1,
             (torch.float32, torch.uint8, torch.bool))
    V, h, w = (int(s) for s in m.shape)
    r = _cams(what, "rtk", rtk, V, at_least=True)
    k = _arg(what, "kaug", kaug, f"({V}, 4)", lambda s: s == (V, 4))
    G = int(grid_size)
    if G < 2 or G > MAX_GRID:
        raise ValueError(f"{what}: grid_size = {grid_size}, expected 2..{MAX_GRID}")
    _on_device(what, m, r, k)
    r, k = L.dev(r)[:V].contiguous(), L.dev(k)
    m = m.contiguous()
    u8 = m.dtype != torch.float32
    if u8:
        m = m.view(torch.uint8)
    dev = r.device
    P = G ** 3
    nparts = (P + BLOCK - 1) // BLOCK
    part = torch.empty((nparts, PART_FIELDS), device=dev, dtype=torch.float64)
    scores = torch.empty((P,), device=dev, dtype=torch.float32) if return_scores else None
    out = torch.empty_like(r)
    status = torch.empty((4,), device=dev, dtype=torch.int32)
    L.call("moda_cam_hull_vote", L.ptr(r), L.ptr(k), L.ptr(m), 1 if u8 else 0, V, h, w, G, L.ptr(scores), L.ptr(part), L.stream())
    L.call("moda_cam_hull_apply", L.ptr(r), V, G, L.ptr(part), L.ptr(out), L.ptr(status), L.stream())
    return (out, status, scores) if return_scores else (out, status)


def align_sfm_sim3(rtk_pred, is_valid, err_valid, kaug, masks, roots_sfm, frame_offset):
    """geom_utils.align_sfm_sim3 (:1516-1550): for every video v with prior cameras roots_sfm[v] ((>= n_v,4,4); None for the
    others) the chain visual_hull_align(roots_sfm[v], kaug_v, masks_v) -> align_sim3(rtk_pred_v, ., is_inlier=is_valid_v,
    err_valid=err_valid_v) replaces the video's predicted cameras and marks them all valid.  frame_offset (n_videos + 1,): host
    integers.  -> new (rtk, is_valid) tensors; the inputs are not modified."""
    what = "align_sfm_sim3"
    r = _cams(what, "rtk_pred", rtk_pred)
    N = r.shape[0]
    val = _arg(what, "is_valid", is_valid, f"({N},) bool", lambda s: s == (N,), (torch.bool,))
    err = _arg(what, "err_valid", err_valid, f"({N},)", lambda s: s == (N,))
    if torch.is_tensor(frame_offset) and frame_offset.is_cuda:
        raise ValueError(f"{what}: frame_offset must be host integers (the loop over the videos runs on the host)")
    off = tuple(int(v) for v in (frame_offset.tolist() if hasattr(frame_offset, "tolist") else frame_offset))
    if len(off) < 2 or off[0] != 0 or off[-1] != N or any(b < a for a, b in zip(off, off[1:])):
        raise ValueError(f"{what}: frame_offset = {off}: expected non-decreasing offsets from 0 to {N}")
    if len(roots_sfm) != len(off) - 1:
        raise ValueError(f"{what}: roots_sfm holds {len(roots_sfm)} entries for {len(off) - 1} videos")
    _on_device(what, r, val, err)
    r = L.dev(r)
    out, valid = r.clone(), val.clone()
    for v, prior in enumerate(roots_sfm):
        if prior is None or off[v + 1] == off[v]:
            continue
        sl = slice(off[v], off[v + 1])
        centred = visual_hull_align(prior, kaug[sl], masks[sl])[0]
        out[sl] = align_sim3(r[sl], centred, is_inlier=val[sl], err_valid=err[sl])[0]
        valid[sl] = True
    return out, valid


# ---- glyphs -------------------------------------------------------------------------------------------------------------------
_BOX_FACES = np.asarray([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                         [1, 5, 7], [1, 7, 3]], np.int64)


def _box(lo, hi):
    """The 8 corners of [lo, hi] (corner 4 a + 2 b + c takes hi's x, y, z where a, b, c are set) and its 12 outward triangles."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.asarray([[(hi if a else lo)[0], (hi if b else lo)[1], (hi if c else lo)[2]] for a in (0, 1) for b in (0, 1) for c in (0, 1)])
    return v, _BOX_FACES


def camera_glyph(axis=True):
    """The unit glyph (in units of the radius): a box of side 1 at the origin and, with axis, three bars of length 5 and
    half-width 0.1 along x, y, z -> (vertices (32|8, 3) float64, faces (48|12, 3) int64, part (32|8,) int: 0 box, 1..3 bars)."""
    parts = [_box([-.5, -.5, -.5], [.5, .5, .5])]
    if axis:
        for a in range(3):
            lo, hi = np.full(3, -0.1), np.full(3, 0.1)
            lo[a], hi[a] = 0.0, 5.0
            parts.append(_box(lo, hi))
    verts = np.concatenate([p[0] for p in parts])
    faces = np.concatenate([p[1] + 8 * i for i, p in enumerate(parts)])
    return verts, faces, np.repeat(np.arange(len(parts)), 8)


def colormap(color, x):
    """'cool' -> (x, 1 - x, 1), 'gray' -> (x, x, x), x clipped to [0, 1] -> (n, 4) uint8 RGBA (floor(255 c + 0.5), alpha 255)."""
    x = np.clip(np.asarray(x, np.float64).reshape(-1), 0.0, 1.0)
    if color == 'cool':
        rgb = np.stack([x, 1.0 - x, np.ones_like(x)], -1)
    elif color == 'gray':
        rgb = np.stack([x, x, x], -1)
    else:
        raise ValueError(f"draw_cams: color = {color!r}: 'cool' and 'gray' are implemented")
    return np.concatenate([np.floor(255.0 * rgb + 0.5), np.full((len(x), 1), 255.0)], -1).astype(np.uint8)


_AXIS_COLORS = np.asarray([[255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 255, 255]], np.uint8)


def _mesh(verts, faces, colors):
    m = TriMesh(verts, faces)
    m.visual.vertex_colors = colors
    return m


def concatenate(meshes):
    """trimesh.util.concatenate for TriMesh: vertices and colours appended, faces offset; device tensors stay on the device."""
    offs = np.cumsum([0] + [int(m.vertices_t.shape[0]) for m in meshes])
    verts = torch.cat([m.vertices_t for m in meshes])
    faces = torch.cat([m.faces_t + int(o) for m, o in zip(meshes, offs)])
    return _mesh(verts, faces, np.concatenate([m.visual.vertex_colors for m in meshes]))


def draw_cams(all_cam, color='cool', axis=True, color_list=None):
    """utils/io.py:190-223: all_cam (n,4,4) device tensor -> a TriMesh of n glyphs, glyph j at the camera centre -R^T t with
    orientation R^T, of radius 0.02 times the median of the non-zero translation norms (NaN vertices when every translation is
    0, as the reference's median of nothing).  color_list: host numbers in [0, 1], one a camera (None: j / n); the origin box
    takes colormap(color, color_list[j]), the bars red, green, blue.  Two launches: the median, the instances."""
    what = "draw_cams"
    cams = _cams(what, "all_cam", all_cam)
    _on_device(what, cams)
    cams = L.dev(cams)
    n = cams.shape[0]
    dev = cams.device
    tv, tf, part = camera_glyph(axis)
    Nv = len(tv)
    tmpl = L.const_tensor(("cam_glyph", bool(axis)), dev, lambda: tv.astype(np.float32))
    key = ("cam_glyph_faces", bool(axis), n, str(dev))
    faces = L._CONST.get(key)
    if faces is None:
        faces = L._CONST[key] = torch.as_tensor((tf[None] + Nv * np.arange(n)[:, None, None]).reshape(-1, 3).astype(np.int32)).to(dev)
    x = np.arange(n) / float(n) if color_list is None else np.asarray(color_list, np.float64).reshape(-1)
    if len(x) != n:
        raise ValueError(f"{what}: color_list holds {len(x)} entries for {n} cameras")
    colors = np.where((part == 0)[None, :, None], colormap(color, x)[:, None], _AXIS_COLORS[np.maximum(part, 1) - 1][None])
    work = torch.empty((n,), device=dev, dtype=torch.float32)
    med = torch.empty((1,), device=dev, dtype=torch.float32)
    verts = torch.empty((n * Nv, 3), device=dev, dtype=torch.float32)
    L.call("moda_cam_tnorm_median", L.ptr(cams), n, L.ptr(work), L.ptr(med), L.stream())
    L.call("moda_cam_glyphs", L.ptr(cams), n, L.ptr(tmpl), Nv, L.ptr(med), 0.02, L.ptr(verts), L.stream())
    return _mesh(verts, faces, colors.reshape(-1, 4))


def draw_cams_pair(cam1, cam2, color='cool', axis=True, color_list=None):
    """utils/io.py:225-240 -> (mesh of cam1, mesh of cam2, lines): one thin box per pair between the two camera centres."""
    what = "draw_cams_pair"
    c1 = _cams(what, "cam1", cam1)
    n = c1.shape[0]
    c2 = _cams(what, "cam2", cam2, n)
    _on_device(what, c1, c2)
    c1, c2 = L.dev(c1), L.dev(c2)
    out = torch.empty((n * 8, 3), device=c1.device, dtype=torch.float32)
    L.call("moda_cam_links", L.ptr(c1), L.ptr(c2), n, 0.001, L.ptr(out), L.stream())
    key = ("cam_link_faces", n, str(c1.device))
    faces = L._CONST.get(key)
    if faces is None:
        faces = L._CONST[key] = torch.as_tensor((_BOX_FACES[None] + 8 * np.arange(n)[:, None, None]).reshape(-1, 3).astype(np.int32)).to(c1.device)
    lines = _mesh(out, faces, np.tile(np.asarray([[102, 102, 102, 255]], np.uint8), (n * 8, 1)))
    return draw_cams(c1, color, axis, color_list), draw_cams(c2, color, axis, color_list), lines


def render_root_txt(cam_dir, cap_frame, device='cuda'):
    """utils/io.py:147-153: load_root, draw_cams, and the mesh written as `<dir>/mesh-<seqname>.obj` -> the path."""
    from .animate import write_obj
    camlist = load_root(cam_dir, cap_frame)
    if camlist.ndim != 3:
        raise ValueError(f"render_root_txt: no cameras under {cam_dir}*.txt")
    mesh = draw_cams(torch.as_tensor(camlist, dtype=torch.float32).to(device))
    save_dir, seqname = cam_dir.rsplit('/', 1)
    path = '%s/mesh-%s.obj' % (save_dir, seqname)
    write_obj(path, mesh.vertices, mesh.faces, mesh.visual.vertex_colors)
    return path
