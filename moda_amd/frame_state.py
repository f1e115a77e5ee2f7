"""The per-frame tables of a training run, device-resident: the reference's `latest_vars` (nnutils/moda.py:339-350), what
banmo.save_latest_vars writes into it every step (moda.py:1497-1513), the near-far reset of forward_default (moda.py:485-491) and
get_near_far (nnutils/geom_utils.py:1105-1135) with its callers reset_nf (nnutils/train_utils.py:826-843) and the obj_bound line
of reset_hparams (:1102-1104).  The scatter and the planes are one HIP launch each (moda_frames_scatter, moda_near_far,
csrc/frames_kernels.hip; two launches where the points of a frame are split over workgroups); nothing is read back, so the
chain compute_rts -> near_far -> rays can be captured.

`FrameState` is also the compatibility view of `latest_vars`: `model.latest_vars = state` keeps mesh.extract_mesh and
feeders.reinit_bones working.  Reading an array key ('rtk', 'rt_raw', 'idk') copies the table to the host -- ONE
synchronisation per read -- and returns a numpy COPY: writing into that copy does not reach the device (assign the whole array,
`state['rtk'] = a`, or use save_latest_vars).

Deviations from the reference, all deliberate:
  * Bad input does not raise inside a step: a frame id outside the tables is not written and counted in status[1], a frame
    given a NaN plane is counted in status[0]; `FrameState.check()` reads the counts back (a synchronisation) and raises.
  * Tensors that require grad are refused (the reference detaches everywhere here): pass `rtk_all.detach()`.
  * `pts=None` restates trimesh.bounds.corners as the 8 corners of mesh_rest.bounds; an empty mesh raises ValueError.
"""
import itertools

import numpy as np
import torch

from . import _lib as L
from . import abi

ARRAY_KEYS = ('rtk', 'rt_raw', 'idk')
HOST_KEYS = ('obj_bound', 'mesh_rest')
_SHAPES = {'rtk': (4, 4), 'rt_raw': (3, 4), 'idk': ()}
MAX_SPLIT = abi.CONSTANTS["MODA_NEAR_FAR_MAX_SPLIT"]
SMALL_N = 32                # up to this many points a frame is one lane's loop


def _no_grad(what, *tensors):
    if any(torch.is_tensor(t) and t.requires_grad for t in tensors):
        raise NotImplementedError(f"{what}: inputs that require grad are not implemented (the frame tables have no backward "
                                  "kernel; the reference detaches here); pass them detached")


def _table(t, shape, what):
    """A table the kernels update IN PLACE: it must already be a contiguous fp32 device tensor of `shape`."""
    if isinstance(t, torch.nn.Parameter):
        t = t.data                                                      # the reference writes model.near_far.data
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{what} must be a CUDA (ROCm) tensor; the HIP library is the only compute path")
    if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} is updated in place: it must be contiguous fp32 of shape {tuple(shape)}, got {t.dtype} "
                         f"{tuple(t.shape)}, contiguous={t.is_contiguous()}")
    return t


def box_corners(bounds):
    """bounds (2,3) -> the 8 corners (8,3) float64 (trimesh.bounds.corners; their order does not matter to a min / max)."""
    b = np.asarray(bounds, np.float64).reshape(2, 3)
    return np.asarray([[b[i, 0], b[j, 1], b[k, 2]] for i, j, k in itertools.product((0, 1), repeat=3)])


class FrameState:
    """The device tables rtk (M,4,4), rt_raw (M,3,4), idk (M,), near_far (M,2) (fp32) and the host values obj_bound, mesh_rest.
    `near_far` may be the model's own tensor (a Parameter's `.data` is taken): the planes are then updated where the rays read
    them.  status: device int32 [#frames given a NaN plane, #frame ids refused, 0, 0]."""

    def __init__(self, num_frames, device='cuda', near_far=None):
        M = int(num_frames)
        if M < 1:
            raise ValueError(f"FrameState: {num_frames} frames")
        self.num_frames = M
        self.device = torch.device(device) if near_far is None else (near_far.data if isinstance(near_far, torch.nn.Parameter) else near_far).device
        z = lambda *s: torch.zeros(s, device=self.device, dtype=torch.float32)
        self.rtk, self.rt_raw, self.idk = z(M, 4, 4), z(M, 3, 4), z(M)
        self.near_far = z(M, 2) if near_far is None else _table(near_far, (M, 2), "FrameState: near_far")
        self.status = torch.zeros((4,), device=self.device, dtype=torch.int32)
        self.obj_bound = None
        self._mesh_rest = None
        self._box = None
        self._ws = None
        self._dtypes = {k: np.dtype(np.float32) for k in ARRAY_KEYS}
        self.extra = {}                                                 # any other key of a loaded dict (sil_err, fp_err, ...), kept as is

    # ---- the dict view ------------------------------------------------------------------------------------------------
    @property
    def mesh_rest(self):
        return self._mesh_rest

    @mesh_rest.setter
    def mesh_rest(self, mesh):
        self._mesh_rest, self._box = mesh, None

    def __contains__(self, key):
        if key in ARRAY_KEYS:
            return True
        if key in HOST_KEYS:
            return getattr(self, key) is not None
        return key in self.extra

    def __getitem__(self, key):
        if key in ARRAY_KEYS:
            return getattr(self, key).detach().cpu().numpy().astype(self._dtypes[key])       # one synchronisation; a copy
        if key in HOST_KEYS:
            v = getattr(self, key)
            if v is None:
                raise KeyError(key)
            return v
        return self.extra[key]

    def __setitem__(self, key, value):
        if key in ARRAY_KEYS:
            a = np.asarray(value)
            shape = (self.num_frames,) + _SHAPES[key]
            if a.shape != shape:
                raise ValueError(f"FrameState['{key}']: expected shape {shape}, got {a.shape}")
            self._dtypes[key] = a.dtype if a.dtype.kind == 'f' else np.dtype(np.float64)
            getattr(self, key).copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
        elif key in HOST_KEYS:
            setattr(self, key, value)
        else:
            self.extra[key] = value

    @classmethod
    def from_vars(cls, vars_dict, near_far=None, device='cuda'):
        """A dict as checkpoint.load_vars returns it -> FrameState (one upload per table)."""
        M = np.asarray(vars_dict['rtk']).shape[0]
        s = cls(M, device, near_far)
        for k, v in vars_dict.items():
            s[k] = v
        return s

    def as_vars(self):
        """-> the dict format of checkpoint.load_vars / np.save (three synchronising copies)."""
        out = {k: self[k] for k in ARRAY_KEYS}
        out.update({k: getattr(self, k) for k in HOST_KEYS if getattr(self, k) is not None})
        out.update(self.extra)
        return out

    # ---- helpers of the launches -------------------------------------------------------------------------------------
    def box(self):
        """The 8 corners of mesh_rest's bounds on the device, uploaded once per mesh (not inside a capture)."""
        if self._box is None:
            if self._mesh_rest is None:
                raise ValueError("get_near_far: pts=None needs latest_vars['mesh_rest']")
            bounds = self._mesh_rest.bounds
            if bounds is None or len(self._mesh_rest.vertices) == 0:
                raise ValueError("get_near_far: mesh_rest is empty, it has no bounds")
            self._box = torch.from_numpy(box_corners(bounds).astype(np.float32)).to(self.device)
        return self._box

    def workspace(self, splits):
        n = self.num_frames * int(splits) * 3
        if self._ws is None or self._ws.numel() < n:
            self._ws = torch.empty((n,), device=self.device, dtype=torch.float32)
        return self._ws

    def check(self):
        """Read `status` back (a synchronisation), zero it, and raise RuntimeError naming what was refused since the last check."""
        s = self.status.cpu().tolist()
        self.status.zero_()
        bad = []
        if s[1]:
            bad.append(f"{s[1]} frame id(s) outside [0, {self.num_frames}) were not written (save_latest_vars)")
        if s[0]:
            bad.append(f"{s[0]} frame(s) were given NaN near / far planes (a NaN or infinite point or pose row)")
        if bad:
            raise RuntimeError("FrameState.check: " + "; ".join(bad))


def _state_of(model, what):
    state = getattr(getattr(model, "module", model), "latest_vars", None)
    if not isinstance(state, FrameState):
        raise TypeError(f"{what}: model.latest_vars must be a moda_amd.FrameState (FrameState.from_vars(dict, model.near_far) "
                        "makes one of the reference's dict)")
    return state


def save_latest_vars(model):
    """banmo.save_latest_vars (moda.py:1497-1513) in one launch: model.rtk (bs,4,4) with row 3 composed with model.kaug (bs,4),
    model.rt_raw (bs,3,4) and idk = 1 into model.latest_vars (a FrameState) at model.frameid; a frame named twice keeps the
    last occurrence, as numpy's fancy assignment does."""
    model = getattr(model, "module", model)
    state = _state_of(model, "save_latest_vars")
    _no_grad("save_latest_vars", model.kaug, model.frameid)
    rtk = L.dev(model.rtk.detach()).reshape(-1, 4, 4)                   # (the reference: self.rtk.clone().detach())
    bs = rtk.shape[0]
    kaug, rt_raw = L.dev(model.kaug).reshape(-1, 4), L.dev(model.rt_raw.detach()).reshape(-1, 3, 4)
    fid = L.dev(model.frameid, torch.int64).reshape(-1)
    if kaug.shape[0] != bs or rt_raw.shape[0] != bs or fid.shape[0] != bs:
        raise ValueError(f"save_latest_vars: rtk, kaug, rt_raw, frameid hold {bs}, {kaug.shape[0]}, {rt_raw.shape[0]}, {fid.shape[0]} entries")
    L.call("moda_frames_scatter", L.ptr(rtk), L.ptr(kaug), L.ptr(rt_raw), L.ptr(fid), bs, L.ptr(state.rtk), L.ptr(state.rt_raw),
           L.ptr(state.idk), state.num_frames, L.ptr(state.status), L.stream())
    return state


def near_far_splits(N, M):
    """How many point ranges moda_near_far cuts a frame into by itself (moda_near_far_splits)."""
    return int(L.load().moda_near_far_splits(int(N), int(M)))


def get_near_far(near_far, vars, tol_fac=1.2, pts=None, *, rtk_all=None, splits=0):
    """geom_utils.get_near_far: near_far (M,2), a contiguous fp32 device tensor, is updated IN PLACE at the frames with idk == 1
    and returned.  vars: a FrameState, or a dict of numpy arrays ('rtk' (M,4,4), 'idk' (M,), 'mesh_rest' for pts=None), which is
    uploaded once per call.  pts (N,3): numpy or a device tensor; None: the 8 corners of mesh_rest's bounds.  rtk_all (M,3,4):
    the pose patch of moda.py:486-488 first (see reset_near_far).  splits: 0 lets the library choose the number of point ranges
    a frame is cut into, > 0 forces it (tests)."""
    if isinstance(vars, FrameState):
        state = vars
    else:
        state = FrameState(np.asarray(vars['rtk']).shape[0], near_far.device if torch.is_tensor(near_far) else 'cuda')
        state['rtk'], state['idk'] = vars['rtk'], vars['idk']
        state.mesh_rest = vars.get('mesh_rest') if pts is None else None
    M = state.num_frames
    _no_grad("get_near_far", near_far if not isinstance(near_far, torch.nn.Parameter) else None, pts, rtk_all)
    nf = _table(near_far, (M, 2), "get_near_far: near_far")
    if pts is None:
        pts = state.box()
    elif not torch.is_tensor(pts):
        pts = torch.from_numpy(np.ascontiguousarray(np.asarray(pts, np.float32))).to(nf.device)
    pts = L.dev(pts)
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise ValueError(f"get_near_far: pts must be (N,3) with N >= 1, got {tuple(pts.shape)}")
    N = pts.shape[0]
    if rtk_all is not None:
        rtk_all = L.dev(rtk_all)
        if tuple(rtk_all.shape) != (M, 3, 4):
            raise ValueError(f"get_near_far: rtk_all must be ({M}, 3, 4), got {tuple(rtk_all.shape)}")
    splits = int(splits)
    if splits < 0 or splits > MAX_SPLIT or (N <= SMALL_N and splits > 1):
        raise ValueError(f"get_near_far: splits = {splits} with N = {N} (0..{MAX_SPLIT}; frames of up to {SMALL_N} points are not split)")
    n_ws = max(splits, near_far_splits(N, M))
    ws = state.workspace(n_ws) if n_ws > 1 else None
    L.call("moda_near_far", L.ptr(pts), N, L.ptr(state.rtk), L.ptr(state.idk), L.ptr(nf), M, float(tol_fac), L.ptr(rtk_all), splits,
           L.ptr(ws), L.ptr(state.status), L.stream())
    return near_far


def reset_near_far(model, rtk_all, tol_fac=1.2):
    """The block of forward_default at moda.py:485-491 as ONE launch: rows [:3] of every seen frame's pose in
    model.latest_vars (a FrameState) become rtk_all's (compute_rts' table, detached), and model.near_far is recomputed from the
    box of mesh_rest at the seen frames.  The caller keeps the `progress >= opts.nf_reset` test."""
    model = getattr(model, "module", model)
    state = _state_of(model, "reset_near_far")
    get_near_far(model.near_far, state, tol_fac, None, rtk_all=rtk_all)
    return model.near_far


def near_far_to_bound(near_far):
    """geom_utils.near_far_to_bound (:1185-1193): mean(far - near) / 2 as a numpy scalar (one synchronisation)."""
    bound = (near_far[:, 1] - near_far[:, 0]).mean() / 2
    return bound.detach().cpu().numpy()


def reset_nf(model, opts, save_dir=None):
    """Trainer.reset_nf (train_utils.py:826-843): obj_bound from the scaled DensePose vertices on a first stage, the planes from
    those vertices when none were loaded (its `near_far[:,0].sum() == 0` test synchronises; it runs once), and init-nf.txt into
    save_dir if given."""
    m = getattr(model, "module", model)
    state = _state_of(m, "reset_nf")
    nf = m.near_far.data if isinstance(m.near_far, torch.nn.Parameter) else m.near_far
    shape_verts = m.dp_verts_unit.detach() / 3 * nf.mean()
    shape_verts = shape_verts * 1.2
    if opts.model_path == '' and opts.bound_factor > 0:
        shape_verts = shape_verts * opts.bound_factor
        state['obj_bound'] = shape_verts.abs().max(0)[0].cpu().numpy()
    if nf[:, 0].sum() == 0:
        get_near_far(nf, state, pts=shape_verts)
    if save_dir is not None:
        np.savetxt('%s/init-nf.txt' % save_dir, nf.cpu().numpy() * m.obj_scale)
    return m.near_far


def reset_obj_bound(state, mesh_rest):
    """The obj_bound line of reset_hparams (train_utils.py:1102-1104): 1.2 x the rest mesh's largest |coordinate| per axis, when
    the mesh has more than 100 vertices.  (The caller keeps the `epoch > num_epochs * bound_reset` test.)"""
    if mesh_rest.vertices.shape[0] > 100:
        state['obj_bound'] = 1.2 * np.abs(mesh_rest.vertices).max(0)
    return state['obj_bound'] if 'obj_bound' in state else None
