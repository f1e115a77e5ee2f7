"""The stage of the reference's training step between `backward()` and `optimizer.step()`: v2s_trainer.clip_grad
(nnutils/train_utils.py:966 -> :1154-1311) -- NaN test of every gradient, 22 parameter groups by name, the groups the current
stage freezes zeroed, `clip_grad_norm_` per group with the group's threshold, the 22 norms into `aux_out`, every gradient
zeroed when a NaN was seen.  Here the whole stage is three launches of csrc/clip_kernels.hip over the gradients where they
lie (a GradBucket's views or separate `.grad` tensors), with no host synchronisation: it can be captured into the step's graph.

One stated deviation: the reference tests `isnan` only, and an infinite gradient gives coef = 0 and inf * 0 = NaN in the
parameters; here any non-finite value rejects the step, and `status` = [invalid, #NaN, #inf, 0] says which it was."""
import torch

from . import _lib as L
from . import abi

# (aux_out key without its `_g`, factor of opts.clip_scale), in the order of train_utils.py:1285-1306
GRAD_GROUPS = (
    ("nerf_coarse", 1.), ("nerf_beta", 1.), ("nerf_feat", .1), ("nerf_beta_feat", .1), ("nerf_fine", .1), ("nerf_unc", .1),
    ("nerf_flowbw", .1), ("nerf_skin", .1), ("nerf_dis", .1), ("nerf_vis", .1), ("nerf_root_rts", 100.), ("nerf_body_rts", 100.),
    ("root_code", .1), ("pose_code", 100.), ("env_code", .1), ("appearance_code", .1), ("vid_code", .1), ("bones", 1.),
    ("skin_aux", .1), ("ks", .1), ("nerf_dp", .1), ("csenet", .1),
)
GROUP_INDEX = {name: i for i, (name, _) in enumerate(GRAD_GROUPS)}
CHUNK = abi.CONSTANTS["MODA_CLIP_CHUNK"]


def grad_group(name):
    """Index into GRAD_GROUPS of the group clip_grad sorts the parameter `name` into, None for a parameter it leaves alone:
    the if / elif chain of train_utils.py:1188-1232 in its order.  The reference sees DistributedDataParallel's names; a name is
    taken with or without that leading `module.`."""
    n = name[len("module."):] if name.startswith("module.") else name
    if "nerf_coarse" in n and "beta" not in n:
        g = "nerf_coarse"
    elif "nerf_coarse" in n and "beta" in n:
        g = "nerf_beta"
    elif "nerf_feat" in n and "beta" not in n:
        g = "nerf_feat"
    elif "nerf_feat" in n and "beta" in n:
        g = "nerf_beta_feat"
    elif "nerf_fine" in n:
        g = "nerf_fine"
    elif "nerf_unc" in n:
        g = "nerf_unc"
    elif "nerf_flowbw" in n or "nerf_flowfw" in n:
        g = "nerf_flowbw"
    elif "nerf_skin" in n:
        g = "nerf_skin"
    elif "nerf_dis" in n:
        g = "nerf_dis"
    elif "nerf_vis" in n:
        g = "nerf_vis"
    elif "nerf_root_rts" in n:
        g = "nerf_root_rts"
    elif "nerf_body_rts" in n:
        g = "nerf_body_rts"
    elif "root_code" in n:
        g = "root_code"
    elif "pose_code" in n or "rest_pose_code" in n:
        g = "pose_code"
    elif "env_code" in n:
        g = "env_code"
    elif "appearance_code" in n:
        g = "appearance_code"
    elif "vid_code" in n:
        g = "vid_code"
    elif n == "bones":
        g = "bones"
    elif n == "skin_aux":
        g = "skin_aux"
    elif n == "ks_param":
        g = "ks"
    elif "nerf_dp" in n:
        g = "nerf_dp"
    elif "csenet" in n:
        g = "csenet"
    else:
        return None
    return GROUP_INDEX[g]


def _group_ids(groups):
    out = set()
    for g in groups:
        if isinstance(g, str):
            g = GROUP_INDEX[g[:-2] if g.endswith("_g") and g[:-2] in GROUP_INDEX else g]
        g = int(g)
        if not 0 <= g < len(GRAD_GROUPS):
            raise ValueError(f"no gradient group {g}")
        out.add(g)
    return out


def build_tables(segments, n_groups=len(GRAD_GROUPS), chunk=CHUNK):
    """Host side of the kernel's tables.  segments: (numel, group or -1) per gradient tensor in parameter order.  Returns
    (chunk_seg, chunk_off, group_begin): chunks of `chunk` elements that never cross a segment, the chunks of group g being
    [group_begin[g], group_begin[g + 1]) in parameter order and the ungrouped ones [group_begin[n_groups], len)."""
    chunk_seg, chunk_off, group_begin = [], [], []
    for g in list(range(n_groups)) + [-1]:
        group_begin.append(len(chunk_seg))
        for s, (numel, sg) in enumerate(segments):
            if sg == g:
                for off in range(0, numel, chunk):
                    chunk_seg.append(s)
                    chunk_off.append(off)
    return chunk_seg, chunk_off, group_begin


class GradClipper:
    """clip_grad's arithmetic over the gradients of `named_params` ((name, parameter) pairs, e.g. `model.named_parameters()`),
    grouped by `grad_group(name)`; group g is clipped to GRAD_GROUPS[g].factor * clip_scale.  The device tables are built once,
    from the `.grad` tensors as they are at construction: views of a GradBucket -- the bucket's `extra`
    floats and padding belong to no segment and are never touched -- or separate tensors.  A parameter whose grad is None is
    skipped; an empty group reports norm 0.

    frozen: groups (names or indices) whose gradients are zeroed before the norms are taken (they report 0);
    frozen_params: names of single parameters frozen the same way inside a group that otherwise trains.

    `clipper()` enqueues three launches on the current stream and returns (norms (22,) fp32, status (4,) int32 =
    [invalid, #NaN, #inf, 0]) -- device tensors, the same two on every call, nothing read back.  If a gradient's address has
    changed since the tables were built (`zero_grad(set_to_none=True)`), an eager call rebuilds them; a call inside stream
    capture raises, because a captured launch would keep the old addresses."""

    def __init__(self, named_params, clip_scale, frozen=(), frozen_params=()):
        self.named = [(n, p) for n, p in named_params]
        if not self.named:
            raise ValueError("GradClipper: no parameter")
        self.groups = [grad_group(n) for n, _ in self.named]
        self.clip_scale = float(clip_scale)
        self.device = self.named[0][1].device
        if self.device.type != "cuda":
            raise RuntimeError("GradClipper takes CUDA (ROCm) parameters; the HIP library is the only compute path")
        G = len(GRAD_GROUPS)
        self.max_norm = torch.tensor([f * self.clip_scale for _, f in GRAD_GROUPS], dtype=torch.float64).to(torch.float32).to(self.device)
        self.frozen = torch.zeros(G, dtype=torch.uint8, device=self.device)
        self.norms = torch.zeros(G, dtype=torch.float32, device=self.device)
        self.coef = torch.zeros(G, dtype=torch.float32, device=self.device)
        self.status = torch.zeros(4, dtype=torch.int32, device=self.device)
        self.norm_views = [self.norms[i] for i in range(G)]        # 0-d views, what clip_grad puts into aux_out
        self._frozen_groups, self._frozen_params = _group_ids(frozen), set(frozen_params)
        self._sig = None
        self.rebuilds = 0
        self._build()

    def _signature(self):
        return tuple(0 if p.grad is None else p.grad.data_ptr() for _, p in self.named)

    def _build(self):
        segs, names, ptrs = [], [], []
        for (name, p), g in zip(self.named, self.groups):
            gr = p.grad
            if gr is None or gr.numel() == 0:
                continue
            if gr.device != self.device or gr.dtype != torch.float32 or not gr.is_contiguous():
                raise ValueError(f"GradClipper: the gradient of {name} must be a contiguous fp32 tensor on {self.device}")
            segs.append((gr.numel(), -1 if g is None else g))
            names.append(name)
            ptrs.append(gr.data_ptr())
        chunk_seg, chunk_off, group_begin = build_tables(segs)
        if len(chunk_seg) >= 2 ** 31:
            raise ValueError("GradClipper: more than 2^31 chunks")
        dev = self.device
        self.seg_names = names
        self.seg_ptr = torch.tensor(ptrs, dtype=torch.int64).to(dev)
        self.seg_numel = torch.tensor([n for n, _ in segs], dtype=torch.int64).to(dev)
        self.seg_group = torch.tensor([g for _, g in segs], dtype=torch.int32).to(dev)
        self.seg_frozen = torch.zeros(len(segs), dtype=torch.uint8, device=dev)
        self.chunk_seg = torch.tensor(chunk_seg, dtype=torch.int32).to(dev)
        self.chunk_off = torch.tensor(chunk_off, dtype=torch.int64).to(dev)
        self.group_begin = torch.tensor(group_begin, dtype=torch.int32).to(dev)
        self.partial = torch.zeros(len(chunk_seg), dtype=torch.float64, device=dev)
        self.nonfinite = torch.zeros(2 * len(chunk_seg), dtype=torch.int32, device=dev)
        self.n_seg, self.n_chunks = len(segs), len(chunk_seg)
        self._sig = self._signature()
        self.rebuilds += 1
        self._upload_frozen()

    def _upload_frozen(self):
        G = len(GRAD_GROUPS)
        self.frozen.copy_(torch.tensor([int(g in self._frozen_groups) for g in range(G)], dtype=torch.uint8))
        if self.n_seg:
            self.seg_frozen.copy_(torch.tensor([int(n in self._frozen_params) for n in self.seg_names], dtype=torch.uint8))

    def set_frozen(self, groups, params=()):
        """Replace the frozen set (device bytes the kernels read on every launch: a captured graph follows it)."""
        groups, params = _group_ids(groups), set(params)
        known = {n for n, _ in self.named}
        if not params <= known:
            raise ValueError(f"GradClipper.set_frozen: unknown parameters {sorted(params - known)}")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("GradClipper.set_frozen copies from the host: call it outside stream capture")
        self._frozen_groups, self._frozen_params = groups, params
        self._upload_frozen()

    def frozen_state(self):
        return frozenset(self._frozen_groups), frozenset(self._frozen_params)

    def __call__(self):
        if self._sig != self._signature():
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("GradClipper: a gradient tensor has moved since the tables were built, and the stream is being "
                                   "captured -- call the clipper once eagerly (or keep the gradients in a GradBucket) before capture")
            self._build()
        p = L.ptr
        L.call("moda_clip_grad", p(self.seg_ptr), p(self.seg_numel), p(self.seg_group), p(self.seg_frozen), self.n_seg,
               p(self.chunk_seg), p(self.chunk_off), self.n_chunks, p(self.group_begin), len(GRAD_GROUPS), p(self.max_norm),
               p(self.frozen), p(self.partial), p(self.nonfinite), p(self.coef), p(self.norms), p(self.status), L.stream())
        return self.norms, self.status


def find_nerf_coarse(nerf_model):
    """train_utils.py:1313-1342 as whole tensors: (parameters frozen entirely, input-layer weights left alone).  The reference
    zeroes the columns [pos_dim:] of the input-layer weights (layer 0 and the skip layers) and every other parameter of the
    network.  A column range that is neither empty nor the whole weight cannot be expressed per tensor: refused, not
    approximated."""
    frozen, kept = [], []
    input_wt_names = [f"xyz_encoding_{layer + 1}.0.weight" for layer in [0] + list(nerf_model.skips)]
    pos_dim = nerf_model.in_channels_xyz - nerf_model.in_channels_code
    for name, p in nerf_model.named_parameters():
        if name in input_wt_names:
            if pos_dim >= p.shape[1]:
                kept.append(p)
            elif pos_dim <= 0:
                frozen.append(p)
            else:
                raise NotImplementedError(
                    f"freeze_coarse zeroes columns [{pos_dim}:{p.shape[1]}] of {name} (train_utils.py:1339): a part of a tensor, "
                    "which the per-tensor freezing of moda_amd.train_utils.clip_grad does not express")
        else:
            frozen.append(p)
    return frozen, kept


def frozen_for_stage(model, opts):
    """The groups and single parameters clip_grad zeroes in the current stage (train_utils.py:1234-1279): (set of group names,
    list of parameters)."""
    groups, params = set(), []
    if model.root_update == 0:
        groups |= {"root_code", "nerf_root_rts"}
    if model.body_update == 0:
        groups |= {"pose_code", "nerf_body_rts"}
    if getattr(opts, "freeze_body_mlp", False):
        groups |= {"nerf_body_rts"}
    if model.shape_update == 1:
        groups |= {"nerf_coarse", "nerf_beta", "nerf_vis", "bones", "nerf_skin", "nerf_dis", "skin_aux"}
    if model.cvf_update == 1:
        groups |= {"nerf_feat", "nerf_beta_feat", "csenet"}
    if getattr(opts, "freeze_coarse", False):
        for net in ("nerf_coarse", "nerf_skin", "nerf_feat"):
            params += find_nerf_coarse(getattr(model, net))[0]
        groups |= {"bones", "skin_aux", "nerf_vis"}
    return groups, params


def clip_grad(model, aux_out, opts, clipper=None):
    """Drop-in for v2s_trainer.clip_grad(aux_out) (train_utils.py:1154-1311) with the trainer's `self.model` and `self.opts`
    passed in: `model` is the (DistributedDataParallel-wrapped or bare) MoDA module carrying root_update, body_update,
    shape_update and cvf_update, `opts` carries clip_scale, freeze_body_mlp and freeze_coarse.  Fills aux_out['<group>_g'] with
    0-d device tensors (views of the clipper's `norms`) and makes no host synchronisation; the frozen bytes are uploaded only
    when the stage changes.  Returns the GradClipper (kept on `model`), whose `status` tells a rejected step."""
    inner = getattr(model, "module", model)
    if clipper is None:
        clipper = getattr(model, "_moda_grad_clipper", None)
        if clipper is None or clipper.clip_scale != float(opts.clip_scale):
            clipper = GradClipper(model.named_parameters(), opts.clip_scale)
            model._moda_grad_clipper = clipper
    groups, params = frozen_for_stage(inner, opts)
    by_id = {id(p): n for n, p in clipper.named}
    names = {by_id[id(p)] for p in params}
    if (frozenset(_group_ids(groups)), frozenset(names)) != clipper.frozen_state():
        clipper.set_frozen(groups, names)
    clipper()
    for (name, _), v in zip(GRAD_GROUPS, clipper.norm_views):
        aux_out[name + "_g"] = v
    return clipper
