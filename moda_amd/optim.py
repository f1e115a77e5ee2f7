"""The last stage of the reference's training step: `optimizer.step(); scheduler.step(); optimizer.zero_grad()`
(nnutils/train_utils.py:967-969) over the optimiser and the schedule that `init_training` builds (:155-290) -- AdamW(betas
(0.9, 0.999), weight_decay 1e-4) over 22 parameter groups, OneCycleLR with per-group peaks (10x for nerf_beta_feat, skin_aux and
ks, lr_nerf_root_rts x for nerf_root_rts and root_code), pct_start = 2 / num_epochs, linear anneal, div_factor 25,
final_div_factor 1/5.  Here the stage is two launches of csrc/optim_kernels.hip over the parameters and gradients where they
lie, with no host synchronisation; the step counter and the learning rates live on the device, so a captured graph follows the
schedule when it is replayed -- which torch's host-side scheduler cannot do.

One stated deviation: past `total_steps` torch's scheduler raises ValueError.  Nothing can raise from a replayed graph: the
learning rate of `total_steps` is held, and `status[0]` counts the steps taken past it."""
import torch

from . import _lib as L
from .train_utils import CHUNK, GRAD_GROUPS, GROUP_INDEX, grad_group

# lr_nerf_root_rts of train_utils.py:252-260, by model.root_basis
ROOT_BASIS_FACTOR = {"exp": 10., "cnn": 0.2, "mlp": 1., "expmlp": 1.}
TEN_X_GROUPS = ("nerf_beta_feat", "skin_aux", "ks")             # train_utils.py:265, :280, :281
ROOT_GROUPS = ("nerf_root_rts", "root_code")                    # train_utils.py:272, :274


def group_lr_factors(root_basis="expmlp"):
    """The 22 factors of opts.learning_rate in OneCycleLR's max_lr list (train_utils.py:262-284), in GRAD_GROUPS order."""
    if root_basis not in ROOT_BASIS_FACTOR:
        raise ValueError(f"root_basis {root_basis!r}: the reference knows {sorted(ROOT_BASIS_FACTOR)}")
    f = [1.] * len(GRAD_GROUPS)
    for n in TEN_X_GROUPS:
        f[GROUP_INDEX[n]] = 10.
    for n in ROOT_GROUPS:
        f[GROUP_INDEX[n]] = ROOT_BASIS_FACTOR[root_basis]
    return f


def check_schedule(total_steps, pct_start):
    """What OneCycleLR's constructor checks, plus the two step counts at which its get_lr divides by zero."""
    if int(total_steps) != total_steps or total_steps < 1:
        raise ValueError(f"total_steps must be a positive integer, got {total_steps}")
    if not 0. <= pct_start <= 1.:
        raise ValueError(f"pct_start must be in [0, 1], got {pct_start}")
    end0, end1 = float(pct_start * total_steps) - 1, float(total_steps) - 1
    if end0 == 0 or end1 == end0:
        raise ValueError(f"OneCycleLR(total_steps={total_steps}, pct_start={pct_start}) has a phase of no length "
                         "(torch divides by zero when it reaches it)")


def check_tensor(what, name, t, device):
    """The kernels read contiguous fp32 memory of one device: anything else is refused by name, never converted."""
    if t.dtype != torch.float32 or not t.is_contiguous() or (device is not None and t.device != device):
        raise ValueError(f"DeviceAdamW: {what} {name} must be a contiguous fp32 tensor"
                         + (f" on {device}" if device is not None else "")
                         + f" (it is {t.dtype}, {'contiguous' if t.is_contiguous() else 'not contiguous'}, on {t.device})")


def build_tables(numels, chunk=CHUNK):
    """Host side of the kernel's tables.  numels: elements per segment.  Returns (chunk_seg, chunk_off, seg_moff, n_state):
    chunks of `chunk` elements that never cross a segment, in segment order; seg_moff[s] = where the segment's moments begin in
    the flat state buffers of n_state floats, a multiple of 4 so that 16-byte accesses stay possible."""
    chunk_seg, chunk_off, seg_moff, n_state = [], [], [], 0
    for s, numel in enumerate(numels):
        if numel < 1:
            raise ValueError(f"segment {s} is empty")
        seg_moff.append(n_state)
        n_state += (numel + 3) // 4 * 4
        for off in range(0, numel, chunk):
            chunk_seg.append(s)
            chunk_off.append(off)
    return chunk_seg, chunk_off, seg_moff, n_state


class DeviceAdamW:
    """The reference's AdamW + OneCycleLR over `named_params` ((name, parameter) pairs, e.g. `model.named_parameters()`), grouped by
    `train_utils.grad_group(name)` -- the name chain of train_utils.py:177-222.  A parameter that falls through the chain is
    NOT optimised, as in the reference (`else: continue`); its name is in `.skipped`.  Group g peaks at
    group_lr_factors(root_basis)[g] * learning_rate.

    The device tables are built from the `.grad` tensors as they are: views of a GradBucket or separate tensors.  A parameter
    whose grad is None is left out -- torch skips it too, and its `step` does not advance -- and joins at k = 1 when a gradient
    appears.  `exp_avg` / `exp_avg_sq` are one flat buffer each.  If a gradient's (or parameter's) address has changed since the
    tables were built, an eager call rebuilds them and carries the state over by name; a call inside stream capture raises,
    because a captured launch would keep the old addresses.

    `step()` enqueues two launches on the current stream and returns (lr (22,) fp32 = the rates this step applied, status (4,)
    int32 = [steps past total_steps, 0, 0, 0]) -- device tensors, the same two on every call, nothing read back.  `lr_views` are
    0-d views of the rates `param_groups[i]['lr']` holds AFTER scheduler.step(), which is what the reference logs
    (train_utils.py:976-977).  The stage never looks at the clipper's status: zero gradients still decay and step, as in torch."""

    def __init__(self, named_params, learning_rate, total_steps, pct_start, root_basis="expmlp", betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=1e-4, div_factor=25., final_div_factor=1. / 5, zero_grad=False):
        named = [(n, p) for n, p in named_params]
        groups = [grad_group(n) for n, _ in named]
        self.skipped = [n for (n, _), g in zip(named, groups) if g is None]
        self.named = [(n, p) for (n, p), g in zip(named, groups) if g is not None]
        self.groups = [g for g in groups if g is not None]
        if not self.named:
            raise ValueError("DeviceAdamW: no parameter belongs to a group")
        if len({n for n, _ in self.named}) != len(self.named):
            raise ValueError("DeviceAdamW: parameter names must be unique (the state is kept by name)")
        for n, p in self.named:
            check_tensor("parameter", n, p, None)
        self.device = self.named[0][1].device
        for n, p in self.named:
            check_tensor("parameter", n, p, self.device)
        check_schedule(total_steps, pct_start)
        if not (div_factor > 0 and final_div_factor > 0 and 0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("DeviceAdamW: div_factor and final_div_factor must be positive, the betas in [0, 1)")
        self.learning_rate, self.total_steps, self.pct_start = float(learning_rate), int(total_steps), float(pct_start)
        self.root_basis, self.betas, self.eps, self.weight_decay = root_basis, (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.div_factor, self.final_div_factor, self.zero_grad = float(div_factor), float(final_div_factor), bool(zero_grad)
        self.max_lr = [f * self.learning_rate for f in group_lr_factors(root_basis)]      # Python doubles, as the reference's list
        if self.device.type != "cuda":
            raise RuntimeError("DeviceAdamW takes CUDA (ROCm) parameters; the HIP library is the only compute path")
        G, dev = len(GRAD_GROUPS), self.device
        self._max_lr = torch.tensor(self.max_lr, dtype=torch.float64).to(dev)
        self.step_count = torch.zeros(1, dtype=torch.int64, device=dev)
        self._lr = torch.zeros(2 * G, dtype=torch.float32, device=dev)
        self.lr, self.lr_next = self._lr[:G], self._lr[G:]
        self.lr_views = [self.lr_next[i] for i in range(G)]
        self.status = torch.zeros(4, dtype=torch.int32, device=dev)
        self._parked = {}              # name -> (k, exp_avg, exp_avg_sq) of parameters with state and, at present, no gradient
        self.seg_names, self.n_seg, self.n_chunks = [], 0, 0
        self._sig = None
        self.rebuilds = 0
        self._build()

    # ------------------------------------------------------------------ tables
    def _signature(self):
        return tuple((p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr()) for _, p in self.named)

    def _export(self):
        """name -> (k, exp_avg, exp_avg_sq) of every parameter that has state: the current segments' and the parked ones'."""
        out = dict(self._parked)
        if self.n_seg:
            ks = self.seg_step.tolist()
            for name, k, off, n in zip(self.seg_names, ks, self._moff, self._numel):
                out[name] = (k, self.exp_avg[off:off + n].clone(), self.exp_avg_sq[off:off + n].clone())
        return out

    def _build(self, state=None):
        state = self._export() if state is None else state
        names, ps, gs, numels, groups = [], [], [], [], []
        for (name, p), g in zip(self.named, self.groups):
            gr = p.grad
            if gr is None or gr.numel() == 0:
                continue
            check_tensor("parameter", name, p, self.device)
            check_tensor("the gradient of", name, gr, self.device)
            names.append(name)
            ps.append(p.data_ptr())
            gs.append(gr.data_ptr())
            numels.append(gr.numel())
            groups.append(g)
        chunk_seg, chunk_off, moff, n_state = build_tables(numels)
        if len(chunk_seg) >= 2 ** 31:
            raise ValueError("DeviceAdamW: more than 2^31 chunks")
        dev = self.device

        def table(v, dt):
            return torch.tensor(v, dtype=dt).to(dev)
        self.seg_names, self._moff, self._numel = names, moff, numels
        self.seg_p, self.seg_g = table(ps, torch.int64), table(gs, torch.int64)
        self.seg_numel, self.seg_group, self.seg_moff = table(numels, torch.int64), table(groups, torch.int32), table(moff, torch.int64)
        self.chunk_seg, self.chunk_off = table(chunk_seg, torch.int32), table(chunk_off, torch.int64)
        self.seg_step = table([state[n][0] if n in state else 0 for n in names], torch.int64)
        self.seg_fac = torch.zeros(3 * len(names), dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(n_state, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n_state, dtype=torch.float32, device=dev)
        for name, off, n in zip(names, moff, numels):
            if name in state:
                _, m, v = state[name]
                if m.numel() != n or v.numel() != n:
                    raise ValueError(f"DeviceAdamW: the state of {name} has {m.numel()} elements, the parameter {n}")
                self.exp_avg[off:off + n].copy_(m.reshape(-1))
                self.exp_avg_sq[off:off + n].copy_(v.reshape(-1))
        live = set(names)
        self._parked = {n: s for n, s in state.items() if n not in live}
        self.n_seg, self.n_chunks, self.n_state = len(names), len(chunk_seg), n_state
        self._sig = self._signature()
        self.rebuilds += 1

    # ------------------------------------------------------------------ the step
    def step(self, zero_grad=None):
        if self._sig != self._signature():
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("DeviceAdamW: a parameter or gradient tensor has moved since the tables were built, and the stream "
                                   "is being captured -- call step() once eagerly (or keep the gradients in a GradBucket) before capture")
            self._build()
        p = L.ptr
        zg = self.zero_grad if zero_grad is None else bool(zero_grad)
        L.call("moda_adamw_step", p(self.seg_p), p(self.seg_g), p(self.seg_numel), p(self.seg_group), p(self.seg_moff), self.n_seg,
               p(self.chunk_seg), p(self.chunk_off), self.n_chunks, p(self._max_lr), len(GRAD_GROUPS), self.total_steps,
               self.pct_start, self.div_factor, self.final_div_factor, self.betas[0], self.betas[1], self.eps, self.weight_decay,
               p(self.step_count), p(self.seg_step), p(self.exp_avg), p(self.exp_avg_sq), self.n_state, p(self._lr), p(self.seg_fac),
               p(self.status), int(zg), L.stream())
        return self.lr, self.status

    # ------------------------------------------------------------------ resume
    def state_dict(self):
        """Everything a resumed run needs: the step counter, the overrun count, and per parameter name its own step count and
        both moments (CPU tensors shaped like the parameter).  Reads the device: call it outside stream capture."""
        shapes = {n: p.shape for n, p in self.named}
        st = self._export()
        return {"step": int(self.step_count.item()), "overrun": int(self.status[0].item()),
                "state": {n: {"step": int(k), "exp_avg": m.reshape(shapes[n]).cpu(), "exp_avg_sq": v.reshape(shapes[n]).cpu()}
                          for n, (k, m, v) in st.items()}}

    def load_state_dict(self, sd):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("DeviceAdamW.load_state_dict copies from the host: call it outside stream capture")
        known = {n: p for n, p in self.named}
        unknown = sorted(set(sd["state"]) - set(known))
        if unknown:
            raise ValueError(f"DeviceAdamW.load_state_dict: no parameter named {unknown}")
        state = {}
        for n, s in sd["state"].items():
            m, v = (torch.as_tensor(s[k]).to(device=self.device, dtype=torch.float32).reshape(-1) for k in ("exp_avg", "exp_avg_sq"))
            if m.numel() != known[n].numel() or v.numel() != known[n].numel():
                raise ValueError(f"DeviceAdamW.load_state_dict: the state of {n} has {m.numel()} elements, the parameter {known[n].numel()}")
            state[n] = (int(s["step"]), m, v)
        self._build(state)
        self.step_count.fill_(int(sd["step"]))
        self.status.zero_()
        self.status[0] = int(sd.get("overrun", 0))


def build_optimizer(model, opts, final_steps, num_epochs, accu_steps=1):
    """The arithmetic of v2s_trainer.init_training (train_utils.py:226-290) with the trainer's model passed in: `model` is the
    (DistributedDataParallel-wrapped or bare) MoDA module carrying root_basis, `opts` carries learning_rate.  total_steps =
    int(final_steps / accu_steps) and pct_start = 2 / num_epochs, as :285-286.  The optimiser is kept on `model` for
    `optimizer_step`."""
    inner = getattr(model, "module", model)
    opt = DeviceAdamW(model.named_parameters(), opts.learning_rate, int(final_steps / accu_steps), 2. / num_epochs,
                      root_basis=getattr(inner, "root_basis", "expmlp"))
    model._moda_optimizer = opt
    return opt


def optimizer_step(model, aux_out, zero_grad=True):
    """Drop-in for train_utils.py:967-969 and :976-977: optimizer.step(), scheduler.step(), optimizer.zero_grad() (zeros written
    by the same pass that reads the gradients) and aux_out['lr_%02d'] = the group's rate after scheduler.step(), as 0-d device
    tensors.  No host synchronisation."""
    opt = getattr(model, "_moda_optimizer", None)
    if opt is None:
        raise RuntimeError("optimizer_step: call build_optimizer(model, opts, final_steps, num_epochs) first")
    opt.step(zero_grad=zero_grad)
    for i, v in enumerate(opt.lr_views):
        aux_out["lr_%02d" % i] = v
    return opt
