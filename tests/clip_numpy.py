"""Oracles for gradient clipping (moda_amd/train_utils.py, csrc/clip_kernels.hip): the arithmetic of the reference trainer's
clip_grad (nnutils/train_utils.py:1154-1311) restated twice.

  clip_grad_f64    float64 numpy: non-finite scan over EVERY gradient, the frozen ones zeroed, the 2-norm of each group,
                   coef = min(1, max / (norm + 1e-6)), every gradient zeroed when the scan found something.
  clip_grad_torch  plain torch on `.grad` tensors in place, with torch.nn.utils.clip_grad_norm_ -- the function the reference
                   itself calls -- and the reference's isnan-only test (it reads back, as the reference does).
Names are sorted into groups by the function given (moda_amd.train_utils.grad_group); neither imports the package."""
import numpy as np


def clip_grad_f64(grads, groups, max_norm, frozen_groups=(), frozen_tensors=(), reject_inf=True):
    """grads: list of float32 arrays (None = no gradient); groups: group index or None per tensor; max_norm (G,) float32 (the
    thresholds as the kernel and torch see them, rounded to fp32).  Returns dict(grads, norms, coef, invalid, n_nan, n_inf) in
    float64.  reject_inf=False: the reference's isnan-only validity test."""
    G = len(max_norm)
    frozen_groups, frozen_tensors = set(frozen_groups), set(frozen_tensors)
    n_nan = sum(int(np.isnan(g).sum()) for g in grads if g is not None)
    n_inf = sum(int(np.isinf(g).sum()) for g in grads if g is not None)
    invalid = n_nan > 0 or (reject_inf and n_inf > 0)
    out = [None if g is None else np.asarray(g, np.float64).copy() for g in grads]
    for i, g in enumerate(out):
        if g is not None and (groups[i] in frozen_groups or i in frozen_tensors):
            g[...] = 0.0
    sq = np.zeros(G)
    with np.errstate(all="ignore"):
        for i, g in enumerate(out):
            if g is not None and groups[i] is not None:
                sq[groups[i]] += float((g * g).sum())
        norms = np.sqrt(sq)
        coef = np.minimum(1.0, np.asarray(max_norm, np.float64) / (norms + 1e-6))
        for i, g in enumerate(out):
            if g is None:
                continue
            if invalid:
                g[...] = 0.0
            elif groups[i] is not None:
                g *= coef[groups[i]]
    return dict(grads=out, norms=norms, coef=coef, invalid=bool(invalid), n_nan=n_nan, n_inf=n_inf)


def clip_grad_torch(named_params, group_of, factors, clip_scale, frozen_groups=(), frozen_tensors=()):
    """The reference's clip_grad on `(name, parameter)` pairs, in place: group_of(name) -> index or None, factors (G,) the
    per-group multiples of clip_scale, frozen_groups indices, frozen_tensors names.  Returns (list of G norms as 0-d tensors,
    is_invalid_grad)."""
    import torch
    from torch.nn.utils import clip_grad_norm_
    named_params = list(named_params)
    invalid = False
    lists = [[] for _ in factors]
    for name, p in named_params:
        if p.grad is not None and p.grad.isnan().sum() > 0:
            invalid = True
        g = group_of(name)
        if g is not None:
            lists[g].append(p)
    for g in frozen_groups:
        for p in lists[g]:
            if p.grad is not None:
                p.grad.zero_()
    frozen_tensors = set(frozen_tensors)
    for name, p in named_params:
        if name in frozen_tensors and p.grad is not None:
            p.grad.zero_()
    norms = [clip_grad_norm_(lst, f * clip_scale) for lst, f in zip(lists, factors)]
    if invalid:
        for _, p in named_params:
            if p.grad is not None:
                p.grad.zero_()
    return [torch.as_tensor(n) for n in norms], invalid
