"""`from moda_amd.samples_loss import SamplesLoss` where the reference has `from geomloss import SamplesLoss`
(nnutils/moda.py:693): the one configuration MoDA calls -- the debiased Sinkhorn divergence, p = 2, uniform weights, between two
clouds of 3-D points -- on the device, with the epsilon schedule decided there (csrc/sinkdiv_kernels.hip).

geomloss is not part of the reference tree (misc/moda.yml:96 names geomloss==0.2.4); the algorithm is restated from its published
sinkhorn_divergence.py (tensorized route) and is unpinned: tests hold the kernels to a float64 restatement, not to geomloss."""
import torch

from . import autograd as A
from . import abi

MAX_POINTS = abi.CONSTANTS["MODA_SINKDIV_MAX_POINTS"]
BAD_DIAMETER, TOO_MANY_STEPS = abi.CONSTANTS["MODA_SINKDIV_BAD_DIAMETER"], abi.CONSTANTS["MODA_SINKDIV_TOO_MANY_STEPS"]     # status[0] flags


def _refuse(option, value, served):
    raise NotImplementedError(f"moda_amd.samples_loss: {option}={value!r} is not implemented (served: {served})")


class SamplesLoss:
    """geomloss.SamplesLoss(loss="sinkhorn", p=2, blur=.05, scaling=.5, debias=True): loss(x (N,3), y (M,3)) -> 0-dim tensor,
    differentiable in x and y with the gradients geomloss' autograd returns (the envelope gradient of the last extrapolation).
    `blur` and `scaling` (in (0, 1)) are honoured as values; `diameter`, when given, replaces the joint bounding box's diagonal.
    Every other option, explicit weights, batched clouds, D != 3 and CPU tensors raise NotImplementedError naming the option.
    `.status` (4,) int32 on the device after a call: [flags, schedule length n (0 when a flag is set), the bits of the diameter as
    fp32, 0]; flags 1: a coordinate or the diameter is not finite (checked with `diameter` given too), or the diameter <= blur, 2: more than 24 schedule steps (diameter / blur > 2^22) -- the loss is then NaN and
    the gradients are zero.  Nothing is read back and the launch count is fixed, so the call can be captured into a graph."""

    def __init__(self, loss="sinkhorn", p=2, blur=.05, reach=None, diameter=None, scaling=.5, truncate=5, cost=None, kernel=None,
                 cluster_scale=None, debias=True, potentials=False, verbose=False, backend="auto"):
        if loss != "sinkhorn":
            _refuse("loss", loss, "'sinkhorn'")
        if p != 2:
            _refuse("p", p, "2")
        if reach is not None:
            _refuse("reach", reach, "None (balanced transport)")
        if not debias:
            _refuse("debias", debias, "True")
        if potentials:
            _refuse("potentials", potentials, "False")
        if cost is not None:
            _refuse("cost", cost, "None (|x - y|^2 / 2)")
        if kernel is not None:
            _refuse("kernel", kernel, "None")
        if cluster_scale is not None:
            _refuse("cluster_scale", cluster_scale, "None (no multiscale route)")
        if backend not in ("auto", "tensorized"):
            _refuse("backend", backend, "'auto', 'tensorized'")
        if not float(blur) > 0:
            raise ValueError(f"SamplesLoss: blur = {blur!r} must be positive")
        if not 0 < float(scaling) < 1:
            raise ValueError(f"SamplesLoss: scaling = {scaling!r} must lie in (0, 1)")
        if diameter is not None and not float(diameter) > 0:
            raise ValueError(f"SamplesLoss: diameter = {diameter!r} must be positive")
        self.loss, self.p, self.blur, self.reach, self.scaling, self.debias = loss, p, float(blur), reach, float(scaling), debias
        self.diameter = None if diameter is None else float(diameter)
        self.truncate, self.potentials, self.verbose, self.backend = truncate, potentials, verbose, backend   # (truncate: multiscale only)
        self.status = None

    def __call__(self, *args):
        if len(args) != 2:
            _refuse("weights", f"{len(args)} positional arguments", "loss(x, y) with uniform weights")
        x, y = args
        for name, t in (("x", x), ("y", y)):
            if not torch.is_tensor(t):
                raise TypeError(f"SamplesLoss: {name} must be a tensor")
            if t.dim() != 2:
                _refuse("batched input", tuple(t.shape), "(N, 3) and (M, 3)")
            if t.shape[1] != 3:
                _refuse("D", t.shape[1], "3")
            if not t.is_cuda:
                _refuse("device", str(t.device), "CUDA (ROCm) tensors; the HIP library is the only compute path")
            if t.dtype != torch.float32:
                _refuse("dtype", t.dtype, "torch.float32")
        if x.shape[0] < 1 or y.shape[0] < 1:
            raise ValueError("SamplesLoss: empty point cloud")
        if x.shape[0] + y.shape[0] > MAX_POINTS:
            raise ValueError(f"SamplesLoss: {x.shape[0]} + {y.shape[0]} points, the kernels hold at most {MAX_POINTS}")
        if self.status is None or self.status.device != x.device:
            self.status = torch.zeros((4,), dtype=torch.int32, device=x.device)
        return A.SinkhornDivFn.apply(x, y, self.blur, self.scaling, self.diameter, self.status)

    forward = __call__
