"""Mesh evaluation on the GPU: what the reference does with an extracted mesh (scripts/visualize/render_vis.py:379-417) --
register the predicted vertices to the ground truth with ICP, take the two-sided Chamfer distance, report `cd` and the
F-score at 1 %, 2 % and 5 % of the bounding box -- behind the names the reference imports:

    chamfer3D.dist_chamfer_3D.chamfer_3DDist   ->  moda_amd.mesh_eval.chamfer_3DDist
    fscore.fscore                              ->  moda_amd.mesh_eval.fscore
    pytorch3d.ops.iterative_closest_point      ->  moda_amd.mesh_eval.iterative_closest_point

The search, the Chamfer gradient, the ICP sums and the similarity update are kernels of moda_amd/csrc/pointset_kernels.hip;
the 3 x 3 alignment of an ICP step is solved on the host in float64 from those sums (one small read-back per iteration).
iterative_closest_point_device and eval_sequence do a whole batch of clouds, or every frame of a sequence, with the alignment
and the stopping rule on the device as well (csrc/icpdev_kernels.hip): no read-back inside the loop.
Every entry point checks its inputs and raises ValueError for a non-finite coordinate: the search orders distances, and a
NaN has no order."""
from collections import namedtuple
import ctypes

import numpy as np
import torch

from . import _lib as L
from . import abi

SimilarityTransform = namedtuple("SimilarityTransform", "R T s")
ICPSolution = namedtuple("ICPSolution", "converged rmse Xt RTs t_history")

_NSUM, _ICP_MAX_BLOCKS = abi.CONSTANTS["MODA_ICP_NSUM"], abi.CONSTANTS["MODA_ICP_MAX_BLOCKS"]


def _clouds(x, y, what):
    """-> (x (B,N,3), y (B,M,3)) fp32 contiguous on the device, batched flag.  Refuses what the kernels do not serve."""
    if not (torch.is_tensor(x) and torch.is_tensor(y)):
        raise TypeError(f"{what}: expected tensors, got {type(x).__name__} and {type(y).__name__}")
    if x.dim() != y.dim() or x.dim() not in (2, 3) or x.shape[-1] != 3 or y.shape[-1] != 3:
        raise ValueError(f"{what}: expected (N,3) and (M,3), or (B,N,3) and (B,M,3); got {tuple(x.shape)} and {tuple(y.shape)}")
    batched = x.dim() == 3
    if not batched:
        x, y = x[None], y[None]
    if x.shape[0] != y.shape[0] or x.shape[0] < 1:
        raise ValueError(f"{what}: batch sizes {x.shape[0]} and {y.shape[0]}")
    B, N, M = int(x.shape[0]), int(x.shape[1]), int(y.shape[1])
    if M < 1:
        raise ValueError(f"{what}: the target cloud is empty")
    if B * N >= 2 ** 31 or B * M >= 2 ** 31:
        raise ValueError(f"{what}: B*N = {B * N} or B*M = {B * M} exceeds int32 indices")
    x, y = L.dev(x.detach()), L.dev(y.detach())
    if not bool(torch.isfinite(x).all() & torch.isfinite(y).all()):          # one fused read-back per call
        raise ValueError(f"{what}: non-finite coordinate in the input")
    return x, y, batched


def nn_plan(B, N, M):
    """-> (ranges, targets per range) of the split over the targets that moda_nn_fwd uses for this shape."""
    rng = ctypes.c_int64(0)
    s = L.load().moda_nn_splits(B, N, M, ctypes.byref(rng))
    return int(s), int(rng.value)


def _nearest(x, y):
    """x (B,N,3), y (B,M,3) checked device tensors -> dist2 (B,N) fp32, idx (B,N) int32."""
    B, N, M = int(x.shape[0]), int(x.shape[1]), int(y.shape[1])
    dist2 = torch.empty((B, N), dtype=torch.float32, device=x.device)
    idx = torch.empty((B, N), dtype=torch.int32, device=x.device)
    keys = torch.empty((B, N), dtype=torch.int64, device=x.device) if N and nn_plan(B, N, M)[0] > 1 else None
    L.call("moda_nn_fwd", L.ptr(x), L.ptr(y), B, N, M, L.ptr(dist2), L.ptr(idx), L.ptr(keys), L.stream())
    return dist2, idx


@torch.no_grad()
def nearest(x, y):
    """For every point of x the nearest point of y: (dist2, idx), squared distance fp32 and int32 index, shaped like x
    without its last axis.  Among targets at equal computed distance the lowest index is returned.  No graph is built."""
    x, y, batched = _clouds(x, y, "nearest")
    d, i = _nearest(x, y)
    return (d, i) if batched else (d[0], i[0])


def _chamfer_bwd(x, y, idx, g, gx, gy):
    B, N, M = int(x.shape[0]), int(x.shape[1]), int(y.shape[1])
    L.call("moda_chamfer_bwd", L.ptr(x), L.ptr(y), L.ptr(idx), L.ptr(g), B, N, M, L.ptr(gx), L.ptr(gy), L.stream())


class _ChamferFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2):
        x, y, _ = _clouds(xyz1, xyz2, "chamfer_3DDist")
        d1, i1 = _nearest(x, y)
        d2, i2 = _nearest(y, x)
        ctx.save_for_backward(x, y, i1, i2)
        ctx.dtypes = (xyz1.dtype, xyz2.dtype)
        ctx.mark_non_differentiable(i1, i2)
        return d1, d2, i1, i2

    @staticmethod
    def backward(ctx, g1, g2, _gi1, _gi2):
        x, y, i1, i2 = ctx.saved_tensors
        gx, gy = torch.zeros_like(x), torch.zeros_like(y)
        if g1 is not None:
            _chamfer_bwd(x, y, i1, L.dev(g1), gx, gy)
        if g2 is not None:
            _chamfer_bwd(y, x, i2, L.dev(g2), gy, gx)
        return gx.to(ctx.dtypes[0]), gy.to(ctx.dtypes[1])


class chamfer_3DDist(torch.nn.Module):
    """chamfer3D.dist_chamfer_3D.chamfer_3DDist (dist_chamfer_3D.py:67-74): `dist1, dist2, idx1, idx2 = chamLoss(xyz1, xyz2)`
    for xyz1 (B,N,3) and xyz2 (B,M,3): squared distance of every xyz1 point to its nearest xyz2 point and back, and the
    int32 indices.  Differentiable in both clouds."""

    def forward(self, input1, input2):
        if input1.dim() != 3 or input2.dim() != 3:
            raise ValueError(f"chamfer_3DDist takes (B,N,3) and (B,M,3), got {tuple(input1.shape)} and {tuple(input2.shape)}")
        if input1.shape[1] < 1:
            raise ValueError("chamfer_3DDist: the first cloud is empty")
        return _ChamferFn.apply(input1, input2)


def fscore(dist1, dist2, threshold=0.001):
    """third_party/fscore.py:27-40: the share of dist1 and of dist2 (squared distances, (B,N) and (B,M)) under `threshold`,
    and their harmonic mean, which is 0 where both shares are 0.  -> (fscore, precision_1, precision_2), each (B,).
    Every quotient is formed in float64 from its fp32 operands and rounded once: for fp32 operands that is the correctly
    rounded fp32 quotient, which is what the reference computes on the CPU.  (On the device torch.mean, and a division by a
    Python scalar, multiply by a rounded reciprocal: 255 / 517 came out one ulp high.)"""
    def quotient(a, b):
        return (a.double() / b.double()).float()
    n1 = torch.full((), dist1.shape[1], dtype=torch.float32, device=dist1.device)
    n2 = torch.full((), dist2.shape[1], dtype=torch.float32, device=dist2.device)
    precision_1 = quotient((dist1 < threshold).float().sum(dim=1), n1)
    precision_2 = quotient((dist2 < threshold).float().sum(dim=1), n2)
    f = quotient(2 * precision_1 * precision_2, precision_1 + precision_2)
    f[torch.isnan(f)] = 0
    return f, precision_1, precision_2


def _icp_sums(x0, y, idx, xt, partials):
    B, N, M = int(y.shape[0]), int(idx.shape[1]), int(y.shape[1])
    sums = torch.zeros((B, _NSUM), dtype=torch.float64, device=y.device)
    L.call("moda_icp_moments", L.ptr(x0), L.ptr(y), L.ptr(idx), L.ptr(xt), B, N, M, L.ptr(partials), L.ptr(sums), L.stream())
    return sums


def icp_moments(x0, y, idx, xt=None):
    """The float64 sums of moda_icp_moments for checked (B,N,3) / (B,M,3) device clouds and idx (B,N) int32: (B,17)."""
    partials = torch.empty((int(y.shape[0]), _ICP_MAX_BLOCKS, _NSUM), dtype=torch.float64, device=y.device)
    return _icp_sums(x0, y, idx, xt, partials)


def _align(sums, n, estimate_scale, allow_reflection):
    """The similarity that maps X onto its correspondences, from the sums of one batch element (float64, host)."""
    mx, my = sums[0:3] / n, sums[3:6] / n
    C = sums[6:15].reshape(3, 3) / n - np.outer(mx, my)
    U, S, Vt = np.linalg.svd(C)
    E = np.ones(3)
    if not allow_reflection:
        E[2] = np.linalg.det(U @ Vt)
    R = (U * E) @ Vt
    s = 1.0
    if estimate_scale:
        var = sums[15] / n - mx @ mx
        s = float((S * E).sum() / var)
    T = my - s * mx @ R
    return R, T, s


def _apply(x, rts_host):
    B, N = int(x.shape[0]), int(x.shape[1])
    rts = torch.as_tensor(rts_host, dtype=torch.float32).to(x.device)
    out = torch.empty_like(x)
    L.call("moda_sim3_apply", L.ptr(x), L.ptr(rts), B, N, L.ptr(out), L.stream())
    return out


@torch.no_grad()
def iterative_closest_point(X, Y, init_transform=None, max_iterations=100, relative_rmse_thr=1e-6, estimate_scale=False,
                            allow_reflection=False):
    """pytorch3d.ops.iterative_closest_point for equal-length clouds X (B,N,3), Y (B,M,3), as render_vis.py:390-392 calls it.
    Row vectors throughout: Xt = s * X @ R + T.  Each iteration finds Yn = Y[nearest(Xt, Y)], solves for the similarity
    mapping the ORIGINAL X onto Yn (Umeyama: centred cross-covariance, SVD, the last singular direction flipped when
    det(U V^T) < 0 unless allow_reflection; s = trace(S E) / var(X) when estimate_scale), updates Xt and
    rmse = sqrt(mean |Xt - Yn|^2), and stops as converged once (prev_rmse - rmse) / prev_rmse <= relative_rmse_thr for
    every batch element (1 on the first iteration; an rmse that is already exactly 0 counts as converged).
    -> ICPSolution(converged, rmse (B,), Xt (B,N,3), SimilarityTransform(R (B,3,3), T (B,3), s (B,)), t_history)."""
    if not (torch.is_tensor(X) and torch.is_tensor(Y)):
        raise ValueError("iterative_closest_point takes equal-length clouds as (B,N,3) tensors; padded point-cloud "
                         "structures with masks are not supported")
    if X.dim() != 3 or Y.dim() != 3:
        raise ValueError(f"iterative_closest_point takes (B,N,3) and (B,M,3), got {tuple(X.shape)} and {tuple(Y.shape)}")
    x0, y, _ = _clouds(X, Y, "iterative_closest_point")
    B, N = int(x0.shape[0]), int(x0.shape[1])
    if N < 1:
        raise ValueError("iterative_closest_point: the source cloud is empty")
    if max_iterations < 1:
        raise ValueError("iterative_closest_point: max_iterations must be at least 1")
    dev = x0.device
    R = np.tile(np.eye(3), (B, 1, 1))
    T = np.zeros((B, 3))
    s = np.ones(B)
    if init_transform is not None:
        try:
            R0, T0, s0 = init_transform
        except Exception:
            raise ValueError("init_transform must be a SimilarityTransform (R (B,3,3), T (B,3), s (B,))")
        R0, T0, s0 = (np.asarray(torch.as_tensor(v).detach().cpu(), np.float64) for v in (R0, T0, s0))
        if R0.shape != (B, 3, 3) or T0.shape != (B, 3) or s0.shape != (B,):
            raise ValueError(f"init_transform shapes {R0.shape}, {T0.shape}, {s0.shape} do not match a batch of {B}")
        R, T, s = R0.copy(), T0.copy(), s0.copy()

    def pack():
        return np.concatenate([R.reshape(B, 9), T, s[:, None]], 1)

    xt = _apply(x0, pack()) if init_transform is not None else x0.clone()
    partials = torch.empty((B, _ICP_MAX_BLOCKS, _NSUM), dtype=torch.float64, device=dev)
    prev = None
    rmse = np.zeros(B)
    converged = False
    history = []
    for _ in range(int(max_iterations)):
        _, idx = _nearest(xt, y)
        sums = _icp_sums(x0, y, idx, None, partials).cpu().numpy()           # the read-back of this iteration
        for b in range(B):
            R[b], T[b], s[b] = _align(sums[b], N, estimate_scale, allow_reflection)
        xt = _apply(x0, pack())
        rmse = np.sqrt(_icp_sums(None, y, idx, xt, partials).cpu().numpy()[:, 16] / N)
        if prev is None:
            relative = np.ones(B)
        else:
            relative = np.where(prev > 0, (prev - rmse) / np.where(prev > 0, prev, 1.0), 0.0)
        history.append(SimilarityTransform(*(torch.as_tensor(v, dtype=torch.float32).to(dev) for v in (R, T, s))))
        prev = rmse
        if bool((relative <= relative_rmse_thr).all()):
            converged = True
            break
    return ICPSolution(converged, torch.as_tensor(rmse, dtype=torch.float32).to(dev), xt, history[-1], history)


def _verts(v, device=None):
    if hasattr(v, "vertices_t"):
        v = v.vertices_t
    elif not torch.is_tensor(v):
        v = torch.as_tensor(np.asarray(getattr(v, "vertices", v), np.float32))
    if v.dim() == 3 and v.shape[0] == 1:
        v = v[0]
    if v.dim() != 2 or v.shape[-1] != 3 or v.shape[0] < 1:
        raise ValueError(f"eval_mesh takes (V,3) vertices, got {tuple(v.shape)}")
    if not v.is_cuda:
        v = v.to(device if device is not None else "cuda")
    return L.dev(v.detach())[None]


@torch.no_grad()
def eval_mesh(verts, verts_gt):
    """render_vis.py:379-417 from the point where both vertex sets are in the camera frame; either argument a TriMesh, a numpy
    array or a tensor of (V,3) vertices.  bbox_max = the longest side of verts_gt's box; verts are scaled by the ratio of the
    median depths (torch.median: the lower median), registered to verts_gt with ICP (no scale, at most 100 iterations), then
    raw_cd, raw_cd_back = chamLoss(verts_gt, verts) and the F-scores at (bbox_max * {0.01, 0.02, 0.05})^2.
    -> dict: cd = mean sqrt(raw_cd) + mean sqrt(raw_cd_back), f001, f002, f005 (floats), raw_cd, raw_cd_back (the square
    roots, device tensors), verts (registered, (V,3)), icp (the ICPSolution), bbox_max, fitted_scale."""
    gt = _verts(verts_gt)
    v = _verts(verts, gt.device)
    _clouds(v, gt, "eval_mesh")                                               # the finite check, before anything is derived
    bbox_max = float((gt.max(1)[0] - gt.min(1)[0]).max().cpu())               # :379
    fitted_scale = gt[..., -1].median() / v[..., -1].median()                 # :387
    v = v * fitted_scale
    frts = iterative_closest_point(v, gt, estimate_scale=False, max_iterations=100)   # :390-391
    v = frts.Xt                                                               # :392, the same update on the device
    raw_cd, raw_cd_back, _, _ = chamfer_3DDist()(gt, v)                       # :399
    out = {}
    for key, frac in (("f001", 0.01), ("f002", 0.02), ("f005", 0.05)):        # :400-405
        out[key] = float(fscore(raw_cd, raw_cd_back, threshold=(bbox_max * frac) ** 2)[0][0].cpu())
    raw_cd, raw_cd_back = raw_cd[0].sqrt(), raw_cd_back[0].sqrt()             # :410-411
    out.update(cd=float((raw_cd.mean(dtype=torch.float64) + raw_cd_back.mean(dtype=torch.float64)).cpu()),
               raw_cd=raw_cd, raw_cd_back=raw_cd_back, verts=v[0], icp=frts, bbox_max=bbox_max,
               fitted_scale=float(fitted_scale.cpu()))
    return out


# ---- the whole sequence at once: ICP and metrics without read-backs (csrc/icpdev_kernels.hip) -------------------------------
_NMETRIC = abi.CONSTANTS["MODA_SEQ_NMETRIC"]


class ICPSolutionDevice(ICPSolution):
    """The ICPSolution of iterative_closest_point_device: `converged` is a (B,) bool device tensor and t_history is None unless
    it was asked for; beside the five fields, .iterations (B,) int32 and .idx (B,N) int32 (the last correspondences)."""


def _capturing():
    return torch.cuda.is_current_stream_capturing()


def _ragged_clouds(X, Y, y_len, what):
    """-> x (B,N,3), y (B,M_max,3) fp32 device, lens (B,) int32 device.  One read-back (finite coordinates in the valid rows,
    lengths in 1..M_max), which is skipped on a capturing stream: there the caller vouches for both."""
    if not (torch.is_tensor(X) and torch.is_tensor(Y)):
        raise TypeError(f"{what}: expected tensors, got {type(X).__name__} and {type(Y).__name__}")
    if X.dim() != 3 or Y.dim() != 3 or X.shape[-1] != 3 or Y.shape[-1] != 3:
        raise ValueError(f"{what} takes (B,N,3) and (B,M,3), got {tuple(X.shape)} and {tuple(Y.shape)}")
    if X.requires_grad or Y.requires_grad:
        raise NotImplementedError(f"{what} has no backward: detach its inputs")
    B, N, M = int(X.shape[0]), int(X.shape[1]), int(Y.shape[1])
    if B < 1 or Y.shape[0] != B:
        raise ValueError(f"{what}: batch sizes {X.shape[0]} and {Y.shape[0]}")
    if N < 1 or M < 1:
        raise ValueError(f"{what}: the {'source' if N < 1 else 'target'} cloud is empty")
    if B * N >= 2 ** 31 or B * M >= 2 ** 31:
        raise ValueError(f"{what}: B*N = {B * N} or B*M = {B * M} exceeds int32 indices")
    x, y = L.dev(X), L.dev(Y)
    if y_len is None:
        lens = torch.full((B,), M, dtype=torch.int32, device=x.device)
    else:
        if not torch.is_tensor(y_len) or not y_len.is_cuda:
            host = np.asarray(y_len.cpu() if torch.is_tensor(y_len) else y_len)
            if host.shape != (B,):
                raise ValueError(f"{what}: y_len has shape {host.shape} for a batch of {B}")
            if (host < 1).any() or (host > M).any():
                raise ValueError(f"{what}: y_len must lie in 1..{M}, got {host.tolist()}")
            y_len = torch.as_tensor(host.astype(np.int32)).to(x.device)
        if tuple(y_len.shape) != (B,):
            raise ValueError(f"{what}: y_len has shape {tuple(y_len.shape)} for a batch of {B}")
        lens = y_len.to(torch.int32).contiguous()
    if _capturing():
        return x, y, lens
    in_range = (lens >= 1) & (lens <= M)
    valid = torch.arange(M, device=x.device)[None, :] < lens[:, None]
    finite = torch.isfinite(x).all() & (torch.isfinite(y).all(-1) | ~valid).all()
    if not bool(finite & in_range.all()):                                     # the one read-back
        if not bool(in_range.all()):
            raise ValueError(f"{what}: y_len must lie in 1..{M}")
        raise ValueError(f"{what}: non-finite coordinate in the input")
    return x, y, lens


def _nearest_ragged(x, y, lens, active, dist2, idx, keys):
    B, N, M = int(x.shape[0]), int(x.shape[1]), int(y.shape[1])
    L.call("moda_nn_fwd_ragged", L.ptr(x), L.ptr(y), B, N, M, L.ptr(lens), L.ptr(active), L.ptr(dist2), L.ptr(idx), L.ptr(keys),
           L.stream())


def _nn_workspace(B, N, M, dev):
    return (torch.empty((B, N), dtype=torch.float32, device=dev), torch.empty((B, N), dtype=torch.int32, device=dev),
            torch.empty((B, N), dtype=torch.int64, device=dev) if nn_plan(B, N, M)[0] > 1 else None)


def _icp_solve(sums, n, estimate_scale=False, allow_reflection=False, sweeps=0, active=None, out=None):
    """moda_icp_solve: sums (B,17) float64 device over n correspondences -> rts (B,13) fp32 = R row-major, T, s: mesh_eval._align
    on the device (one-sided Jacobi SVD; sweeps = 0: the library's fixed count)."""
    B = int(sums.shape[0])
    rts = torch.zeros((B, 13), dtype=torch.float32, device=sums.device) if out is None else out
    L.call("moda_icp_solve", L.ptr(sums), B, int(n), int(bool(estimate_scale)), int(bool(allow_reflection)), int(sweeps),
           L.ptr(active), L.ptr(rts), L.stream())
    return rts


@torch.no_grad()
def iterative_closest_point_device(X, Y, y_len=None, init_transform=None, max_iterations=100, relative_rmse_thr=1e-6,
                                   estimate_scale=False, allow_reflection=False, per_element=False, check_every=0,
                                   keep_history=False):
    """iterative_closest_point with nothing read back inside the loop: the alignment (moda_icp_solve) and the stopping rule
    (moda_icp_advance) run on the device, six entry calls per iteration on the current stream.
    X (B,N,3); Y (B,M_max,3) with y_len (B,) | None: cloud b's targets are Y[b, :y_len[b]], the rows behind them are never read.
    per_element: a cloud stops the moment it has converged itself, so it gets exactly what a batch of one gives it; otherwise
    pytorch3d's rule, as in iterative_closest_point: everybody iterates until all have converged in the same iteration.
    check_every = 0: all max_iterations rounds are issued -- a stopped cloud costs launches that return at once -- and nothing
    is read back, so the call can be captured with torch.cuda.graph (on a capturing stream the input check, a read-back, is
    skipped: the caller vouches for finite coordinates and lengths in 1..M_max).  check_every = k: one int32 ("is anyone still
    active") is read every k iterations and the loop ends early; the results are the same bits.
    -> ICPSolutionDevice(converged (B,) bool, rmse (B,), Xt, SimilarityTransform(R, T, s), t_history | None (keep_history)),
    with .iterations (B,) int32 and .idx (B,N) int32."""
    what = "iterative_closest_point_device"
    x0, y, lens = _ragged_clouds(X, Y, y_len, what)
    B, N, M = int(x0.shape[0]), int(x0.shape[1]), int(y.shape[1])
    if max_iterations < 1:
        raise ValueError(f"{what}: max_iterations must be at least 1")
    if check_every < 0:
        raise ValueError(f"{what}: check_every must be 0 (never) or a positive period")
    dev = x0.device
    rts = torch.zeros((B, 13), dtype=torch.float32, device=dev)
    xt = torch.empty_like(x0)
    if init_transform is not None:
        try:
            R0, T0, s0 = (torch.as_tensor(v).detach().to(device=dev, dtype=torch.float32) for v in init_transform)
        except Exception:
            raise ValueError("init_transform must be a SimilarityTransform (R (B,3,3), T (B,3), s (B,))")
        if tuple(R0.shape) != (B, 3, 3) or tuple(T0.shape) != (B, 3) or tuple(s0.shape) != (B,):
            raise ValueError(f"init_transform shapes {tuple(R0.shape)}, {tuple(T0.shape)}, {tuple(s0.shape)} do not match a batch of {B}")
        rts.copy_(torch.cat([R0.reshape(B, 9), T0, s0[:, None]], 1))
        L.call("moda_sim3_apply", L.ptr(x0), L.ptr(rts), B, N, L.ptr(xt), L.stream())
    else:
        rts[:, 0] = rts[:, 4] = rts[:, 8] = rts[:, 12] = 1.0
        xt.copy_(x0)
    active = torch.ones(B, dtype=torch.int32, device=dev)
    iterations = torch.zeros(B, dtype=torch.int32, device=dev)
    converged = torch.zeros(B, dtype=torch.int32, device=dev)
    flags = torch.ones(1, dtype=torch.int32, device=dev)
    prev = torch.zeros(B, dtype=torch.float64, device=dev)
    rmse = torch.zeros(B, dtype=torch.float32, device=dev)
    sums = torch.zeros((B, _NSUM), dtype=torch.float64, device=dev)
    partials = torch.empty((B, _ICP_MAX_BLOCKS, _NSUM), dtype=torch.float64, device=dev)
    dist2, idx, keys = _nn_workspace(B, N, M, dev)
    idx.zero_()
    history = [] if keep_history else None
    st = L.stream()
    for it in range(int(max_iterations)):
        _nearest_ragged(xt, y, lens, active, dist2, idx, keys)
        L.call("moda_icp_moments_ragged", L.ptr(x0), L.ptr(y), L.ptr(idx), None, B, N, M, L.ptr(lens), L.ptr(active),
               L.ptr(partials), L.ptr(sums), st)
        _icp_solve(sums, N, estimate_scale, allow_reflection, active=active, out=rts)
        L.call("moda_sim3_apply_masked", L.ptr(x0), L.ptr(rts), B, N, L.ptr(active), L.ptr(xt), st)
        L.call("moda_icp_moments_ragged", None, L.ptr(y), L.ptr(idx), L.ptr(xt), B, N, M, L.ptr(lens), L.ptr(active),
               L.ptr(partials), L.ptr(sums), st)
        L.call("moda_icp_advance", L.ptr(sums), B, N, float(relative_rmse_thr), int(bool(per_element)), L.ptr(prev), L.ptr(rmse),
               L.ptr(iterations), L.ptr(converged), L.ptr(active), L.ptr(flags), st)
        if keep_history:
            history.append(SimilarityTransform(rts[:, :9].reshape(B, 3, 3).clone(), rts[:, 9:12].clone(), rts[:, 12].clone()))
        if check_every and (it + 1) % check_every == 0 and not int(flags[0]):  # the one int32 read every check_every rounds
            break
    sol = ICPSolutionDevice(converged.bool(), rmse, xt,
                            SimilarityTransform(rts[:, :9].reshape(B, 3, 3).clone(), rts[:, 9:12].clone(), rts[:, 12].clone()), history)
    sol.iterations, sol.idx = iterations, idx
    return sol


class SequenceEval:
    """What eval_sequence returns, all device tensors: cd, f001, f002, f005 (F,) float64, iterations (F,) int32, converged (F,)
    bool, fitted_scale, bbox_max (F,) fp32, verts (F,V,3) the registered prediction, and metrics (F,10): cd, the three F-scores,
    then (precision_1, precision_2) at each threshold."""

    def __init__(self, metrics, iterations, converged, fitted_scale, bbox_max, verts):
        self.metrics, self.iterations, self.converged = metrics, iterations, converged
        self.fitted_scale, self.bbox_max, self.verts = fitted_scale, bbox_max, verts
        self.cd, self.f001, self.f002, self.f005 = (metrics[:, k] for k in range(4))

    def __len__(self):
        return int(self.metrics.shape[0])

    def summary(self):
        """The figures render_vis.py:513-525 prints: cd_ave, cd_max and ave / min of each F-score, as floats (one read-back)."""
        m = self.metrics[:, :4]
        cd, f1, f2, f5 = torch.stack([m.mean(0), m.max(0)[0], m.min(0)[0]]).cpu().numpy().T.tolist()
        return dict(cd_ave=cd[0], cd_max=cd[1], f001_ave=f1[0], f001_min=f1[2], f002_ave=f2[0], f002_min=f2[2],
                    f005_ave=f5[0], f005_min=f5[2])


def _sequence_gt(verts_gt, gt_lens, dev, F):
    """-> gt (F,M_max,3) fp32 device, lens (F,) | None.  A list is padded on upload with copies of each frame's first vertex."""
    if torch.is_tensor(verts_gt):
        return verts_gt, gt_lens
    if gt_lens is not None:
        raise ValueError("eval_sequence: gt_lens goes with a padded (F,M_max,3) tensor, not with a list")
    items = []
    for g in verts_gt:
        if hasattr(g, "vertices_t"):
            g = g.vertices_t
        elif not torch.is_tensor(g):
            g = torch.as_tensor(np.asarray(getattr(g, "vertices", g), np.float32))
        if g.dim() != 2 or g.shape[-1] != 3:
            raise ValueError(f"eval_sequence: a ground-truth frame has shape {tuple(g.shape)}, expected (M,3)")
        if g.shape[0] < 1:
            raise ValueError("eval_sequence: a ground-truth cloud is empty")
        if g.requires_grad:
            raise NotImplementedError("eval_sequence has no backward: detach its inputs")
        items.append(g)
    if len(items) != F:
        raise ValueError(f"eval_sequence: {len(items)} ground-truth frames for {F} predicted frames")
    lens = [int(g.shape[0]) for g in items]
    gt = torch.empty((F, max(lens), 3), dtype=torch.float32, device=dev)
    for f, g in enumerate(items):
        gt[f, :lens[f]] = g.to(device=dev, dtype=torch.float32)
        gt[f, lens[f]:] = gt[f, 0]
    return gt, (None if min(lens) == max(lens) else lens)


@torch.no_grad()
def eval_sequence(verts, verts_gt, gt_lens=None):
    """eval_mesh for every frame of a sequence at once (render_vis.py:346-417 per frame, :513-525 over the sequence), nothing
    read back but the input check.  verts (F,V,3) device tensor or a MeshSequence; verts_gt (F,M,3), or a list of (M_f,3)
    arrays / tensors / TriMesh objects (padded on upload), or (F,M_max,3) with gt_lens (F,): frame f's ground truth is
    verts_gt[f, :gt_lens[f]].  Per frame: bbox_max and the lower-median depth ratio over the valid rows, ICP with
    per_element=True (no scale, 100 iterations), the Chamfer pass and the metrics row of moda_seq_metrics.  Frame f gets what
    eval_mesh(verts[f], verts_gt[f]) gets, up to the last bits of the 3 x 3 SVD.  -> SequenceEval."""
    what = "eval_sequence"
    if hasattr(verts, "verts") and not torch.is_tensor(verts):
        verts = verts.verts
    if not torch.is_tensor(verts) or verts.dim() != 3 or verts.shape[-1] != 3:
        raise ValueError(f"{what} takes (F,V,3) vertices or a MeshSequence, got {type(verts).__name__}"
                         + (f" {tuple(verts.shape)}" if torch.is_tensor(verts) else ""))
    if not verts.is_cuda:
        raise RuntimeError("moda_amd ops take CUDA (ROCm) tensors; the HIP library is the only compute path")
    F, V = int(verts.shape[0]), int(verts.shape[1])
    gt, gt_lens = _sequence_gt(verts_gt, gt_lens, verts.device, F)
    v, gt, lens = _ragged_clouds(verts, gt, gt_lens, what)                    # the finite check, once for the batch
    M = int(gt.shape[1])
    dev = v.device
    valid = (torch.arange(M, device=dev)[None, :] < lens[:, None])[..., None]
    inf = torch.full((), float("inf"), device=dev)
    bbox_max = (torch.where(valid, gt, -inf).max(1)[0] - torch.where(valid, gt, inf).min(1)[0]).max(1)[0].contiguous()   # :379
    gz = torch.where(valid[..., 0], gt[..., 2], inf).sort(1)[0]
    gt_med = gz.gather(1, ((lens.long() - 1) // 2)[:, None])[:, 0]            # torch.median: the lower median
    fitted_scale = gt_med / v[..., 2].median(1)[0]                            # :387
    v = v * fitted_scale[:, None, None]
    icp = iterative_closest_point_device(v, gt, lens, estimate_scale=False, max_iterations=100, per_element=True)   # :390-391
    v = icp.Xt
    d_gt, i_gt, keys = _nn_workspace(F, M, V, dev)                            # :399, gt -> pred: the padding rows search too,
    L.call("moda_nn_fwd", L.ptr(gt), L.ptr(v), F, M, V, L.ptr(d_gt), L.ptr(i_gt), L.ptr(keys), L.stream())   # and are not counted
    d_pred, i_pred, keys = _nn_workspace(F, V, M, dev)
    _nearest_ragged(v, gt, lens, None, d_pred, i_pred, keys)
    metrics = torch.empty((F, _NMETRIC), dtype=torch.float64, device=dev)
    L.call("moda_seq_metrics", L.ptr(d_gt), L.ptr(d_pred), F, M, V, L.ptr(lens), L.ptr(bbox_max), L.ptr(metrics),
           L.stream())
    return SequenceEval(metrics, icp.iterations, icp.converged, fitted_scale, bbox_max, v)
