"""float64 numpy restatement of the debiased Sinkhorn divergence as geomloss 0.2.4 computes it on its tensorized route
(SamplesLoss("sinkhorn", p=2, blur, scaling, reach=None, debias=True, potentials=False), uniform weights), the call of
nnutils/moda.py:693-695.  geomloss is not part of the reference tree: this follows its published sinkhorn_divergence.py and is
unpinned.  Plain loops over the schedule and materialised matrices -- nothing of the kernel's structure.

`sinkdiv_torch` is the same arithmetic in torch (any dtype) with geomloss' detach pattern, for autograd and for measuring what
fp32 itself loses."""
import numpy as np


def max_diameter(x, y):
    pts = np.concatenate([x, y], 0)
    return float(np.linalg.norm(pts.max(0) - pts.min(0)))


def epsilon_schedule(d, blur, scaling, p=2):
    mid = [float(np.exp(e)) for e in np.arange(p * np.log(d), p * np.log(blur), p * np.log(scaling))]
    return [d ** p] + mid + [blur ** p]


def cost(u, v):
    diff = u[:, None, :] - v[None, :, :]
    return (diff ** 2).sum(-1) / 2


def softmax_rows(z):
    """(logsumexp over the columns, softmax weights) of the rows of z."""
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(1, keepdims=True)
    return (m + np.log(s))[:, 0], e / s


def softmin(eps, C, h):
    return -eps * softmax_rows(h[None, :] - C / eps)[0]


def sinkdiv(x, y, blur=0.05, scaling=0.5, diameter=None):
    """-> dict(loss, grad_x, grad_y, a_x, b_x, a_y, b_y, d, n, eps) in float64."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    N, M = len(x), len(y)
    la, lb = np.full(N, -np.log(N)), np.full(M, -np.log(M))
    d = max_diameter(x, y) if diameter is None else float(diameter)
    eps_s = epsilon_schedule(d, blur, scaling)
    C_xx, C_yy, C_xy, C_yx = cost(x, x), cost(y, y), cost(x, y), cost(y, x)
    eps = eps_s[0]
    a_x, b_y = softmin(eps, C_xx, la), softmin(eps, C_yy, lb)
    a_y, b_x = softmin(eps, C_yx, la), softmin(eps, C_xy, lb)
    for eps in eps_s:
        at_x = softmin(eps, C_xx, la + a_x / eps)
        bt_y = softmin(eps, C_yy, lb + b_y / eps)
        at_y = softmin(eps, C_yx, la + b_x / eps)
        bt_x = softmin(eps, C_xy, lb + a_y / eps)
        a_x, b_y, a_y, b_x = 0.5 * (a_x + at_x), 0.5 * (b_y + bt_y), 0.5 * (a_y + at_y), 0.5 * (b_x + bt_x)
    eps = eps_s[-1]
    lse_ax, v = softmax_rows((la + a_x / eps)[None, :] - C_xx / eps)
    lse_by, vy = softmax_rows((lb + b_y / eps)[None, :] - C_yy / eps)
    lse_ay, wy = softmax_rows((la + b_x / eps)[None, :] - C_yx / eps)
    lse_bx, w = softmax_rows((lb + a_y / eps)[None, :] - C_xy / eps)
    a_x, b_y, a_y, b_x = -eps * lse_ax, -eps * lse_by, -eps * lse_ay, -eps * lse_bx
    loss = (b_x - a_x).mean() + (a_y - b_y).mean()
    # the envelope gradient through the row point of the last extrapolation
    gx = ((w[:, :, None] * (x[:, None, :] - y[None, :, :])).sum(1) - (v[:, :, None] * (x[:, None, :] - x[None, :, :])).sum(1)) / N
    gy = ((wy[:, :, None] * (y[:, None, :] - x[None, :, :])).sum(1) - (vy[:, :, None] * (y[:, None, :] - y[None, :, :])).sum(1)) / M
    return dict(loss=float(loss), grad_x=gx, grad_y=gy, a_x=a_x, b_x=b_x, a_y=a_y, b_y=b_y, d=d, n=len(eps_s), eps=eps_s)


def sinkdiv_torch(x, y, blur=0.05, scaling=0.5, diameter=None):
    """The same in torch, in the dtype of x, with geomloss' pattern: the loop runs without gradients, the last extrapolation with
    them, the column cloud of every cost matrix detached; the diameter leaves the tensor as a Python float (`.item()`).
    -> (loss 0-d tensor, attached to x and y; dict(P = largest |final potential|, n))."""
    import torch

    def tcost(u, v):
        return ((u[:, None, :] - v[None, :, :]) ** 2).sum(-1) / 2

    def tsoftmin(eps, C, h):
        return -eps * (h[None, :] - C / eps).logsumexp(1)

    N, M = x.shape[0], y.shape[0]
    la = torch.full((N,), 1.0 / N, dtype=x.dtype, device=x.device).log()
    lb = torch.full((M,), 1.0 / M, dtype=x.dtype, device=x.device).log()
    if diameter is None:
        pts = torch.cat([x, y], 0).detach()
        diameter = (pts.max(0).values - pts.min(0).values).norm().item()
    eps_s = epsilon_schedule(diameter, blur, scaling)
    C_xx, C_yy, C_xy, C_yx = tcost(x, x.detach()), tcost(y, y.detach()), tcost(x, y.detach()), tcost(y, x.detach())
    with torch.no_grad():
        eps = eps_s[0]
        a_x, b_y = tsoftmin(eps, C_xx, la), tsoftmin(eps, C_yy, lb)
        a_y, b_x = tsoftmin(eps, C_yx, la), tsoftmin(eps, C_xy, lb)
        for eps in eps_s:
            at_x = tsoftmin(eps, C_xx, la + a_x / eps)
            bt_y = tsoftmin(eps, C_yy, lb + b_y / eps)
            at_y = tsoftmin(eps, C_yx, la + b_x / eps)
            bt_x = tsoftmin(eps, C_xy, lb + a_y / eps)
            a_x, b_y, a_y, b_x = 0.5 * (a_x + at_x), 0.5 * (b_y + bt_y), 0.5 * (a_y + at_y), 0.5 * (b_x + bt_x)
    eps = eps_s[-1]
    a_x, b_y, a_y, b_x = (tsoftmin(eps, C_xx, (la + a_x / eps).detach()), tsoftmin(eps, C_yy, (lb + b_y / eps).detach()),
                          tsoftmin(eps, C_yx, (la + b_x / eps).detach()), tsoftmin(eps, C_xy, (lb + a_y / eps).detach()))
    loss = (b_x - a_x).mean() + (a_y - b_y).mean()
    P = max(float(t.detach().abs().max()) for t in (a_x, b_y, a_y, b_x))
    return loss, dict(P=P, n=len(eps_s))


# ---- the test family: the reference's geometry (bones inside a squashed sphere of surface samples), scaled by 10 --------------
def squashed_sphere(rng, M, radius=(0.3, 0.2, 0.25), centre=(0.0, 0.0, 0.0)):
    v = rng.standard_normal((M, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * np.asarray(radius) + np.asarray(centre)) * 10


def gaussian_bones(rng, N, sigma=0.1, centre=(0.0, 0.0, 0.0)):
    return (rng.standard_normal((N, 3)) * sigma + np.asarray(centre)) * 10


def frac_log2(d, blur=0.05):
    t = np.log2(d / blur)
    return float(t - np.floor(t))


def with_diameter(x, y, target, blur=0.05):
    """Scale both clouds about the origin so that their joint box diagonal is `target`."""
    s = target / max_diameter(x, y)
    return x * s, y * s
