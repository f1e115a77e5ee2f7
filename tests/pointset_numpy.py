"""Float64 numpy oracle for moda_amd/mesh_eval.py (not a test): brute-force nearest neighbour with the lowest-index tie rule,
the Chamfer gradients, ICP as moda_amd.mesh_eval.iterative_closest_point's docstring states it, fscore and eval_mesh.  Inputs
are fp32 values widened to float64, so the oracle sees exactly the numbers the kernels see; every result is float64."""
from collections import namedtuple

import numpy as np

SimilarityTransform = namedtuple("SimilarityTransform", "R T s")
ICPSolution = namedtuple("ICPSolution", "converged rmse Xt RTs t_history idx")


def dist2_matrix(x, y):
    """(n,3), (m,3) -> (n,m) squared distances from differences."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    d = x[:, None, 0] - y[None, :, 0]
    out = d * d
    for c in (1, 2):
        d = x[:, None, c] - y[None, :, c]
        out += d * d
    return out


def nearest(x, y, chunk=None, with_second=False):
    """(N,3), (M,3) -> dist2 (N,), idx (N,) int64: np.argmin returns the FIRST minimum, the lowest-index tie rule.
    with_second: also the second-smallest distance of each query (inf when M == 1)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n, m = len(x), len(y)
    chunk = chunk or max(1, int(4e6 // max(m, 1)))
    d2, idx, second = np.empty(n), np.empty(n, np.int64), np.full(n, np.inf)
    for a in range(0, n, chunk):
        D = dist2_matrix(x[a:a + chunk], y)
        i = D.argmin(1)
        r = np.arange(len(i))
        idx[a:a + chunk], d2[a:a + chunk] = i, D[r, i]
        if with_second and m > 1:
            D[r, i] = np.inf
            second[a:a + chunk] = D.min(1)
    return (d2, idx, second) if with_second else (d2, idx)


def chamfer(x, y):
    d1, i1 = nearest(x, y)
    d2, i2 = nearest(y, x)
    return d1, d2, i1, i2


def chamfer_grad(x, y, i1, i2, g1, g2):
    """Gradients of sum(g1 * dist1) + sum(g2 * dist2) for fixed correspondences, and per element the sum of |terms| and the
    number of terms (for rounding bounds): -> gx, gy, abs_x, abs_y, count_x, count_y."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    gx, gy = np.zeros_like(x), np.zeros_like(y)
    ax, ay = np.zeros_like(x), np.zeros_like(y)
    cx, cy = np.zeros(len(x), np.int64), np.zeros(len(y), np.int64)
    for p, q, i, g, gp, gq, ap, aq, cp, cq in ((x, y, i1, g1, gx, gy, ax, ay, cx, cy), (y, x, i2, g2, gy, gx, ay, ax, cy, cx)):
        v = 2.0 * np.asarray(g, np.float64)[:, None] * (p - q[i])
        gp += v
        ap += np.abs(v)
        cp += 1
        np.add.at(gq, i, -v)
        np.add.at(aq, i, np.abs(v))
        np.add.at(cq, i, 1)
    return gx, gy, ax, ay, cx, cy


def fscore(dist1, dist2, threshold=0.001):
    """(B,N), (B,M) squared distances -> fscore, precision_1, precision_2, each (B,); 0/0 is 0."""
    p1 = (np.asarray(dist1) < threshold).mean(1)
    p2 = (np.asarray(dist2) < threshold).mean(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = 2 * p1 * p2 / (p1 + p2)
    f[np.isnan(f)] = 0
    return f, p1, p2


def align(X, Yn, estimate_scale=False, allow_reflection=False):
    """The similarity mapping X onto Yn (row vectors: s * X @ R + T), Umeyama's solution."""
    n = len(X)
    mx, my = X.mean(0), Yn.mean(0)
    Xc, Yc = X - mx, Yn - my
    C = Xc.T @ Yc / n
    U, S, Vt = np.linalg.svd(C)
    E = np.ones(3)
    if not allow_reflection:
        E[2] = np.linalg.det(U @ Vt)
    R = (U * E) @ Vt
    s = (S * E).sum() / ((Xc * Xc).sum() / n) if estimate_scale else 1.0
    T = my - s * mx @ R
    return R, T, s


def iterative_closest_point(X, Y, init_transform=None, max_iterations=100, relative_rmse_thr=1e-6, estimate_scale=False,
                            allow_reflection=False):
    """One batch element: X (N,3), Y (M,3).  idx in the result is the last iteration's correspondence."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    R, T, s = (np.eye(3), np.zeros(3), 1.0) if init_transform is None else init_transform
    Xt = s * X @ R + T
    prev, converged, hist, idx, rmse = None, False, [], None, 0.0
    for _ in range(max_iterations):
        _, idx = nearest(Xt, Y)
        Yn = Y[idx]
        R, T, s = align(X, Yn, estimate_scale, allow_reflection)
        Xt = s * X @ R + T
        rmse = np.sqrt(((Xt - Yn) ** 2).sum(1).mean())
        relative = 1.0 if prev is None else ((prev - rmse) / prev if prev > 0 else 0.0)
        hist.append(SimilarityTransform(R, T, s))
        prev = rmse
        if relative <= relative_rmse_thr:
            converged = True
            break
    return ICPSolution(converged, rmse, Xt, hist[-1], hist, idx)


def eval_mesh(verts, verts_gt):
    """(V,3), (G,3) -> dict with cd, f001, f002, f005, the squared distances d_gt (G,), d_back (V,), the thresholds, icp."""
    v, gt = np.asarray(verts, np.float64), np.asarray(verts_gt, np.float64)
    bbox_max = float((gt.max(0) - gt.min(0)).max())

    def lower_median(a):
        return np.sort(a)[(len(a) - 1) // 2]
    v = v * (lower_median(gt[:, 2]) / lower_median(v[:, 2]))
    icp = iterative_closest_point(v, gt, estimate_scale=False, max_iterations=100)
    v = icp.Xt
    d_gt, d_back, _, _ = chamfer(gt, v)
    out = dict(bbox_max=bbox_max, d_gt=d_gt, d_back=d_back, icp=icp, verts=v, thresholds={})
    for key, frac in (("f001", 0.01), ("f002", 0.02), ("f005", 0.05)):
        thr = (bbox_max * frac) ** 2
        out[key] = float(fscore(d_gt[None], d_back[None], thr)[0][0])
        out["thresholds"][key] = thr
    out["cd"] = float(np.sqrt(d_gt).mean() + np.sqrt(d_back).mean())
    return out


# ---- the known-motion construction of the ICP tests ----------------------------------------------------------------------
def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(degrees)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def icp_case(seed, degrees, scale=1.0, n_y=3000, n_x=1500):
    """Y: n_y points u * (0.30, 0.18, 0.11) * (1 + 0.25 sin(5 u_x) cos(3 u_y)) for random unit vectors u; X: a random subset
    of n_x of them moved by the inverse of (R, T, scale), then rounded to fp32 -- so s * X @ R + T returns to Y[subset] up
    to that rounding.  -> X, Y (fp32), subset, R, T (float64; row-vector convention)."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n_y, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    Y = (u * np.array([0.30, 0.18, 0.11]) * (1 + 0.25 * np.sin(5 * u[:, :1]) * np.cos(3 * u[:, 1:2]))).astype(np.float32)
    subset = rng.permutation(n_y)[:n_x]
    R = rotation((1, 2, 3), degrees)
    T = rng.uniform(-0.05, 0.05, 3)
    X = ((Y[subset].astype(np.float64) - T) @ R.T / scale).astype(np.float32)
    return X, Y, subset, R, T
