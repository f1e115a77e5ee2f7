"""Float64 numpy oracle for the whole-sequence route of moda_amd/mesh_eval.py (not a test): the ragged nearest search, the
Umeyama solve from the 17 sums with np.linalg.svd, ICP over a batch under the per-element and the all-element stopping rule,
and the per-frame metrics row with the sequence summary.  Built on tests/pointset_numpy.py; inputs are fp32 values widened to
float64, every result is float64."""
import numpy as np

import pointset_numpy as psn


def nearest_ragged(x, y, y_len, with_second=False):
    """x (B,N,3), y (B,M_max,3), y_len (B,) -> per cloud the search over y[b, :y_len[b]] only: lists of psn.nearest results."""
    return [psn.nearest(x[b], y[b][:int(y_len[b])], with_second=with_second) for b in range(len(x))]


def moments(X, Yn, Xt=None):
    """The 17 sums of moda_icp_moments for one cloud: sum x, sum yn, sum x (x) yn, sum |x|^2, sum |xt - yn|^2."""
    X, Yn = np.asarray(X, np.float64), np.asarray(Yn, np.float64)
    res = 0.0 if Xt is None else ((np.asarray(Xt, np.float64) - Yn) ** 2).sum()
    return np.concatenate([X.sum(0), Yn.sum(0), (X.T @ Yn).reshape(-1), [(X * X).sum()], [res]])


def solve(sums, n, estimate_scale=False, allow_reflection=False):
    """Umeyama's similarity from the sums of one cloud (row vectors: s * X @ R + T) -> R, T, s, and the singular values."""
    sums = np.asarray(sums, np.float64)
    mx, my = sums[0:3] / n, sums[3:6] / n
    C = sums[6:15].reshape(3, 3) / n - np.outer(mx, my)
    U, S, Vt = np.linalg.svd(C)
    E = np.ones(3)
    if not allow_reflection:
        E[2] = np.linalg.det(U @ Vt)
    R = (U * E) @ Vt
    s = float((S * E).sum() / (sums[15] / n - mx @ mx)) if estimate_scale else 1.0
    return R, my - s * mx @ R, s, S


def icp_batch(X, Y, y_len=None, per_element=False, max_iterations=100, relative_rmse_thr=1e-6, estimate_scale=False,
              allow_reflection=False):
    """X (B,N,3); Y (B,M_max,3) or a list of (M_b,3); y_len (B,) | None.  per_element: a cloud stops when it has converged
    itself; else nobody stops until all have converged in the same iteration.  -> dict of per-cloud lists: R, T, s, Xt, rmse,
    iterations, converged, idx."""
    B = len(X)
    Ys = [np.asarray(Y[b], np.float64)[:(len(Y[b]) if y_len is None else int(y_len[b]))] for b in range(B)]
    Xs = [np.asarray(X[b], np.float64) for b in range(B)]
    n = len(Xs[0])
    out = dict(R=[np.eye(3)] * B, T=[np.zeros(3)] * B, s=[1.0] * B, Xt=[x.copy() for x in Xs], rmse=[0.0] * B,
               iterations=[0] * B, converged=[False] * B, idx=[None] * B)
    active, prev = [True] * B, [None] * B
    for _ in range(max_iterations):
        verdict = {}
        for b in range(B):
            if not active[b]:
                continue
            _, idx = psn.nearest(out["Xt"][b], Ys[b])
            Yn = Ys[b][idx]
            R, T, s, _ = solve(moments(Xs[b], Yn), n, estimate_scale, allow_reflection)
            Xt = s * Xs[b] @ R + T
            rmse = np.sqrt(((Xt - Yn) ** 2).sum() / n)
            rel = 1.0 if prev[b] is None else ((prev[b] - rmse) / prev[b] if prev[b] > 0 else 0.0)
            prev[b] = rmse
            out["R"][b], out["T"][b], out["s"][b], out["Xt"][b], out["rmse"][b], out["idx"][b] = R, T, s, Xt, rmse, idx
            out["iterations"][b] += 1
            verdict[b] = rel <= relative_rmse_thr
        if per_element:
            for b, conv in verdict.items():
                out["converged"][b], active[b] = conv, not conv
        elif all(verdict.values()):
            for b in verdict:
                out["converged"][b], active[b] = True, False
        if not any(active):
            break
    return out


def metrics_row(d_gt, d_back, bbox_max):
    """Squared distances gt -> pred (G,), pred -> gt (V,) -> [cd, f001, f002, f005, (p1, p2) x 3] and the thresholds."""
    d_gt, d_back = np.asarray(d_gt, np.float64), np.asarray(d_back, np.float64)
    row, thresholds = [np.sqrt(d_gt).mean() + np.sqrt(d_back).mean()], []
    pairs = []
    for frac in (0.01, 0.02, 0.05):
        thr = (bbox_max * frac) ** 2
        f, p1, p2 = psn.fscore(d_gt[None], d_back[None], thr)
        row.append(float(f[0]))
        pairs += [float(p1[0]), float(p2[0])]
        thresholds.append(thr)
    return np.array(row + pairs), thresholds


def fitted_scale(verts, verts_gt):
    """The ratio of the lower medians of the depths, ground truth over prediction (render_vis.py:387)."""
    def lower_median(a):
        return np.sort(a)[(len(a) - 1) // 2]
    return float(lower_median(np.asarray(verts_gt, np.float64)[:, 2]) / lower_median(np.asarray(verts, np.float64)[:, 2]))


def eval_sequence(verts, gts):
    """verts (F,V,3), gts: a list of (M_f,3) -> per-frame dicts of psn.eval_mesh plus `row`, and the summary of the sequence."""
    frames = []
    for v, g in zip(verts, gts):
        e = psn.eval_mesh(v, g)
        e["row"], _ = metrics_row(e["d_gt"], e["d_back"], e["bbox_max"])
        e["fitted_scale"] = fitted_scale(v, g)
        frames.append(e)
    return frames, summary([f["row"] for f in frames])


def summary(rows):
    r = np.asarray(rows, np.float64)
    out = dict(cd_ave=r[:, 0].mean(), cd_max=r[:, 0].max())
    for k, key in enumerate(("f001", "f002", "f005")):
        out[key + "_ave"], out[key + "_min"] = r[:, 1 + k].mean(), r[:, 1 + k].min()
    return out
