"""Restatement of the warm-up stages (moda_amd/warmup.py, csrc/warmup_kernels.hip; the reference's shape_init_loss, rtk_loss,
compute_root_sm_loss, rot_angle and pytorch3d's matrix_to_quaternion) in numpy: float64 with gradients, and fp32 in the reference's
operation order, with the fp32 error bounds the tests hold the kernels (and the reference's own fp32 records) to.  Every function
returns a dict of values and a dict of bounds with the same keys; the float64 form (dtype=np.float64) reads the fp32 inputs
exactly, so its own error (~1e-15) is ignored.

Bounds (u = 2^-24, gamma_n = n u / (1 - n u)); each covers ANY order of the sums it names, so one bound serves the kernels' fixed
trees and torch's vectorised CPU sums:
  * pts = (u * 2) * b - b with b = obj_bound * bound_factor: three separately rounded fp32 operations that numpy's element-wise
    arithmetic reproduces bit for bit.  Bound 0.
  * dis, ellipsoid.  q_k = p_k / o_k (u), its square (3 u), the sum of three positive terms (2 more): s carries gamma_5, r = sqrt(s)
    gamma_5 / 2 + u <= gamma_4.  r - 1 adds u |r - 1|, the mean of the bound gamma_3 (two additions, one division), the product u:
    |err| <= gamma_4 r mean + gamma_6 |dis|.  Sphere: s carries gamma_3 (no division), r gamma_3: |err| <= gamma_3 r + gamma_2 |dis|.
  * shape loss.  r_i = fl(-y_i - dis_i) (u), its square (3 u), the mean's division (u) and, for an fp32 sum of N positive terms
    in any order, gamma_{N-1}: |err| <= gamma_{N+4} loss.  dy_i = -((g / N) (2 r_i)): gamma_4 |dy_i|.
  * rot_angle.  tr is nine products and eight additions: e_tr = gamma_10 S, S = sum |X_ik Y_ik|; cos = (tr - 1) / 2:
    e_cos = (e_tr + u |tr - 1|) / 2 + u, the last u for the clamp bounds, which fp32 holds rounded.  acos o clamp is Lipschitz with
    the constant D = max 1 / sqrt(1 - c^2) over the part of [c - e_cos, c + e_cos] inside the clamp (D <= 70.8 at the bounds);
    acosf itself is taken as 4 u angle: e_angle = D e_cos + 4 u angle.
    Its derivative -1 / sqrt(1 - c^2) changes by at most e_cos |c| / (1 - c^2)^(3/2) (at the interval's far end) plus gamma_5 of
    itself; where the interval straddles a clamp bound the gradient may be on or off: the bound is then D itself.
  * rtk_loss.  rot_loss = 0.01 mean angle: 0.01 mean e_angle + gamma_{T+3} |rot_loss|.  trn_loss: differences (u), squares, sums:
    gamma_{T+6} trn_loss.  dR = gc Rg with gc = g 0.01 / T * dangle / 2: |Rg| (|k| e_dangle + gamma_6 |gc|).  dt = (g / T) 2 (tp - tg):
    gamma_5 |dt|.
  * compute_root_sm_loss over P pooled pairs.  |t_i - t_{i+1}| carries gamma_4 (as r above).  loss: 1e-3 mean e_angle +
    0.1 gamma_4 mean trn + gamma_{P+4} |loss|.  A frame's gradient sums its pairs: dR: sum |R_other| (|k| e_dangle + gamma_6 |gc|)
    + gamma_2 |dR|; dt: gamma_12 sum |terms|, and exactly 0 where the difference is zero.
  * matrix_to_quaternion, round trip.  The input is a rotation rounded to fp32: |E_ij| <= u.  The candidate 4 q_k q is linear in
    the entries: its diagonal component moves by at most 3 u, the others by 2 u, |.|_2 <= sqrt(9 + 12) u = 4.59 u; 4 q_k >= 2, and
    normalising does not enlarge an error: e_q <= 2.3 u (float64).  fp32 arithmetic adds gamma_3 (1 + |r00| + |r11| + |r22|) <= 12 u
    on the diagonal component and 2 u on the others, |.|_2 <= 12.5 u, halved, plus gamma_6 for the normalisation:
    e_q <= (4.59 + 12.5) / 2 u + 6 u = 14.6 u.  Every entry of quaternion_to_matrix has a gradient of norm <= 4 in q:
    |R' - R| <= 4 e_q + u.
"""
import numpy as np

U32 = 2.0 ** -24
EPS = 1e-4
ROUNDTRIP_F64 = (4 * 4.59 / 2 + 1) * U32
ROUNDTRIP_F32 = (4 * ((4.59 + 12.5) / 2 + 6) + 1) * U32


def gamma(n):
    return n * U32 / (1 - n * U32)


# ---- shape initialisation -------------------------------------------------------------------------------------------------------
def shape_target(u, obj_bound, bound_factor, ellips, dtype=np.float64, wide_pts=False):
    """u (N,3) fp32, obj_bound (3,) fp32 -> ({pts (N,3) fp32, dis (N,)}, bounds).  wide_pts: the points themselves in `dtype`, as a
    float64 run of the reference forms them (they then differ from the fp32 points, and dis with them)."""
    u, ob = np.asarray(u, np.float32), np.asarray(obj_bound, np.float32)
    b = ob * np.float32(bound_factor)
    pts = (u * np.float32(2)) * b - b
    if wide_pts:
        bw = ob.astype(dtype) * dtype(bound_factor)
        pts = (u * np.float32(2)).astype(dtype) * bw - bw
    p, o = pts.astype(dtype), ob.astype(dtype)
    if ellips:
        q = p / o
        r = np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
        mean = ((o[0] + o[1]) + o[2]) / dtype(3)
        dis = (r - dtype(1)) * mean
        bound = gamma(4) * r * float(mean) + gamma(6) * np.abs(dis)
    else:
        r = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
        dis = r - o.min()
        bound = gamma(3) * r + gamma(2) * np.abs(dis)
    return {"pts": pts, "dis": dis}, {"pts": np.zeros_like(pts), "dis": bound.astype(np.float64)}


def shape_loss(y, dis, g=1.0, dtype=np.float64):
    """y (N,), dis (N,) -> ({loss, dy (N,)}, bounds) for the incoming gradient g."""
    y, dis = np.asarray(y).reshape(-1).astype(dtype), np.asarray(dis).reshape(-1).astype(dtype)
    N = y.shape[0]
    r = -y - dis
    loss = (r * r).mean(dtype=dtype)
    dy = -((dtype(g) / dtype(N)) * (dtype(2) * r))
    return {"loss": loss, "dy": dy}, {"loss": gamma(N + 4) * float(loss), "dy": gamma(4) * np.abs(dy).astype(np.float64)}


# ---- rotation angle -------------------------------------------------------------------------------------------------------------
def _angle(X, Y, dtype):
    """X, Y (P,3,3) -> (cos, angle, dangle / dcos, e_angle, e_dangle) of rot_angle(X Y^T)."""
    X, Y = X.astype(dtype), Y.astype(dtype)
    prod = X * Y
    tr = prod.sum((1, 2))
    S = np.abs(prod).sum((1, 2)).astype(np.float64)
    c = (tr - dtype(1)) / dtype(2)
    lo, hi = dtype(-1 + EPS), dtype(1 - EPS)
    cc = np.clip(c, lo, hi)
    angle = np.arccos(cc)
    inside = (c >= lo) & (c <= hi)
    with np.errstate(divide="ignore", invalid="ignore"):
        dang = np.where(inside, -1 / np.sqrt(1 - cc * cc), 0).astype(dtype)
    c64 = c.astype(np.float64)
    e_cos = (gamma(10) * S + U32 * np.abs(tr.astype(np.float64) - 1)) / 2 + U32
    far = np.minimum(np.abs(c64) + e_cos, 1 - EPS)                     # the end of the interval where acos is steepest
    D = 1 / np.sqrt(1 - far * far)
    e_angle = D * e_cos + 4 * U32 * angle.astype(np.float64)
    straddles = (np.abs(np.abs(c64) - (1 - EPS)) <= e_cos)
    e_dang = np.where(straddles, D, np.where(inside, e_cos * far / (1 - far * far) ** 1.5 + gamma(5) * np.abs(dang.astype(np.float64)), 0))
    return c, angle, dang, e_angle, e_dang


def _split(rtk, dtype):
    rtk = np.asarray(rtk, np.float32)
    return rtk[:, :3, :3].astype(dtype), rtk[:, :3, 3].astype(dtype)


def rtk_loss(rtk, rtk_raw, g=(1.0, 0.0, 0.0), dtype=np.float64):
    """rtk, rtk_raw (T, 3|4, 4) fp32 -> ({total, rot_loss, trn_loss, drtk (the shape of rtk)}, bounds); g = the gradients of
    (total, rot_loss, trn_loss)."""
    Rp, tp = _split(rtk, dtype)
    Rg, tg = _split(rtk_raw, dtype)
    T = Rp.shape[0]
    _, angle, dang, e_angle, e_dang = _angle(Rp, Rg, dtype)
    rot = dtype(0.01) * angle.mean(dtype=dtype)
    d = tp - tg
    trn = (d * d).sum(-1).mean(dtype=dtype)
    total = rot + trn
    gr, gn = dtype(g[0] + g[1]), dtype(g[0] + g[2])
    k = gr * dtype(0.01) / dtype(T) * dtype(0.5)
    gc = k * dang
    drtk = np.zeros(np.asarray(rtk).shape, dtype)
    drtk[:, :3, :3] = gc[:, None, None] * Rg
    drtk[:, :3, 3] = gn / dtype(T) * dtype(2) * d
    b_rot = 0.01 * e_angle.mean() + gamma(T + 3) * abs(float(rot))
    b_trn = gamma(T + 6) * float(trn)
    b_d = np.zeros(drtk.shape)
    b_d[:, :3, :3] = np.abs(Rg).astype(np.float64) * (abs(float(k)) * e_dang + gamma(6) * np.abs(gc.astype(np.float64)))[:, None, None]
    b_d[:, :3, 3] = gamma(5) * np.abs(drtk[:, :3, 3].astype(np.float64))
    return ({"total": total, "rot_loss": rot, "trn_loss": trn, "drtk": drtk},
            {"total": b_rot + b_trn + U32 * abs(float(total)), "rot_loss": b_rot, "trn_loss": b_trn, "drtk": b_d})


def pair_starts(data_offset, T):
    """The first frames of the pooled pairs: (i, i + 1) inside one video."""
    out = []
    for v in range(len(data_offset) - 1):
        s, e = max(int(data_offset[v]), 0), min(int(data_offset[v + 1]), T)
        out += list(range(s, e - 1))
    return np.asarray(out, np.int64)


def root_sm_loss(rtk_all, data_offset, g=1.0, dtype=np.float64):
    """compute_root_sm_loss: rtk_all (T, 3|4, 4) fp32 -> ({loss, rot, trn, pairs, drtk}, bounds).  No pooled pair: NaN, zero
    gradient."""
    R, t = _split(rtk_all, dtype)
    T = R.shape[0]
    drtk = np.zeros(np.asarray(rtk_all).shape, dtype)
    b_d = np.zeros(drtk.shape)
    j = pair_starts(data_offset, T)
    P = len(j)
    if P == 0:
        nan = dtype(np.nan)
        return ({"loss": nan, "rot": nan, "trn": nan, "pairs": 0, "drtk": drtk}, {"loss": 0.0, "rot": 0.0, "trn": 0.0, "drtk": b_d})
    _, angle, dang, e_angle, e_dang = _angle(R[j], R[j + 1], dtype)
    d = t[j] - t[j + 1]
    nrm = np.sqrt((d * d).sum(-1))
    rot = angle.mean(dtype=dtype) * dtype(1e-3)
    trn = nrm.mean(dtype=dtype) * dtype(0.1)
    loss = rot + trn
    k = dtype(g) * dtype(1e-3) / dtype(P) * dtype(0.5)
    gc = k * dang
    with np.errstate(divide="ignore", invalid="ignore"):
        gt = np.where(nrm > 0, dtype(g) * dtype(0.1) / dtype(P) / nrm, 0).astype(dtype)
    e_gc = abs(float(k)) * e_dang + gamma(6) * np.abs(gc.astype(np.float64))
    term = gt[:, None] * d
    for a, (me, other, sgn) in enumerate(((j, j + 1, 1), (j + 1, j, -1))):
        np.add.at(drtk[:, :3, :3], me, gc[:, None, None] * R[other])
        np.add.at(drtk[:, :3, 3], me, sgn * term)
        np.add.at(b_d[:, :3, :3], me, np.abs(R[other]).astype(np.float64) * e_gc[:, None, None])
        np.add.at(b_d[:, :3, 3], me, gamma(12) * np.abs(term.astype(np.float64)))
    b_d[:, :3, :3] += gamma(2) * np.abs(drtk[:, :3, :3].astype(np.float64))
    b_rot = 1e-3 * e_angle.mean() + gamma(P + 4) * abs(float(rot))
    b_trn = 0.1 * gamma(4) * float(nrm.mean()) + gamma(P + 4) * abs(float(trn))
    return ({"loss": loss, "rot": rot, "trn": trn, "pairs": P, "drtk": drtk},
            {"loss": b_rot + b_trn + U32 * abs(float(loss)), "rot": b_rot, "trn": b_trn, "drtk": b_d})


# ---- quaternions ----------------------------------------------------------------------------------------------------------------
def matrix_to_quaternion(R, dtype=np.float64):
    """R (T,3,3) -> unit quaternions (T,4), real part first and >= 0, by the rule of include/moda_hip.h (moda_matrix_to_quat)."""
    R = np.asarray(R, np.float32).astype(dtype)
    one = dtype(1)
    r = lambda a, b: R[:, a, b]
    d = np.stack([((one + r(0, 0)) + r(1, 1)) + r(2, 2), ((one + r(0, 0)) - r(1, 1)) - r(2, 2),
                  ((one - r(0, 0)) + r(1, 1)) - r(2, 2), ((one - r(0, 0)) - r(1, 1)) + r(2, 2)], -1)
    best = d.argmax(-1)                                                # the first of equal maxima
    cand = np.stack([
        np.stack([d[:, 0], r(2, 1) - r(1, 2), r(0, 2) - r(2, 0), r(1, 0) - r(0, 1)], -1),
        np.stack([r(2, 1) - r(1, 2), d[:, 1], r(0, 1) + r(1, 0), r(0, 2) + r(2, 0)], -1),
        np.stack([r(0, 2) - r(2, 0), r(0, 1) + r(1, 0), d[:, 2], r(1, 2) + r(2, 1)], -1),
        np.stack([r(1, 0) - r(0, 1), r(0, 2) + r(2, 0), r(1, 2) + r(2, 1), d[:, 3]], -1)], 1)
    q = cand[np.arange(len(R)), best]
    n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    s = np.where(q[:, 0] < 0, -one, one) / n
    return q * s[:, None]


def random_rotations(rng, n):
    """n rotations drawn as unit quaternions, formed in float64 and rounded to fp32: |R - rotation| <= u per entry."""
    q = rng.standard_normal((n, 4))
    return quaternion_to_matrix(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def quaternion_to_matrix(q):
    """Unit (or any non-zero) quaternions (T,4), real first -> (T,3,3) float64: the standard matrix scaled by 2 / |q|^2."""
    q = np.asarray(q, np.float64)
    r, i, j, k = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    s = 2.0 / (q * q).sum(-1)
    return np.stack([1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r),
                     s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r),
                     s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)], -1).reshape(-1, 3, 3)


def half_turns():
    """Rotations by 180 degrees about x, y, z (trace -1: the real part is 0, one per dominant axis) and about a skew axis."""
    out = [np.diag(v) for v in ((1., -1., -1.), (-1., 1., -1.), (-1., -1., 1.))]
    a = np.asarray([1., 2., 3.]) / np.sqrt(14.)
    out.append(2 * np.outer(a, a) - np.eye(3))
    return np.stack(out).astype(np.float32)
