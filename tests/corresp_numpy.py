"""Float64 reference, fp32 kernel models and per-element conditions of the correspondence heads and per-ray sums of the training
route (csrc/train_kernels.hip project_fwd / project_bwd / flow_render / pts_exp / points_bwd / segsum kernels, csrc/render_kernels.hip
sample_rays4_kernel<false> / points_kernel, csrc/loss_kernels.hip logsig_loss_kernel), restating the reference's
  project   obj_to_cam + pinhole_cam with K = mat2K(Kmatinv(Kinv))   geom_utils.py:567-581, 612-673, rendering.py:439-449
  flow      vrender_flo                                              geom_utils.py:1704-1743
  pts_exp   compute_pts_exp                                          loss_utils.py:165-175
  points    o + d z                                                  rendering.py:88-89
  rows      the row repeat of update_rays                            moda.py:1281-1311
  vis       the two -logsigmoid terms of visibility_loss             loss_utils.py:139-146
Inputs are taken as given (float32 arrays are widened, never re-rounded); nothing here imports the package.  u = U = 2^-24.
The reference's constants 1e-6, 1e-5 and 1e-9 meet fp32 tensors there and are rounded to fp32 by torch before they are used (the
kernels write 1e-6f, 1e-5f, 1e-9f), so the float64 evaluation takes the fp32 constants widened (C6, C5, C9): with the double 1e-5
the sample at Z = 1e-5f would be invalid in float64 and valid in fp32 and in the reference.

Per operation `op` there are four functions:
  op(..., f=np.float64)     forward in dtype f (float64: the truth; float32: the plain numpy fp32 figure the bars are scaled by)
  op_grads(...)             closed-form float64 gradients of sum(g * out)                       (pinned to autograd by the CPU test)
  op_model(..., mutate=)    fp32 numpy model in the KERNEL's arithmetic order: every lane's partial sum over its trips
                            s = lane, lane + 64, ... in order, then the 64-lane butterfly v[l] += v[l ^ o], o = 32 ... 1
                            (lane_sum); segsum's four row phases and their in-order sum (seg_sum); logsig's wave sums, the four
                            waves' sum, the scale and the blocks added in launch order.  mutate: one of MUTATIONS.
  op_condition(...)         per element the closed form with every term in absolute value, divisors included: a sum's magnitude
                            is the sum of its terms' magnitudes, a product's the product, and a quotient a / b has magnitude
                            mag(a) mag(b) / b^2 -- what a relative error of b does to a / b, mag(b) being the sum of |terms| b
                            was formed from (Z = R3 . x + T3 cancels; 1e-9 + sum w does not, the weights being >= 0).  k relative
                            roundings spread over such an expression move it by at most k u condition, to first order.  A
                            condition of 0 is an exact statement (an invalid sample's gradient, d_proj[..., 2], the untouched
                            columns of d_rtk).

FLOOR[output] = k, the relative roundings ONE term gathers on its way through the kernel (no contraction assumed: a fused
multiply-add only removes one).  S <= 256: a lane makes at most 4 trips, 3 additions (the first lands on 0), and the butterfly 6:
a per-ray sum costs a term 9.
  project   X, Y, Z: product 1 + three sums = 4.  den = 1e-6 + Z: 5.  fx = 1 / k0, px = -k2 / k0: 1.
            nu = fx X + px Z: 1 + 4 + 1, the sum = 7.   u = nu / den: 7 + 5 + 1 = 13; Z: 4                              proj 13
            dnu = gu / den: 5 + 1 = 6.  dX = dnu fx: 8.  (gu nu + gv nv): 7 + 1 + 1 = 9; den den: 11; the quotient 21; dZ's three
            sums: 24.   d_xyz = R0 dX + R3 dY + R6 dZ: 24 + 1 + 2                                                       d_xyz 27
            aR += dZ x: 25, the ray sum 9: 34.  aT: 33.  afx += dnu X: 6 + 4 + 1 = 11, + 9 = 20; / (k0 k0): 22; apx k2 /
            (k0 k0): 23; their sum 24                                                                                  d_rtk 34
  flow      sw: 9.  sx: (u - ox) 1, times w 1, + 9 = 11.  den = 1e-9 + sw: 10.  sc = 2 / img: 1.  sx / den sc: 11 + 10 + 1 + 1 + 1   flo 24
            gx = g sc: 2.  common: gx sx 14, the sum 15, den den 21, quotient 37.  gx (u - ox) + gy (v - oy): 5, / den: 16;
            + common: 38                                                                                                 d_w 38
            w gx / den: 3 + 10 + 1                                                                                    d_proj 14
  pts_exp   a: 1 + 9 = 10; den 10; a / den                                                                           pts_exp 21
            common: g a 11, two sums 13, den den 21, quotient 35; g . p / den: 3 + 10 + 1 = 14; + common: 36           d_w_pts 36
            (w / den) g: 10 + 1 + 1                                                                                     d_pts 12
  points    o + d z: 2                                                                                                    xyz 2
            d . g: 1 + 2 = 3 (the atomic add lands on 0: exact).  sum g: 9.  sum z g: 10                    d_z 3, d_o 9, d_d 10
  rows      forward: a copy, exact (rows 0).  backward: a row phase adds ceil(k / 4) - 1 times, the four phases 3: k <= 16   dx_rows 6
  vis       expf 2 (1 ulp); log1pf 2 and its argument's 2 (d log1p(e) / d e times e / log1p(e) <= 1): 4; the difference 5;
            times w 6; wave sum 6; the four waves 3; the scale (fl(0.1 / n): 1) and its product 2: 17; one atomic add per
            workgroup onto the running sum, 15 workgroups at most in the cases: 32                                     vis_loss 32
            sg = 1 / (1 + expf(z)): 2 + 1 + 1 = 4; g scale: 2; times sg: 7; times w: 8                                   dx_vis 8
Left out on purpose: nothing.  The counts are worst cases of a linear bound, so the kernels sit far below them (module docstring of
tests/test_gpu_corresp.py); a seeded mistake moves an element by a fraction of its own magnitude, 1 / u = 1.7e7 of these units."""
import numpy as np
import torch

U = 2.0 ** -24
C6, C5, C9 = (float(np.float32(v)) for v in (1e-6, 1e-5, 1e-9))
BUTTERFLY = (32, 16, 8, 4, 2, 1)
MUTATIONS = ("one_trip", "flow_common", "pts_common", "den_sq", "ninv_wave")
FLOOR = {"proj": 13.0, "d_xyz": 27.0, "d_rtk": 34.0, "flo": 24.0, "d_w": 38.0, "d_proj": 14.0, "pts_exp": 21.0, "d_w_pts": 36.0,
         "d_pts": 12.0, "xyz": 2.0, "d_z": 3.0, "d_o": 9.0, "d_d": 10.0, "rows": 0.0, "dx_rows": 6.0, "vis_loss": 32.0, "dx_vis": 8.0}


def ratio(got, ref, cond):
    """|got - ref| / (u cond) per element; 0 where both vanish, inf where only the condition does (an exact statement missed)
    or where `got` is not finite."""
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        diff = np.abs(got - ref)
    diff = np.where(np.isfinite(got), diff, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(cond > 0, diff / np.where(cond > 0, U * cond, 1.0), np.where(diff == 0, 0.0, np.inf))


# --------------------------------------------------------------------------------------------------------------------- reductions
def plain_sum(q, mutate=None):
    return q.sum(1)


def lane_sum(q, mutate=None):
    """q (N, S, ...) -> (N, ...): one wave per ray.  mutate 'one_trip': lanes stop after their first trip; 'no_wave': lane 0's
    partial sum is taken for the wave's."""
    N, S = q.shape[:2]
    trips = (S + 63) // 64
    q = np.concatenate([q, np.zeros((N, trips * 64 - S) + q.shape[2:], q.dtype)], 1).reshape((N, trips, 64) + q.shape[2:])
    acc = q[:, 0].copy()
    for t in range(1, trips):
        if mutate == "one_trip":
            break
        acc = acc + q[:, t]
    if mutate == "no_wave":
        return acc[:, 0]
    lanes = np.arange(64)
    for o in BUTTERFLY:
        acc = acc + acc[:, lanes ^ o]
    assert acc.dtype == q.dtype
    return acc[:, 0]


def seg_sum(g, k):
    """segsum_kernel on g (F * k, C) -> (F, C): row phase `sub` adds rows sub, sub + 4, ... in order, then ((p0 + p1) + p2) + p3."""
    g = g.reshape(-1, k, g.shape[-1])
    ph = []
    for sub in range(4):
        acc = np.zeros((g.shape[0], g.shape[-1]), g.dtype)
        for q in range(sub, k, 4):
            acc = acc + g[:, q]
        ph.append(acc)
    return ((ph[0] + ph[1]) + ph[2]) + ph[3]


def _cols(a, f):
    return [np.asarray(a[..., k], f) for k in range(a.shape[-1])]


# ------------------------------------------------------------------------------------------------------------------------ project
def _cam(rtk, f):
    r = [np.asarray(rtk[:, k:k + 1], f) for k in range(21)]
    k0, k1, k2, k3 = r[12], r[16], r[14], r[17]                  # mat2K(Kinv)
    return r, (f(1) / k0, f(1) / k1, -k2 / k0, -k3 / k1), (k0, k1, k2, k3)      # K2inv


def _project(xyz, rtk, g, f, rsum, mutate=None):
    x, y, z = _cols(xyz, f)
    r, (fx, fy, px, py), (k0, k1, k2, k3) = _cam(rtk, f)
    X = r[0] * x + r[1] * y + r[2] * z + r[9]
    Y = r[3] * x + r[4] * y + r[5] * z + r[10]
    Z = r[6] * x + r[7] * y + r[8] * z + r[11]
    den = f(C6) + Z
    nu, nv = fx * X + px * Z, fy * Y + py * Z
    out = np.stack([nu / den, nv / den, Z], -1)
    if g is None:
        return {"proj": out}
    gu, gv, gz = _cols(g, f)
    dnu, dnv = gu / den, gv / den
    dX, dY = dnu * fx, dnv * fy
    dZ = gz + dnu * px + dnv * py - (gu * nu + gv * nv) / (den if mutate == "den_sq" else den * den)
    d_xyz = np.stack([r[0] * dX + r[3] * dY + r[6] * dZ, r[1] * dX + r[4] * dY + r[7] * dZ, r[2] * dX + r[5] * dY + r[8] * dZ], -1)
    s = rsum(np.stack([dX * x, dX * y, dX * z, dY * x, dY * y, dY * z, dZ * x, dZ * y, dZ * z, dX, dY, dZ,
                       dnu * X, dnu * Z, dnv * Y, dnv * Z], -1), mutate)
    afx, apx, afy, apy = (s[:, k] for k in (12, 13, 14, 15))
    k0, k1, k2, k3 = (v[:, 0] for v in (k0, k1, k2, k3))
    d_rtk = np.zeros((xyz.shape[0], 21), f)
    d_rtk[:, :12] = s[:, :12]
    d_rtk[:, 12] = -afx / (k0 * k0) + apx * k2 / (k0 * k0)
    d_rtk[:, 14] = -apx / k0
    d_rtk[:, 16] = -afy / (k1 * k1) + apy * k3 / (k1 * k1)
    d_rtk[:, 17] = -apy / k1
    res = {"proj": out, "d_xyz": d_xyz, "d_rtk": d_rtk}
    assert all(v.dtype == f for v in res.values())
    return res


def project(xyz, rtk, f=np.float64):
    return _project(xyz, rtk, None, f, plain_sum)


def project_grads(xyz, rtk, g):
    return _project(xyz, rtk, g, np.float64, plain_sum)


def project_model(xyz, rtk, g, mutate=None):
    return _project(xyz, rtk, g, np.float32, lane_sum, mutate)


def project_condition(xyz, rtk, g):
    f = np.float64
    x, y, z = (np.abs(c) for c in _cols(xyz, f))
    r, (fx, fy, px, py), (k0, k1, k2, k3) = _cam(rtk, f)
    xs, ys, zs = _cols(xyz, f)
    den = f(C6) + (r[6] * xs + r[7] * ys + r[8] * zs + r[11])
    r = [np.abs(v) for v in r]
    fx, fy, px, py = (np.abs(v) for v in (fx, fy, px, py))
    X = r[0] * x + r[1] * y + r[2] * z + r[9]
    Y = r[3] * x + r[4] * y + r[5] * z + r[10]
    Z = r[6] * x + r[7] * y + r[8] * z + r[11]
    denm = C6 + Z
    iden = denm / den ** 2                                       # the magnitude of 1 / den
    nu, nv = fx * X + px * Z, fy * Y + py * Z
    gu, gv, gz = (np.abs(c) for c in _cols(g, f))
    dnu, dnv = gu * iden, gv * iden
    dX, dY = dnu * fx, dnv * fy
    dZ = gz + dnu * px + dnv * py + (gu * nu + gv * nv) * denm ** 2 / den ** 4
    d_xyz = np.stack([r[0] * dX + r[3] * dY + r[6] * dZ, r[1] * dX + r[4] * dY + r[7] * dZ, r[2] * dX + r[5] * dY + r[8] * dZ], -1)
    s = np.stack([dX * x, dX * y, dX * z, dY * x, dY * y, dY * z, dZ * x, dZ * y, dZ * z, dX, dY, dZ,
                  dnu * X, dnu * Z, dnv * Y, dnv * Z], -1).sum(1)
    afx, apx, afy, apy = (s[:, k] for k in (12, 13, 14, 15))
    k0, k1, k2, k3 = (np.abs(v[:, 0]) for v in (k0, k1, k2, k3))
    d_rtk = np.zeros((xyz.shape[0], 21))
    d_rtk[:, :12] = s[:, :12]
    d_rtk[:, 12] = afx / (k0 * k0) + apx * k2 / (k0 * k0)
    d_rtk[:, 14] = apx / k0
    d_rtk[:, 16] = afy / (k1 * k1) + apy * k3 / (k1 * k1)
    d_rtk[:, 17] = apy / k1
    return {"proj": np.stack([nu * iden, nv * iden, Z], -1), "d_xyz": d_xyz, "d_rtk": d_rtk}


def torch_project(xyz, rtk):
    """obj_to_cam and pinhole_cam as the reference writes them (matmul with the transposed matrices), in the arguments' dtype."""
    N = xyz.shape[0]
    R, Tm, Ki = rtk[:, 0:9].reshape(N, 3, 3), rtk[:, 9:12].reshape(N, 1, 3), rtk[:, 12:21].reshape(N, 3, 3)
    K = torch.zeros(N, 3, 3, dtype=xyz.dtype)                    # K2mat(mat2K(K2inv(mat2K(Kinv))))
    K[:, 0, 0], K[:, 1, 1] = 1.0 / Ki[:, 0, 0], 1.0 / Ki[:, 1, 1]
    K[:, 0, 2], K[:, 1, 2] = -Ki[:, 0, 2] / Ki[:, 0, 0], -Ki[:, 1, 2] / Ki[:, 1, 1]
    K[:, 2, 2] = 1
    v = (xyz.matmul(R.permute(0, 2, 1)) + Tm).matmul(K.permute(0, 2, 1))
    vz = v[:, :, 2:3]
    return torch.cat([v[:, :, :2] / (C6 + vz), vz], -1)


# --------------------------------------------------------------------------------------------------------------------------- flow
def invalid_mask(proj, img, f=np.float64):
    u, v, Z = _cols(proj, f)
    with np.errstate(invalid="ignore", over="ignore"):
        return (Z < f(C5)) | (np.sqrt(u * u + v * v) > f(2) * f(img))


def _flow(w, proj, xys, img, g, f, rsum, mutate=None):
    u, v, Z = _cols(proj, f)
    w = np.asarray(w, f)
    ox, oy = np.asarray(xys[:, 0:1], f), np.asarray(xys[:, 1:2], f)
    inv = invalid_mask(proj, img, f)
    zero = f(0)
    with np.errstate(invalid="ignore", over="ignore"):
        ww = np.where(inv, zero, w)
        tx, ty = ww * (np.where(inv, zero, u) - ox), ww * (np.where(inv, zero, v) - oy)
    sw, sx, sy = rsum(ww, mutate), rsum(tx, mutate), rsum(ty, mutate)
    ninv = rsum(inv.astype(f), "no_wave" if mutate == "ninv_wave" else mutate)
    den = f(C9) + sw
    sc = f(2) / f(img)
    res = {"flo": np.stack([sx / den * sc, sy / den * sc], -1), "valid": (ninv == 0).astype(f)[:, None]}
    if g is None:
        return res
    gx, gy = np.asarray(g[:, 0], f) * sc, np.asarray(g[:, 1], f) * sc
    common = -(gx * sx + gy * sy) / (den * den)
    if mutate == "flow_common":
        common = np.zeros_like(common)
    gx, gy, den, common = gx[:, None], gy[:, None], den[:, None], common[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        res["d_w"] = np.where(inv, zero, (gx * (u - ox) + gy * (v - oy)) / den + common)
        res["d_proj"] = np.stack([np.where(inv, zero, ww * gx / den), np.where(inv, zero, ww * gy / den), np.zeros_like(ww)], -1)
    assert all(a.dtype == f for a in res.values())
    return res


def flow(w, proj, xys, img, f=np.float64):
    return _flow(w, proj, xys, img, None, f, plain_sum)


def flow_grads(w, proj, xys, img, g):
    return _flow(w, proj, xys, img, g, np.float64, plain_sum)


def flow_model(w, proj, xys, img, g, mutate=None):
    return _flow(w, proj, xys, img, g, np.float32, lane_sum, mutate)


def flow_condition(w, proj, xys, img, g):
    f = np.float64
    inv = invalid_mask(proj, img)
    u, v, _ = _cols(np.where(inv[..., None], 0.0, proj), f)                                # (poison sits at invalid samples only)
    ws = np.where(inv, 0.0, np.asarray(w, f))
    ww = np.abs(ws)
    ax, ay = np.abs(u - np.asarray(xys[:, 0:1], f)), np.abs(v - np.asarray(xys[:, 1:2], f))  # the difference of two INPUTS rounds once
    sx, sy = (ww * ax).sum(1), (ww * ay).sum(1)
    den, denm = C9 + ws.sum(1), C9 + ww.sum(1)
    iden = denm / den ** 2
    sc = 2.0 / img
    gx, gy = np.abs(np.asarray(g[:, 0], f)) * sc, np.abs(np.asarray(g[:, 1], f)) * sc
    common = (gx * sx + gy * sy) * denm ** 2 / den ** 4
    d_w = np.where(inv, 0.0, (gx[:, None] * ax + gy[:, None] * ay) * iden[:, None] + common[:, None])
    d_proj = np.stack([ww * (gx * iden)[:, None], ww * (gy * iden)[:, None], np.zeros_like(ww)], -1)
    return {"flo": np.stack([sx * iden * sc, sy * iden * sc], -1), "d_w": d_w, "d_proj": d_proj}


def torch_flow(w, proj, xys, img):
    """vrender_flo with the in-place masking written as torch.where -> flo (N, 2), valid (N, 1)."""
    xy, Z = proj[..., :2], proj[..., 2]
    inv = torch.logical_or(Z < C5, xy.detach().norm(2, -1).abs() > 2 * img)
    w = torch.where(inv, torch.zeros_like(w), w)
    xy = torch.where(inv[..., None], torch.zeros_like(xy), xy)
    w = w / (C9 + w.sum(-1)[..., None])
    flo = (w[..., None] * (xy - xys.view(w.shape[:-1] + (1, 2)))).sum(-2)
    return flo / img * 2, (inv.sum(-1) == 0).to(w.dtype)[..., None]


# ------------------------------------------------------------------------------------------------------------------------ pts_exp
def _pts_exp(w, pts, g, f, rsum, mutate=None):
    w = np.asarray(w, f)
    p = _cols(pts, f)
    sw = rsum(w, mutate)
    a = [rsum(w * c, mutate) for c in p]
    den = f(C9) + sw
    res = {"pts_exp": np.stack([c / den for c in a], -1)}
    if g is None:
        return res
    g0, g1, g2 = (np.asarray(g[:, k], f) for k in range(3))
    common = -(g0 * a[0] + g1 * a[1] + g2 * a[2]) / (den * den)
    if mutate == "pts_common":
        common = np.zeros_like(common)
    g0, g1, g2, den, common = (v[:, None] for v in (g0, g1, g2, den, common))
    res["d_w_pts"] = (g0 * p[0] + g1 * p[1] + g2 * p[2]) / den + common
    wn = w / den
    res["d_pts"] = np.stack([wn * g0, wn * g1, wn * g2], -1)
    assert all(v.dtype == f for v in res.values())
    return res


def pts_exp(w, pts, f=np.float64):
    return _pts_exp(w, pts, None, f, plain_sum)


def pts_exp_grads(w, pts, g):
    return _pts_exp(w, pts, g, np.float64, plain_sum)


def pts_exp_model(w, pts, g, mutate=None):
    return _pts_exp(w, pts, g, np.float32, lane_sum, mutate)


def pts_exp_condition(w, pts, g):
    f = np.float64
    ws = np.asarray(w, f)
    w, p = np.abs(ws), [np.abs(c) for c in _cols(pts, f)]
    a = [(w * c).sum(1) for c in p]
    den, denm = C9 + ws.sum(1), C9 + w.sum(1)
    iden = denm / den ** 2
    g0, g1, g2 = (np.abs(np.asarray(g[:, k], f)) for k in range(3))
    common = (g0 * a[0] + g1 * a[1] + g2 * a[2]) * denm ** 2 / den ** 4
    d_w = (g0[:, None] * p[0] + g1[:, None] * p[1] + g2[:, None] * p[2]) * iden[:, None] + common[:, None]
    wn = w * iden[:, None]
    return {"pts_exp": np.stack([c * iden for c in a], -1), "d_w_pts": d_w,
            "d_pts": np.stack([wn * g0[:, None], wn * g1[:, None], wn * g2[:, None]], -1)}


def torch_pts_exp(w, pts):
    prob = w.reshape(-1, w.shape[-1], 1)
    prob = prob / (C9 + prob.sum(1)[:, None])
    return (pts * prob).sum(1)


# ------------------------------------------------------------------------------------------------------------------------- points
def _points(o, d, z, g, f, rsum, mutate=None):
    o, d, z = np.asarray(o, f), np.asarray(d, f), np.asarray(z, f)
    res = {"xyz": o[:, None, :] + d[:, None, :] * z[..., None]}
    if g is None:
        return res
    gx, gy, gz = _cols(g, f)
    res["d_z"] = d[:, 0:1] * gx + d[:, 1:2] * gy + d[:, 2:3] * gz
    res["d_o"] = rsum(np.asarray(g, f), mutate)
    res["d_d"] = rsum(z[..., None] * np.asarray(g, f), mutate)
    assert all(v.dtype == f for v in res.values())
    return res


def points(o, d, z, f=np.float64):
    return _points(o, d, z, None, f, plain_sum)


def points_grads(o, d, z, g):
    return _points(o, d, z, g, np.float64, plain_sum)


def points_model(o, d, z, g, mutate=None):
    return _points(o, d, z, g, np.float32, lane_sum, mutate)


def points_condition(o, d, z, g):
    return _points(np.abs(o), np.abs(d), np.abs(z), np.abs(g), np.float64, plain_sum)


def torch_points(o, d, z):
    return o[:, None, :] + d[:, None, :] * z[..., None]


# --------------------------------------------------------------------------------------------------------------------------- rows
def rows(x, k, f=np.float64):
    return {"rows": np.repeat(np.asarray(x, f), k, 0)}


def rows_grads(x, k, g):
    return {"rows": rows(x, k)["rows"], "dx_rows": np.asarray(g, np.float64).reshape(x.shape[0], k, -1).sum(1)}


def rows_model(x, k, g, mutate=None):
    return {"rows": rows(x, k, np.float32)["rows"], "dx_rows": seg_sum(np.asarray(g, np.float32), k)}


def rows_condition(x, k, g):
    return {"rows": np.zeros((x.shape[0] * k, x.shape[1])), "dx_rows": np.abs(np.asarray(g, np.float64)).reshape(x.shape[0], k, -1).sum(1)}


def torch_rows(x, k):
    return x[:, None, :].repeat(1, k, 1).reshape(-1, x.shape[1])


# ---------------------------------------------------------------------------------------------------------------------------- vis
def _softplus_neg(z):
    """-logsigmoid(z) = -(min(z, 0) - log1p(exp(-|z|))), torch's formula."""
    return -(np.minimum(z, 0) - np.log1p(np.exp(-np.abs(z))))


def vis(x, w_pos, n_neg, f=np.float64):
    x, w_pos = np.asarray(x, f).reshape(-1), np.asarray(w_pos, f).reshape(-1)
    neg = _softplus_neg(-x[:n_neg]).sum() * f(0.1 / n_neg)
    pos = (_softplus_neg(x[n_neg:]) * w_pos).sum() * f(1.0 / n_neg)
    return {"vis_loss": np.asarray(pos + neg, f).reshape(1)}


def vis_grads(x, w_pos, n_neg, g):
    x, w_pos = np.asarray(x, np.float64).reshape(-1), np.asarray(w_pos, np.float64).reshape(-1)
    g = float(np.asarray(g).reshape(-1)[0])
    dneg = g * (0.1 / n_neg) / (1.0 + np.exp(-x[:n_neg]))        # sign -1: -sign sigmoid(-sign x) = sigmoid(x)
    dpos = -g * (1.0 / n_neg) / (1.0 + np.exp(x[n_neg:])) * w_pos
    return {"vis_loss": vis(x, w_pos, n_neg)["vis_loss"], "dx_vis": np.concatenate([dneg, dpos])}


def _logsig_model(x, w, sign, scale, out, g):
    f = np.float32
    z = f(sign) * x
    wi = np.ones_like(x) if w is None else w
    if g is None:
        t = -(np.minimum(z, f(0)) - np.log1p(np.exp(-np.abs(z)))) * wi
        n = t.shape[0]
        blocks = min((n + 255) // 256, 2048)
        assert blocks * 256 >= n                                 # one trip per thread in every case here
        t = np.concatenate([t, np.zeros(blocks * 256 - n, f)]).reshape(blocks * 4, 64)
        lanes = np.arange(64)
        for o in BUTTERFLY:
            t = t + t[:, lanes ^ o]
        wv = t[:, 0].reshape(blocks, 4)
        for b in range(blocks):
            out = out + f(scale) * (((wv[b, 0] + wv[b, 1]) + wv[b, 2]) + wv[b, 3])
        return out
    sg = f(1) / (f(1) + np.exp(z))
    return g * f(scale) * (-f(sign) * sg) * wi


def vis_model(x, w_pos, n_neg, g, mutate=None):
    f = np.float32
    x, w_pos = np.asarray(x, f).reshape(-1), np.asarray(w_pos, f).reshape(-1)
    out = _logsig_model(x[:n_neg], None, -1.0, 0.1 / n_neg, f(0), None)
    out = _logsig_model(x[n_neg:], w_pos, 1.0, 1.0 / n_neg, out, None)
    g = f(np.asarray(g).reshape(-1)[0])
    dx = np.concatenate([_logsig_model(x[:n_neg], None, -1.0, 0.1 / n_neg, None, g),
                         _logsig_model(x[n_neg:], w_pos, 1.0, 1.0 / n_neg, None, g)])
    assert out.dtype == f and dx.dtype == f
    return {"vis_loss": np.asarray(out).reshape(1), "dx_vis": dx}


def vis_condition(x, w_pos, n_neg, g):
    x, w_pos = np.asarray(x, np.float64).reshape(-1), np.abs(np.asarray(w_pos, np.float64).reshape(-1))
    mag = lambda z: np.abs(np.minimum(z, 0)) + np.log1p(np.exp(-np.abs(z)))
    loss = mag(-x[:n_neg]).sum() * (0.1 / n_neg) + (mag(x[n_neg:]) * w_pos).sum() / n_neg
    return {"vis_loss": np.asarray([loss]), "dx_vis": np.abs(vis_grads(x, w_pos, n_neg, g)["dx_vis"])}


def torch_vis(x, w_pos, n_neg):
    import torch.nn.functional as F
    x = x.reshape(-1)
    neg = -F.logsigmoid(-x[:n_neg]).sum() * 0.1 / n_neg
    pos = -(F.logsigmoid(x[n_neg:]) * w_pos.reshape(-1)).sum() / n_neg
    return (pos + neg).reshape(1)


# ---------------------------------------------------------------------------------------------------------------------- the table
# op -> (input names, differentiated inputs and the name of their gradient, outputs, forward, grads, model, condition, torch restatement)
OPS = {
    "project": (("xyz", "rtk"), {"xyz": "d_xyz", "rtk": "d_rtk"}, ("proj",), project, project_grads, project_model, project_condition,
                lambda a: torch_project(a["xyz"], a["rtk"])),
    "flow": (("w", "proj", "xys", "img"), {"w": "d_w", "proj": "d_proj"}, ("flo",), flow, flow_grads, flow_model, flow_condition,
             lambda a: torch_flow(a["w"], a["proj"], a["xys"], a["img"])[0]),
    "pts_exp": (("w", "pts"), {"w": "d_w_pts", "pts": "d_pts"}, ("pts_exp",), pts_exp, pts_exp_grads, pts_exp_model, pts_exp_condition,
                lambda a: torch_pts_exp(a["w"], a["pts"])),
    "points": (("o", "d", "z"), {"o": "d_o", "d": "d_d", "z": "d_z"}, ("xyz",), points, points_grads, points_model, points_condition,
               lambda a: torch_points(a["o"], a["d"], a["z"])),
    "rows": (("x", "k"), {"x": "dx_rows"}, ("rows",), rows, rows_grads, rows_model, rows_condition, lambda a: torch_rows(a["x"], a["k"])),
    "vis": (("x", "w_pos", "n_neg"), {"x": "dx_vis"}, ("vis_loss",), vis, vis_grads, vis_model, vis_condition,
            lambda a: torch_vis(a["x"], a["w_pos"], a["n_neg"])),
}


def torch_grads(op, case, dtype):
    """Autograd through the torch restatement of `op` in `dtype` on case = {input: array or scalar, 'g': array} ->
    {output: value, gradient name: gradient}, float64 numpy."""
    names, diff, outs, *_, fn = OPS[op]
    a = {k: (torch.from_numpy(np.array(case[k])).to(dtype) if isinstance(case[k], np.ndarray) else case[k]) for k in names}
    for k in diff:
        a[k].requires_grad_(True)
    out = fn(a)
    (out * torch.from_numpy(np.array(case["g"])).to(dtype).reshape(out.shape)).sum().backward()
    res = {outs[0]: out.detach().double().numpy()}
    for k, name in diff.items():
        res[name] = np.zeros(a[k].shape) if a[k].grad is None else a[k].grad.double().numpy()
    return res


def reference(op, case):
    """-> {name: (truth, condition, float32 figure, bar)} for the forward output and every gradient of one case: truth the
    float64 closed form, the float32 figure the worst |f32 - truth| / (u condition) of the plain float32 evaluation (forward:
    numpy fp32; gradients: torch fp32 autograd through the restatement), bar = max(FLOOR, 4 x that figure)."""
    names, diff, outs, fwd, grads, _, cond, _ = OPS[op]
    args = [case[k] for k in names]
    truth, c = grads(*args, case["g"]), cond(*args, case["g"])
    f32 = dict(torch_grads(op, case, torch.float32))
    f32.update({k: v for k, v in fwd(*args, f=np.float32).items() if k in outs})
    res = {}
    for k in outs + tuple(diff.values()):
        fig = ratio(f32[k], truth[k], c[k])
        of = float(np.where(np.isfinite(fig), fig, 0.0).max()) if fig.size else 0.0
        res[k] = (truth[k], c[k], of, max(FLOOR[k], 4.0 * of))
    return res
