"""Float64 closed-form reference of the articulation chain, forward and backward, exactly as the kernels define it:
bone_prep / bone_transform / dq_inverse (csrc/prep_kernels.hip), the skinning softmax + dual-quaternion blend (warp_body in
csrc/render_kernels.hip, warp_bwd_kernel and warp_bwd_reduce_kernel in csrc/train_kernels.hip).  Plain numpy; inputs are taken as
given (float32 arrays are widened, never re-rounded); nothing here imports the package.  u = U = 2^-24, the fp32 unit round-off.

Layouts     bones (.., 10) = [centre 3 | quaternion 4, real first | log scale 3];  prep (nsets, B, 16) = [c | R row-major | exp(scale)
            | 0], nsets = 1 (shared bones) or N (per ray);  q (N, B, 8) the dual quaternions blended as given;  pts, pts_tf, cyc_ref
            (N, S, 3);  dskin, skin (N, S, B);  skin_aux (2,), [0] the log scale of the gaussians.
The maths    e = c_b - x,  m_k = sum_j R[j][k] e_j,  logit_b = G sum_k s_k m_k^2 + dskin_b,  G = -1000 exp(skin_aux[0]),
            skin = softmax_b(logit),  bl = sum_b skin_b q_b,  c = bl / |bl[:4]| = (a0, d0, ae, de),  p = pts_tf or pts,
            out = p + 2 d0 x (d0 x p + a0 p) + 2 (a0 de - ae d0 + d0 x de),  cyc = |cyc_ref - out|.
            Backward: g = g_out - d_ref with d_ref = g_cyc (ref - out) / cyc and d_ref = 0 where cyc == 0;  dbl from g through the
            transform and the normalisation;  ds_b = g_skin_b + dbl . q_b,  sdot = sum_j skin_j ds_j,  dl_b = skin_b (ds_b - sdot)
            = d_dskin;  d_q[n, b] = sum_s skin_b dbl;  d_prep[n, b] = sum_s dl_b d logit_b / d prep_b (summed over n too when the
            bones are shared);  d_aux0 = sum_{n,s,b} dl_b G sum_k s_k m_k^2;  d_pts = (transform part, unless pts_tf takes it)
            - sum_b dl_b d logit_b / d e.

Error figure  |got - truth| / (u * condition) per element (ratio()).  A condition of exactly 0 means the element must be exactly
            0.  Where a condition is not 0, TINY = 2^-100 is added, so that u * condition never lies under the fp32 normal range
            (a weight of 1e-60 in float64 is 0 in fp32).
Conditions  of a gradient: the element's closed form with every term taken in absolute value.  d_q, d_prep, d_aux0: the sum of
            the absolute per-sample contributions (over s; over n, s and b for d_aux0; over n too for shared d_prep), the factor
            dl_b of a contribution to d_prep and d_aux0 read as d_dskin's condition (below).  d_dskin:
            |skin_b| (|ds_b| + sum_j |skin_j ds_j|), |ds_b| read term by term as |g_skin_b| + sum_k |dbl_k q_bk|: out does not
            change when bl is scaled, so dbl . bl = 0, and where one weight is 1 (bl = q_b) ds_b = dbl . q_b is ITSELF a sum
            that cancels to nothing -- with the plain |ds_b| two float64 evaluations differ by 1e-3 of the condition there.
            dbl, wherever it enters a condition (d_q's contributions skin_b dbl, ds_b), is its own absolute terms through the
            transform and the normalisation, like d_pts_tf: dbl cancels too.  Its dual real part is -2 (g . d0) / |bl[:4]|, three
            products; on the case B = 33, (N, S) = (3, 21), shared bones, cyc only, they are 0.0456, -0.0081, -0.0370 on the
            sample that gives 78 % of d_q[2, 1, 4] and add up to 0.00054.  With |dbl| as it stands the figure of that element is
            127 for a float64 backward of the saved fp32 weights (a backward kernel without any rounding), 239 for the same in
            fp32 numpy, 335 for the kernel, and 62 to 81 for float32 autograd depending on the CPU it runs on (55 to 137 on
            B = 49, (1, 257), per-ray, pts_tf): a bar of 4 x autograd's figure then tells nothing about the kernel.
            d_pts: sum_b |dl_b| |d logit_b / d x| (term by term) plus the transform part's absolute terms, |dl_b| read as
            d_dskin's condition for the same reason (the dominant bone's dl_b = -sum of the others' cancels in ds_b - sdot);
            d_pts_tf: the transform part's alone.  d_ref_j: |g_cyc| (R_j + |r_j| sum_i |r_i| R_i / cyc^2) / cyc with R = |ref| + the absolute terms of out: what r = ref - out cancels from.
            of a forward output: skin_b (1 + L_b + sum_j skin_j L_j), L_b = |G| sum_k s_k (sum_j |R_jk e_j|)^2 + |dskin_b| the
            logit's absolute terms (a logit of 1e3 carries an absolute error of 1e3 u, which the softmax turns into a relative
            one);  out_j: its absolute terms plus sum_b |d out_j / d skin_b| cond(skin_b);  cyc: |cond(ref - out)|_2 + cyc.
            The gradients' conditions do NOT hold what the saved fp32 weights are off by: that part is measured, not counted --
            the bar of tests/test_gpu_warp.py is max(FLOOR, 4 x the figure of float32 torch autograd on the same case), and
            float32 autograd carries the same logit error.

FLOOR       the relative roundings ONE term gathers in the kernel (fp contraction on: an fma rounds once), as formulas in B, S
            and N (floors()).  Counted, not tuned:
  skin      e 1, m three products and two sums 3, squared (doubles) 8 + 1, s, 100, e_aux (expf: 2) 4, three terms 2, -10 and
            + dskin 2: 20 on the logit; l - max and the exponent's scaling 2, the hardware exponential 2: 24; the B-term sum of
            the normaliser B, 1 / sum and the product 2                                                             26 + B
  out       skin's, the blend's B fmas, |bl[:4]| 4, division 1, the transform's depth of 10 products and sums      41 + 2B
  cyc       out's, the difference, the norm 4                                                                      46 + 2B
  dbl       the recomputed blend B + 5, g (2 g, cycle term) 3, cross products and sums of dc 8, the dot with bl 9, dn 3,
            dc / n + dn bl / n 4                                                                                    32 + B
  d_pts_tf  the same chain with dp in place of dbl, no normaliser: B + 5 + 3 + 8                                   16 + B
  d_dskin   dbl's, ds: g_skin + 8 fmas 9, sdot's B fmas, ds - sdot and the product 2                               43 + 2B
  d_pts     d_dskin's, d logit / d e: m 4, G 3, 2 s m 3, R dm 3, the B-term difference chain B; the transform part is under it
                                                                                                                   56 + 3B
  d_ref     out's, ref - out 1, the norm 4, g r / len 2                                                            48 + 2B
  d_q       dbl's, the product, ceil(S / 8) fmas of one slice, the 8-slice tree 8                         41 + B + ceil(S / 8)
  d_prep    d_dskin's, the contribution (as d_pts: 13), ceil(S / 8) sums, the tree 8; shared bones: N more (the column sum
            over the rays)                                                                   64 + 2B + ceil(S / 8) [+ N]
  d_aux0    d_dskin's, the contribution 13, ceil(S / 8) sums, the tree 8, N ceil(B / 32) 32 <= N (B + 31) atomic adds
                                                                                 64 + 2B + ceil(S / 8) + N (B + 31)
  prep kernels (PREP_FLOOR): bone_prep |q| 4, u 1, ts 5, a 2 + 8 sums 10, G 12, ts a - c q 4, dot 5, (du - u dot) / |q| 3: 44;
            the exp(scale) entries 3.  bone_transform: R 8, dR 1, quat_to_mat_bwd 31, two Hamilton products and their sums
            2 x 5 + 3: 53 for d_rts; d_bones R^T g 5, conj(r) gp 5: 5, per ray, N more for the column sum.  dq_inverse: n2 4,
            dot 9, n2^2 and the division 3, the two terms 4: 20.
"""
import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -100
PREP_FLOOR = {"bone_prep": 44.0, "bone_transform_rts": 53.0, "bone_transform_bones": 5.0, "dq_inverse": 20.0}


def floors(B, S, N=1, shared=False):
    """FLOOR per output of the warp, forward and backward (module docstring)."""
    s8 = -(-S // 8)
    return {"skin": 26.0 + B, "out": 41.0 + 2 * B, "cyc": 46.0 + 2 * B, "d_pts_tf": 16.0 + B, "d_dskin": 43.0 + 2 * B,
            "d_pts": 56.0 + 3 * B, "d_ref": 48.0 + 2 * B, "d_q": 41.0 + B + s8, "d_prep": 64.0 + 2 * B + s8 + (N if shared else 0),
            "d_aux0": 64.0 + 2 * B + s8 + N * (B + 31)}


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def _tiny(c):
    return c + TINY * (c > 0)


def ratio(got, ref, cond):
    """|got - ref| / (u cond) per element; 0 where both vanish, inf where only the condition does (an exact statement missed)
    or where `got` is not finite."""
    got = np.asarray(got, np.float64)
    diff = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(cond > 0, diff / (U * np.where(cond > 0, cond, 1.0)), np.where(diff == 0, 0.0, np.inf))
    return np.where(np.isfinite(got), r, np.inf)


# ----------------------------------------------------------------------------------------------------------------------- quaternions
_QS = np.array([[[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [0, 0, 0, -1]],      # o_i = sum_jk _QS[i, j, k] a_j b_k (Hamilton)
                [[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1], [0, 0, -1, 0]],
                [[0, 0, 1, 0], [0, 0, 0, -1], [1, 0, 0, 0], [0, 1, 0, 0]],
                [[0, 0, 0, 1], [0, 0, 1, 0], [0, -1, 0, 0], [1, 0, 0, 0]]], np.float64)
_CONJ = np.array([1.0, -1.0, -1.0, -1.0])


def qmul(a, b, ab=False):
    if ab:
        return np.einsum("ijk,...j,...k->...i", np.abs(_QS), np.abs(a), np.abs(b))
    return np.einsum("ijk,...j,...k->...i", _QS, a, b)


def _qv(q):
    """v (.., 9) with matrix(q) = I + ts v, ts = 2 / |q|^2, and the same with both products of an entry in absolute value."""
    r, i, j, k = (q[..., n] for n in range(4))
    t1 = np.stack([-j * j, i * j, i * k, i * j, -i * i, j * k, i * k, j * k, -i * i], -1)
    t2 = np.stack([-k * k, -k * r, j * r, k * r, -k * k, -i * r, -j * r, i * r, -j * j], -1)
    return t1 + t2, np.abs(t1) + np.abs(t2)


def quat_to_mat(q):
    ts = 2.0 / (q * q).sum(-1, keepdims=True)
    return np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]) + ts * _qv(q)[0]


def quat_to_mat_bwd(q, g, ab=False):
    """dL/dq of R = matrix(q) given g = dL/dR (.., 9): ts a - ts^2 (v . g) q."""
    r, i, j, k = (q[..., n] for n in range(4))
    z = np.zeros_like(r)
    M = np.stack([np.stack([z, -k, j, k, z, -i, -j, i, z], -1),
                  np.stack([z, j, k, j, -2 * i, -r, k, r, -2 * i], -1),
                  np.stack([-2 * j, i, r, i, z, k, -r, k, -2 * j], -1),
                  np.stack([-2 * k, -r, i, r, -2 * k, j, i, j, z], -1)], -2)
    ts = 2.0 / (q * q).sum(-1, keepdims=True)
    v, va = _qv(q)
    if ab:
        return ts * np.einsum("...ik,...k->...i", np.abs(M), np.abs(g)) + ts * ts * (va * np.abs(g)).sum(-1, keepdims=True) * np.abs(q)
    return ts * np.einsum("...ik,...k->...i", M, g) - ts * ts * (v * g).sum(-1, keepdims=True) * q


# ---------------------------------------------------------------------------------------------------------------------- prep kernels
def bone_prep(bones):
    b = _f64(bones)
    q = b[..., 3:7]
    nrm = np.maximum(np.sqrt((q * q).sum(-1, keepdims=True)), 1e-12)
    return np.concatenate([b[..., :3], quat_to_mat(q / nrm), np.exp(b[..., 7:10]), np.zeros_like(b[..., :1])], -1)


def bone_prep_bwd(bones, g):
    """-> (d_bones, condition), (.., 10) each."""
    b, g = _f64(bones), _f64(g)
    q = b[..., 3:7]
    nrm = np.maximum(np.sqrt((q * q).sum(-1, keepdims=True)), 1e-12)
    u = q / nrm
    out = []
    for ab in (False, True):
        du = quat_to_mat_bwd(u, g[..., 3:12], ab)
        if ab:
            dq = (du + np.abs(u) * (du * np.abs(u)).sum(-1, keepdims=True)) / nrm
        else:
            dq = (du - u * (du * u).sum(-1, keepdims=True)) / nrm
        A = np.abs if ab else (lambda v: v)
        out.append(np.concatenate([A(g[..., :3]), dq, A(g[..., 12:15]) * np.exp(b[..., 7:10])], -1))
    return out[0], _tiny(out[1])


def bone_transform(bones, rts):
    """bones (B, 10), rts (N, B, 8) -> (N, B, 10); the orientation's sign makes its real part >= 0."""
    b, rts = _f64(bones), _f64(rts)
    r, d = rts[..., :4], rts[..., 4:]
    R = quat_to_mat(r).reshape(r.shape[:-1] + (3, 3))
    t = 2.0 * qmul(d, r * _CONJ)[..., 1:]
    centre = np.einsum("nbjk,bk->nbj", R, b[:, :3]) + t
    p = qmul(r, np.broadcast_to(b[None, :, 3:7], r.shape))
    p = np.where(p[..., :1] < 0, -p, p)
    return np.concatenate([centre, p, np.broadcast_to(b[None, :, 7:10], r.shape[:-1] + (3,))], -1)


def orient_real(bones, rts):
    """The real part of r (x) q0 before the sign rule: what decides the sign."""
    b, rts = _f64(bones), _f64(rts)
    return qmul(rts[..., :4], np.broadcast_to(b[None, :, 3:7], rts[..., :4].shape))[..., 0]


def bone_transform_bwd(bones, rts, g, force_sg=None):
    """-> {d_rts: (value, condition) (N, B, 8), d_bones_ray: (N, B, 10), d_bones: (B, 10), summed over the rays}.
    force_sg: a fixed sign in place of the rule (the test's mutant)."""
    b, rts, g = _f64(bones), _f64(rts), _f64(g)
    r, d = rts[..., :4], rts[..., 4:]
    R = quat_to_mat(r).reshape(r.shape[:-1] + (3, 3))
    c = np.broadcast_to(b[None, :, :3], r.shape[:-1] + (3,))
    q0 = np.broadcast_to(b[None, :, 3:7], r.shape)
    gc = g[..., :3]
    sg = np.where(qmul(r, q0)[..., :1] < 0, -1.0, 1.0) if force_sg is None else force_sg
    res = []
    for ab in (False, True):
        A = np.abs if ab else (lambda v: v)
        dbc = np.einsum("nbjk,nbj->nbk", A(R), A(gc))
        dR = (gc[..., :, None] * c[..., None, :]).reshape(r.shape[:-1] + (9,))
        dr = quat_to_mat_bwd(r, dR, ab)
        du = np.concatenate([np.zeros_like(gc[..., :1]), 2.0 * gc], -1)
        dd = qmul(du, r, ab)
        drc = qmul(d * _CONJ, du, ab)
        dr = dr + (drc if ab else drc * _CONJ)
        gp = sg * g[..., 3:7]
        dr = dr + qmul(gp, q0 * _CONJ, ab)
        dq0 = qmul(r * _CONJ, gp, ab)
        res.append((np.concatenate([dr, dd], -1), np.concatenate([dbc, dq0, A(g[..., 7:10])], -1)))
    (v_r, v_b), (c_r, c_b) = res
    return {"d_rts": (v_r, _tiny(c_r)), "d_bones_ray": (v_b, _tiny(c_b)), "d_bones": (v_b.sum(0), _tiny(c_b.sum(0)))}


_DQ_SG = np.array([1.0, -1, -1, -1, 1, -1, -1, -1])


def dq_inverse(dq):
    q = _f64(dq)
    return q * _DQ_SG / (q[..., :4] ** 2).sum(-1, keepdims=True)


def dq_inverse_bwd(dq, g):
    q, g = _f64(dq), _f64(g)
    n2 = (q[..., :4] ** 2).sum(-1, keepdims=True)
    real = np.array([1.0, 1, 1, 1, 0, 0, 0, 0])
    dot = (g * _DQ_SG * q).sum(-1, keepdims=True)
    val = _DQ_SG * g / n2 - real * 2.0 * q * dot / (n2 * n2)
    cond = np.abs(g) / n2 + real * 2.0 * np.abs(q) * np.abs(g * q).sum(-1, keepdims=True) / (n2 * n2)
    return val, _tiny(cond)


# ------------------------------------------------------------------------------------------------------------------------------ warp
def _cross(a, b, ab=False):
    ax, ay, az = (a[..., n] for n in range(3))
    bx, by, bz = (b[..., n] for n in range(3))
    if ab:
        return np.stack([ay * bz + az * by, az * bx + ax * bz, ax * by + ay * bx], -1)
    return np.stack([ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx], -1)


def _skin_chain(prep, per_ray, pts, dskin, skin_aux):
    P = _f64(prep)
    x = _f64(pts)
    N, S, _ = x.shape
    B = P.shape[1]
    assert P.shape[0] == (N if per_ray else 1), P.shape
    P = np.broadcast_to(P, (N, B, 16))
    R = P[:, :, 3:12].reshape(N, B, 3, 3)                        # R[j][k] at 3 + 3 j + k
    sc = P[:, :, 12:15]
    G = -1000.0 * np.exp(float(_f64(skin_aux)[0]))
    e = P[:, None, :, :3] - x[:, :, None, :]                     # (N, S, B, 3)
    m = np.einsum("nbjk,nsbj->nsbk", R, e)
    gauss = G * (sc[:, None] * m * m).sum(-1)                    # (N, S, B)
    logit = gauss if dskin is None else gauss + _f64(dskin)
    mabs = np.einsum("nbjk,nsbj->nsbk", np.abs(R), np.abs(e))
    L = abs(G) * (sc[:, None] * mabs * mabs).sum(-1) + (0.0 if dskin is None else np.abs(_f64(dskin)))
    z = logit - logit.max(-1, keepdims=True)
    ez = np.exp(z)
    skin = ez / ez.sum(-1, keepdims=True)
    return dict(N=N, S=S, B=B, R=R, sc=sc, G=G, e=e, m=m, gauss=gauss, skin=skin, L=L)


def _transform(c, p, ab=False):
    """out = p + 2 d0 x (d0 x p + a0 p) + 2 (a0 de - ae d0 + d0 x de); ab: the sum of the terms' magnitudes."""
    if ab:
        c, p = np.abs(c), np.abs(p)
    a0, d0, ae, de = c[..., 0:1], c[..., 1:4], c[..., 4:5], c[..., 5:8]
    u = _cross(d0, p, ab) + a0 * p
    t = a0 * de + (ae * d0 if ab else -ae * d0) + _cross(d0, de, ab)
    return p + 2.0 * _cross(d0, u, ab) + 2.0 * t


def _transform_bwd(bl, p, g, ab=False):
    """g = dL/d out -> (dp, dbl) through out = transform(bl / |bl[:4]|, p), as warp_bwd_kernel orders it; ab: every term in
    absolute value."""
    nrm = np.sqrt((bl[..., :4] ** 2).sum(-1, keepdims=True))
    c = bl / nrm
    if ab:
        c, p, g, bl = np.abs(c), np.abs(p), np.abs(g), np.abs(bl)
    sgn = 1.0 if ab else -1.0
    a0, d0, ae, de = c[..., 0:1], c[..., 1:4], c[..., 4:5], c[..., 5:8]
    dot = lambda a, b: (a * b).sum(-1, keepdims=True)
    u = _cross(d0, p, ab) + a0 * p
    g2 = 2.0 * g
    gu = _cross(g2, d0, ab)
    dd0 = _cross(u, g2, ab)
    dp = g + _cross(gu, d0, ab) + a0 * gu
    dd0 = dd0 + _cross(p, gu, ab)
    da0 = dot(gu, p) + dot(g2, de)
    dde = a0 * g2 + _cross(g2, d0, ab)
    dae = sgn * dot(g2, d0)
    dd0 = dd0 + sgn * ae * g2 + _cross(de, g2, ab)
    dc = np.concatenate([da0, dd0, dae, dde], -1)
    dn = sgn * dot(dc, bl) / (nrm * nrm)
    real = np.array([1.0, 1, 1, 1, 0, 0, 0, 0])
    return dp, dc / nrm + real * dn * bl / nrm


def warp(prep, per_ray, q, pts, pts_tf, dskin, skin_aux, cyc_ref):
    """-> {out, cyc (None without cyc_ref), skin: (float64 value, condition)}."""
    ch = _skin_chain(prep, per_ray, pts, dskin, skin_aux)
    q, skin = _f64(q), ch["skin"]
    p = _f64(pts) if pts_tf is None else _f64(pts_tf)
    c_skin = skin * (1.0 + ch["L"] + (skin * ch["L"]).sum(-1, keepdims=True))
    bl = np.einsum("nsb,nbk->nsk", skin, q)
    c = bl / np.sqrt((bl[..., :4] ** 2).sum(-1, keepdims=True))
    out = _transform(c, p)
    c_out = _transform(c, p, True)
    for j in range(3):
        _, dbl = _transform_bwd(bl, p, np.broadcast_to(np.eye(3)[j], p.shape))
        c_out[..., j] += (np.abs(np.einsum("nsk,nbk->nsb", dbl, q)) * c_skin).sum(-1)
    res = {"out": (out, _tiny(c_out)), "skin": (skin, _tiny(c_skin)), "cyc": None, "bl": bl}
    if cyc_ref is not None:
        r = _f64(cyc_ref) - out
        ln = np.sqrt((r * r).sum(-1))
        c_r = c_out + np.abs(_f64(cyc_ref))
        res["cyc"] = (ln, _tiny(np.sqrt((c_r * c_r).sum(-1)) + ln))
    return res


def warp_bwd(prep, per_ray, q, pts, pts_tf, dskin, skin_aux, cyc_ref, g_out, g_cyc, g_skin, sdot_without_g_skin=False):
    """-> {d_pts, d_pts_tf, d_dskin, d_q, d_prep, d_aux0, d_ref: (value, condition), None where the input is absent}, and
    'aux_terms' (N, S, B), 'dl' (N, S, B): the per-sample contributions to d_aux0 and the logit gradients.
    d_prep is (N, B, 16) per ray and (1, B, 16) for shared bones; d_aux0 has shape (1,).  d_dskin is reported whether dskin is
    given or not (it is the logits' gradient).  sdot_without_g_skin: the test's mutant."""
    ch = _skin_chain(prep, per_ray, pts, dskin, skin_aux)
    N, S, B, R, sc, G, e, m, skin = (ch[k] for k in ("N", "S", "B", "R", "sc", "G", "e", "m", "skin"))
    q = _f64(q)
    x = _f64(pts)
    p = x if pts_tf is None else _f64(pts_tf)
    bl = np.einsum("nsb,nbk->nsk", skin, q)
    nrm = np.sqrt((bl[..., :4] ** 2).sum(-1, keepdims=True))
    g = np.zeros((N, S, 3)) if g_out is None else _f64(g_out).copy()
    g_abs = np.abs(g)
    res = {"d_ref": None, "d_pts_tf": None}
    if cyc_ref is not None and g_cyc is not None:
        out = _transform(bl / nrm, p)
        out_abs = _transform(bl / nrm, p, True)
        ref = _f64(cyc_ref)
        r = ref - out
        ln = np.sqrt((r * r).sum(-1, keepdims=True))
        nz = ln > 0
        lns = np.where(nz, ln, 1.0)
        gc = _f64(g_cyc)[..., None]
        s = np.where(nz, gc * r / lns, 0.0)
        Rr = np.abs(ref) + out_abs
        c_s = np.where(nz, np.abs(gc) * (Rr + np.abs(r) * (np.abs(r) * Rr).sum(-1, keepdims=True) / (lns * lns)) / lns, 0.0)
        res["d_ref"] = (s, _tiny(c_s))
        g = g - s
        g_abs = g_abs + np.abs(s)
    dp, dbl = _transform_bwd(bl, p, g)
    dp_abs, dbl_abs = _transform_bwd(bl, p, g_abs, True)
    gs = np.zeros((N, S, B)) if g_skin is None else _f64(g_skin)
    ds = gs + np.einsum("nsk,nbk->nsb", dbl, q)
    sdot = (skin * (ds - gs if sdot_without_g_skin else ds)).sum(-1, keepdims=True)
    dl = skin * (ds - sdot)
    ds_abs = np.abs(gs) + np.einsum("nsk,nbk->nsb", dbl_abs, np.abs(q))          # |ds_b|, term by term (module docstring)
    res["d_dskin"] = (dl, _tiny(np.abs(skin) * (ds_abs + (np.abs(skin) * ds_abs).sum(-1, keepdims=True))))
    tq = skin[..., None] * dbl[:, :, None, :]                                    # (N, S, B, 8)
    res["d_q"] = (tq.sum(1), _tiny((np.abs(skin)[..., None] * dbl_abs[:, :, None, :]).sum(1)))
    # logit_b = G sum_k s_k m_k^2 (+ dskin_b)
    dm = dl[..., None] * G * 2.0 * sc[:, None] * m                               # (N, S, B, 3)
    de = np.einsum("nbjk,nsbk->nsbj", R, dm)
    t_R = (e[..., :, None] * dm[..., None, :]).reshape(N, S, B, 9)
    t_s = dl[..., None] * G * m * m
    t_aux = dl * ch["gauss"]
    terms = np.concatenate([de, t_R, t_s, np.zeros((N, S, B, 1))], -1)          # (N, S, B, 16)
    c_dl = res["d_dskin"][1]                                                      # |dl_b| term by term (module docstring)
    c_dm = c_dl[..., None] * abs(G) * 2.0 * sc[:, None] * np.abs(m)
    c_terms = np.concatenate([np.einsum("nbjk,nsbk->nsbj", np.abs(R), c_dm), (np.abs(e)[..., :, None] * c_dm[..., None, :]).reshape(N, S, B, 9),
                              c_dl[..., None] * abs(G) * m * m, np.zeros((N, S, B, 1))], -1)
    d_prep, c_prep = terms.sum(1), c_terms.sum(1)
    if not per_ray:
        d_prep, c_prep = d_prep.sum(0, keepdims=True), c_prep.sum(0, keepdims=True)
    res["d_prep"] = (d_prep, _tiny(c_prep))
    res["d_aux0"] = (np.asarray([t_aux.sum()]), _tiny(np.asarray([(c_dl * np.abs(ch["gauss"])).sum()])))
    dlx, dlx_abs = -de.sum(2), np.einsum("nbjk,nsbk->nsbj", np.abs(R), c_dm).sum(2)
    if pts_tf is None:
        res["d_pts"] = (dp + dlx, _tiny(dp_abs + dlx_abs))
    else:
        res["d_pts"] = (dlx, _tiny(dlx_abs))
        res["d_pts_tf"] = (dp, _tiny(dp_abs))
    res["aux_terms"], res["dl"] = t_aux, dl
    return res


# ------------------------------------------------------------------------------------------------------- the restatement in torch
def torch_bone_prep(bones):
    """[c | matrix(q / |q|) | exp(scale) | 0] with oracle/torch_ref.quaternion_to_matrix, in the dtype of its argument."""
    from oracle import torch_ref as tr
    qn = bones[..., 3:7]
    qn = qn / qn.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return torch.cat([bones[..., :3], tr.quaternion_to_matrix(qn).reshape(bones.shape[:-1] + (9,)), bones[..., 7:10].exp(),
                      torch.zeros_like(bones[..., :1])], -1)


def torch_warp(prep, q, pts, pts_tf, dskin, skin_aux, cyc_ref):
    """The warp on PREPARED bone data in torch (float64: pinned to warp() / warp_bwd(); float32: the figure a plain fp32
    autograd reaches): oracle/torch_ref.skinning's operations from [c | R | s] on, then oracle/torch_ref.dqs."""
    from oracle import torch_ref as tr
    N, S, _ = pts.shape
    B = prep.shape[1]
    P = prep.expand(N, B, 16)
    Rt = P[:, :, 3:12].reshape(N, B, 3, 3).transpose(-1, -2)
    mdis = P[:, None, :, :3] - pts[:, :, None, :]
    mdis = (Rt[:, None] * mdis[..., None, :]).sum(-1)
    mdis = P[:, None, :, 12:15] * mdis ** 2
    mdis = mdis * 100 * skin_aux[0].exp()
    logits = -10 * mdis.sum(-1)
    if dskin is not None:
        logits = logits + dskin
    skin = logits.softmax(-1)
    out = tr.dqs(q, skin, pts if pts_tf is None else pts_tf)
    cyc = None if cyc_ref is None else (cyc_ref - out).norm(dim=-1)
    return out, cyc, skin


WARP_LEAVES = ("prep", "q", "pts", "pts_tf", "dskin", "skin_aux", "cyc_ref")


def torch_warp_grads(a, g, dtype):
    """a: dict of numpy inputs (WARP_LEAVES; None = absent), g: dict out / cyc / skin -> numpy upstream gradient or None.
    -> (forward {out, cyc, skin}, gradients {d_prep, d_q, d_pts, d_pts_tf, d_dskin, d_aux0, d_ref}), float64 numpy arrays
    computed in `dtype`; a gradient nothing reaches is None."""
    t = {k: (None if a.get(k) is None else torch.from_numpy(np.array(a[k])).to(dtype).requires_grad_(True)) for k in WARP_LEAVES}
    out, cyc, skin = torch_warp(*(t[k] for k in WARP_LEAVES))
    fw = {"out": out, "cyc": cyc, "skin": skin}
    loss = None
    for k, v in fw.items():
        if v is not None and g.get(k) is not None:
            term = (v * torch.from_numpy(np.array(g[k])).to(dtype)).sum()
            loss = term if loss is None else loss + term
    loss.backward()
    gr = lambda k: None if t[k] is None or t[k].grad is None else t[k].grad.double().numpy()
    grads = {"d_prep": gr("prep"), "d_q": gr("q"), "d_pts": gr("pts"), "d_pts_tf": gr("pts_tf"), "d_dskin": gr("dskin"),
             "d_aux0": None if gr("skin_aux") is None else gr("skin_aux")[:1], "d_ref": gr("cyc_ref")}
    return {k: (None if v is None else v.detach().double().numpy()) for k, v in fw.items()}, grads
