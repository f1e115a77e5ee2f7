"""Float64 reference of the compositing entry point (moda_amd/rendering.py::composite, csrc/moda_dev.h composite_ray / comp_alpha,
csrc/train_kernels.hip composite_bwd_kernel), restating the reference's rendering.py:183-237 with every option: noise, clip mask,
vis_pred mask, rgb_filter_scale, F feature channels, cyc, n_live and term_tau.  Inputs are taken as given (float32 arrays are
widened, never re-rounded); nothing here imports the package.  u = U = 2^-24, the fp32 unit round-off.

forward()   every output in float64 together with a first-order running bound of what an fp32 evaluation of the same
            recurrence may differ by.  With alpha_i the opacity, t_i = 1 - alpha_i + 1e-10, T_i = prod_{k<i} t_k, w_i = alpha_i T_i
            and eps_i the absolute error of alpha_i:
              E_0 = 0,   E_{i+1} = E_i t_i + T_i (eps_i + 2 u t_i) + u T_{i+1},   E_w,i = E_i alpha_i + T_i eps_i + u w_i
            (2 u t_i: the two roundings of 1 - alpha + 1e-10, which the float64 value does not have; u T_{i+1}: the product.  A
            product of k factors carries k - 1 roundings in ANY association -- the sequential cumprod of the oracle as well as the
            kernel's 32-lane Hillis-Steele scan times its carried prefix -- so one u per step covers both.)
            A sum over the samples of w_i c_i is bounded by  sum_i |c_i| E_w,i + r u |w_i c_i| + u d_i |w_i c_i|,  r the roundings
            of the term itself (1; with rgb_filter 7 + 10 |sigma_raw|: sigmoid(-10 sigma) = 1 / (1 + expf(10 sigma)) is a product,
            an expf (2 u and the product's u magnified by |10 sigma|), a sum, a division and two more products) and d_i the
            number of partial sums the term passes through: S - max(i, 1) in the oracle's sequential sum, 5 + G - g_i in the
            kernel (a 5-level butterfly over the term's group of 32, then the groups' sums added in order; G groups, g_i the
            term's); the larger of the two is taken.
eps_i       counted from comp_alpha (fp contraction off, every operation rounds once = u relative):
              |d|      three products, two sums, a square root (which halves what it is given):          3 u          (C_DNORM)
              delta    z_{i+1} - z_i of two fp32 INPUTS rounds once (u |delta|; the cancellation term u (|z_i| + |z_{i+1}|)
                       would belong to depths that carry an error of their own: these are inputs, taken as given), times |d|:
                       1 + 3 + 1 =                                                                      5 u          (C_DELTA)
              ibeta    1 / (|beta| + 1e-9): a sum and a division:                                        2 u          (C_IBETA)
              x        -|sdf| ibeta, sdf = -(sigma_raw [+ noise]): (1 with noise) + 2 + 1 =             3 u or 4 u   (c_x)
              em       expm1f(x), 1 ulp = 2 u (C_EXP, the device library's documented accuracy; numpy's float32 routines are
                       within it too) and e^x c_x u |x| from its argument
              p        0.5 + 0.5 sgn em: the halving is exact, the sum rounds once.  ABSOLUTE error 0.5 E_em + u p, about
                       u |em|: for sdf > 0, p = 0.5 e^x is what is left after 0.5 - 0.5 |em| cancels, so the density p ibeta
                       carries an absolute error of order u / beta however small it is.  With |sdf| / beta beyond 17, expm1f
                       returns -1, p is exactly 0 in fp32 and 0.5 e^x in float64.
              dens     p ibeta: ibeta E_p + 3 u dens
              y        -delta dens: delta E_dens + 6 u |y|
              alpha    1 - expf(y): e^(y + E_y) - e^y (NOT linearised: the last sample has delta = 1e10, E_y is of order
                       1e10 u / beta there and the bound reaches 1: the last weight of a ray in empty space flips between 0
                       and T in fp32, in the oracle as in the kernel) + 2 u e^y + u alpha, at most 1 (alpha lies in [0, 1]).
            Masked samples have alpha = 0 exactly, eps = 0.  Where a bound is not 0, 2^-120 is added for results in the
            denormal range (transmittances behind a saturated sample fall by 1e-10 per step).
gradients() float64 gradients of sum(g * out) for rgbsigma, feat, z, rays_d, beta and cyc by torch autograd over torch_forward()
            (the same restatement written with torch, masks as torch.where; cyc_out is composed with DETACHED weights and
            vis_out is not differentiable, rendering.py:408, 473).
condition() per gradient element, the closed form of that element (analytic(), pinned to autograd by the CPU test) with every term
            replaced by its absolute value (|v_i| T_i + sum_{k>i} |v_k| w_k / t_i for d alpha, 0.5 + 0.5 |em| for p,
            |d delta_i| + |d delta_{i-1}| for d z, ...) and every weight, transmittance and divisor in it by what an fp32 evaluation
            may have it off by: E_w + u w, E_T + u T and (eps + 2 u t) / t of the forward recurrence above, and the factor
            1 - alpha = expf(y) of d alpha / d dens and d alpha / d delta by eps times the magnitude of the rest.  (u w alone would not
            do: alpha = 1 - expf(y) cancels for a thin sample, so a weight of 1e-5 T carries u T, not 1e-5 u T; and behind a
            surface every factor t of a transmittance is off by u in absolute terms.)  The result is at least u times the sum of
            the terms' magnitudes, so the kernel's  v T - suffix / t  is judged against what its cancellation and its inputs'
            own round-off allow; BWD_FLOOR counts the remaining relative roundings per term.
backward_reference()  truth, condition and bar of every gradient of one case: what the GPU test and the CPU models are held to."""
import numpy as np
import torch

U = 2.0 ** -24
C_EXP = 2.0
C_DNORM = 3.0
C_DELTA = 5.0
C_IBETA = 2.0
TINY = 2.0 ** -120
FWD_FLOOR = 1.0          # the counted constants are inside the bound: an fp32 evaluation with those roundings stays within it
SUMS = ("rgb", "feat", "depth", "sil", "vis_out", "cyc_out")
PER_SAMPLE = ("weights", "visibility")


# Backward floors, in units of the condition figure.  condition() already holds what the saved weights and transmittances, the divisor
# t and the factor expf(y) may be off by (1: they may sit AT their forward bound), and is at least u times the sum of the element's
# terms' magnitudes; the floor adds the relative roundings ONE term gathers on its way through composite_bwd_kernel.  They do not grow
# with S (a term passes through a six-step scan and at most three carried suffixes, not through S partial sums) nor with |x| or |y|:
#   v         up to 6 + F products (rgb 3, depth, sil, weights, F <= 16 features) added one at a time: 6 + F = 22; with rgb_filter
#             sem = scale / (1 + expf(10 sigma)) adds 8 (two products, expf 2 and its argument 10 |sigma| < 1 of the cases, sum,
#             division): 30
#   dalpha    v w 1, scan 6, p - v w 1, + suffix 1, the suffix carried over at most three blocks 3, / t 1, the difference 1: 44
#   ddens     delta 5 (C_DELTA), expf 2, two products: 53          ddelta  dens 10 (expf 2, e - 1 and 0.5 + 0.5 . against
#             0.5 + 0.5 |em| 2, its argument 4 |x| e^x / 0.5 <= 3, ibeta 2, product 1), expf 2, two products: 58
#   d sigma   ddens 0.5 ib ib e: ibeta 2 x 2, expf 2, three products: 62, and the bound's 1: 63
#   d z       ddelta |d|: |d| 3, product, the depth term's product, the difference, the neighbour's atomic add: 64 -> 65
#   d rays_d  ddelta zdiff 2, a lane's three blocks 3, butterfly 6, d / |d| 5: 74 -> 75
#   d beta    ddens ddib: ddib 8 and the product, three blocks 3, butterfly 6, sign ib ib 6, the atomics of nine rays 8: 85 -> 86
#   d rgb     w sem g: 10, under d sigma's in the same tensor          d feat, d cyc   w g: the product, 1 -> 2
# Left out on purpose: expf(x) in d sigma carries its argument's 4 |x| u, up to 120 u on the empty rays.  Neither the float32
# autograd nor the fp32 model of the kernel (tests/test_composite_oracle.py::backward_model) comes near the floor without it.
BWD_FLOOR = {"rgbsigma": 63.0, "feat": 2.0, "z": 65.0, "rays_d": 75.0, "beta": 86.0, "cyc": 2.0}


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def _alpha_chain(rgbsigma, z, rays_d, beta, noise, xyz, clip, vis_pred, exp_form=False):
    rs, z, rd = _f64(rgbsigma), _f64(z), _f64(rays_d)
    N, S = z.shape
    sraw = rs[..., 3]
    dnorm = np.sqrt((rd * rd).sum(-1))[:, None]
    zdiff = np.concatenate([z[:, 1:] - z[:, :-1], np.full((N, 1), 1e10)], -1)
    delta = zdiff * dnorm
    ib = 1.0 / (abs(float(np.asarray(beta, np.float64).reshape(-1)[0])) + 1e-9)
    sg = sraw if noise is None else sraw + _f64(noise)
    sdf = -sg
    x = -np.abs(sdf) * ib
    em = np.expm1(x)
    sgn = np.sign(sdf)
    p = 0.5 + 0.5 * sgn * em                # the reference's form; in float64 it still cancels to 1e-16 / e^x relative, so the
    if exp_form:                            # gradients' truth is written on the form without the cancellation (torch_forward)
        p = np.where(sdf > 0, 0.5 * np.exp(x), np.where(sdf < 0, 1.0 - 0.5 * np.exp(x), 0.5))
    dens = p * ib
    y = -delta * dens
    ey = np.exp(y)
    masked = np.zeros((N, S), bool)
    if clip is not None:
        masked |= (np.abs(_f64(xyz)) > _f64(clip).reshape(1, 1, 3)).any(-1)
    if vis_pred is not None:
        masked |= _f64(vis_pred) < 0.5
    alpha = np.where(masked, 0.0, 1.0 - ey)
    return dict(rs=rs, z=z, rd=rd, N=N, S=S, sraw=sraw, dnorm=dnorm, zdiff=zdiff, delta=delta, ib=ib, sdf=sdf, x=x, em=em, sgn=sgn,
                p=p, dens=dens, y=y, ey=ey, masked=masked, alpha=alpha, has_noise=noise is not None)


def _excl_cumprod(t):
    return np.concatenate([np.ones_like(t[:, :1]), np.cumprod(t, -1)[:, :-1]], -1)


def _semantic(c, rgb_filter_scale):
    """Per-sample colour factor and the roundings of one colour term (module docstring)."""
    N, S = c["N"], c["S"]
    if rgb_filter_scale > 0:
        sem = rgb_filter_scale / (1.0 + np.exp(10.0 * c["sraw"]))
        sem[:, -1] = 0.0
        return sem, 7.0 + 10.0 * np.abs(c["sraw"])
    return np.ones((N, S)), np.ones((N, S))


def forward(rgbsigma, feat, z, rays_d, beta, noise=None, xyz=None, clip=None, vis_pred=None, cyc=None, rgb_filter_scale=0.0,
            n_live=None, term_tau=0.0):
    """-> {name: (float64 value, bound)} for weights, visibility (N, S), rgb (N, 3), feat (N, F), depth, sil, vis_out, cyc_out (N,)
    (None where the entry point returns none), 'n_used': (N,) int and 'abs_sums': {sum: sum_i |w_i c_i|}.  With n_live / term_tau the weights behind the cut are
    exactly 0 (bound 0); visibility is 0 at and behind n_live and is T elsewhere (behind a term_tau cut the entry point writes T
    inside the cut's block of 64 and 0 behind it: not restated, not compared)."""
    c = _alpha_chain(rgbsigma, z, rays_d, beta, noise, xyz, clip, vis_pred)
    N, S, alpha = c["N"], c["S"], c["alpha"]
    t = 1.0 - alpha + 1e-10
    T = _excl_cumprod(t)
    idx = np.arange(S)[None]
    s_end = np.full((N,), S) if n_live is None else np.minimum(np.asarray(n_live, np.int64).reshape(N), S)
    used = s_end.copy()
    if term_tau > 0:
        dead = (T < term_tau) & (idx < s_end[:, None])
        used = np.where(dead.any(-1), np.argmax(dead, -1), s_end)
    live = idx < used[:, None]
    w = np.where(live, alpha * T, 0.0)
    vis = np.where(idx < s_end[:, None], T, 0.0)

    # ---- eps_i and the running bound
    cx = 4.0 if c["has_noise"] else 3.0
    with np.errstate(over="ignore", invalid="ignore"):
        E_em = C_EXP * U * np.abs(c["em"]) + np.exp(c["x"]) * cx * U * np.abs(c["x"])
        E_p = 0.5 * E_em + U * np.abs(c["p"])
        E_dens = c["ib"] * E_p + (1.0 + C_IBETA) * U * c["dens"]
        E_y = np.abs(c["delta"]) * E_dens + (C_DELTA + 1.0) * U * np.abs(c["y"])
        eps = np.exp(np.minimum(c["y"] + E_y, 0.0)) - c["ey"] + C_EXP * U * c["ey"] + U * (1.0 - c["ey"])
    eps = np.where(c["masked"], 0.0, np.minimum(eps, 1.0))
    E_T = np.zeros((N, S))
    E_w = np.zeros((N, S))
    E = np.zeros(N)
    for i in range(S):
        E_T[:, i] = E
        E_w[:, i] = E * alpha[:, i] + T[:, i] * eps[:, i] + U * alpha[:, i] * T[:, i]
        E = E * t[:, i] + T[:, i] * (eps[:, i] + 2.0 * U * t[:, i]) + U * T[:, i] * t[:, i]
    raw = {"E_w": E_w, "E_T": E_T, "eps": eps}
    E_w = np.where(live, E_w, 0.0)
    E_T = np.where(idx < s_end[:, None], E_T, 0.0)
    tiny = lambda b: b + TINY * (b > 0)

    G = (S + 31) // 32
    depth_seq = S - np.maximum(np.arange(S), 1)
    depth_ker = 5 + G - np.arange(S) // 32
    d = np.maximum(depth_seq, depth_ker).astype(np.float64)[None]

    def wsum(coef, wt=w, Ewt=E_w, r=1.0):
        """sum_i wt_i coef_i over the samples and its bound; coef (N, S) or (N, S, C)."""
        coef = _f64(coef)
        if coef.ndim == 3:
            wt, Ewt, dd, rr = wt[..., None], Ewt[..., None], d[..., None], (r[..., None] if np.ndim(r) else r)
        else:
            dd, rr = d, r
        term = wt * coef
        abs_sums.append(np.abs(term).sum(1))
        return term.sum(1), tiny((np.abs(coef) * Ewt + (rr + dd) * U * np.abs(term)).sum(1))

    abs_sums = []
    sem, r_sem = _semantic(c, rgb_filter_scale)
    out = {"weights": (w, tiny(E_w)), "visibility": (vis, tiny(E_T)), "n_used": used}
    out["rgb"] = wsum(c["rs"][..., :3], w * sem, E_w * sem, r_sem)
    out["feat"] = None if feat is None else wsum(feat)
    out["depth"] = wsum(c["z"])
    notlast = (idx < S - 1).astype(np.float64) * np.ones((N, 1))
    out["sil"] = wsum(notlast, r=0.0)
    out["vis_out"] = None if vis_pred is None else wsum(vis_pred)
    out["cyc_out"] = None if cyc is None else wsum(cyc)
    out["errors"] = raw                     # the recurrences themselves: E_w, E_T, eps (N, S), before any termination
    out["abs_sums"] = dict(zip([k for k in SUMS if out[k] is not None], abs_sums))      # sum_i |w_i c_i|: a sum's own scale
    return out


def ratio(got, ref, bound):
    """|got - ref| / bound per element; 0 where both vanish, inf where only the bound does (an exact statement missed)."""
    diff = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff == 0, 0.0, np.inf))


# ------------------------------------------------------------------------------------------------------------------------ backward
def torch_forward(rgbsigma, feat, z, rays_d, beta, noise=None, xyz=None, clip=None, vis_pred=None, cyc=None, rgb_filter_scale=0.0,
                  exp_form=False):
    """The restatement in torch, in the dtype of its arguments (float64: the truth; float32: the figure a plain fp32 autograd
    reaches).  -> dict rgb, feat, depth, sil, weights, cyc_out (None where absent).
    exp_form: p written as 0.5 e^x (sdf > 0), 1 - 0.5 e^x (sdf < 0), 0.5 (sdf = 0) instead of 0.5 + 0.5 sgn expm1(x) -- the same
    function, but autograd differentiates expm1 as (result + 1), which at x = -30 cancels to 1e-3 relative even in float64."""
    rgbs, sraw = rgbsigma[..., :3], rgbsigma[..., 3]
    deltas = z[:, 1:] - z[:, :-1]
    deltas = torch.cat([deltas, torch.full_like(z[:, :1], 1e10)], -1) * rays_d.norm(dim=-1, keepdim=True)
    semantic = rgb_filter_scale * torch.sigmoid(-10 * sraw)
    sg = sraw if noise is None else sraw + noise
    ib = 1 / (beta.abs() + 1e-9)
    sdf = -sg
    if exp_form:
        e = torch.exp(-sdf.abs() * ib)
        dens = torch.where(sdf > 0, 0.5 * e, torch.where(sdf < 0, 1 - 0.5 * e, torch.full_like(e, 0.5))) * ib
    else:
        dens = (0.5 + 0.5 * sdf.sign() * torch.expm1(-sdf.abs() * ib)) * ib
    alphas = 1 - torch.exp(-deltas * dens)
    if clip is not None:
        alphas = torch.where((xyz.abs() > clip.reshape(1, 1, 3)).any(-1), torch.zeros_like(alphas), alphas)
    if vis_pred is not None:
        alphas = torch.where(vis_pred < 0.5, torch.zeros_like(alphas), alphas)
    shifted = torch.cat([torch.ones_like(alphas[:, :1]), 1 - alphas + 1e-10], -1)
    T = torch.cumprod(shifted, -1)[:, :-1]
    w = alphas * T
    if rgb_filter_scale > 0:
        rgb = ((w[:, :-1] * semantic[:, :-1])[..., None] * rgbs[:, :-1]).sum(-2)
    else:
        rgb = (w[..., None] * rgbs).sum(-2)
    return {"rgb": rgb, "feat": None if feat is None else (w[..., None] * feat).sum(-2), "depth": (w * z).sum(-1),
            "sil": w[:, :-1].sum(-1), "weights": w, "cyc_out": None if cyc is None else (w.detach() * cyc).sum(-1)}


GRAD_INPUTS = ("rgbsigma", "feat", "z", "rays_d", "beta", "cyc")


def gradients(inputs, g, dtype=torch.float64, rgb_filter_scale=0.0, exp_form=None):
    """inputs: dict of numpy arrays (rgbsigma, feat, z, rays_d, beta, noise, xyz, clip, vis_pred, cyc; None = absent); g: dict
    output name -> numpy gradient (None / absent = that output is not differentiated).  -> dict of float64 numpy gradients
    (None where the input is absent or nothing reaches it), computed in `dtype`; exp_form (torch_forward) defaults to True in
    float64 (the truth) and False in float32 (the reference's own formula)."""
    exp_form = (dtype == torch.float64) if exp_form is None else exp_form
    t = {k: (None if v is None else torch.from_numpy(np.array(v)).to(dtype)) for k, v in inputs.items()}
    for k in GRAD_INPUTS:
        if t.get(k) is not None:
            t[k].requires_grad_(True)
    out = torch_forward(t["rgbsigma"], t.get("feat"), t["z"], t["rays_d"], t["beta"], t.get("noise"), t.get("xyz"), t.get("clip"),
                        t.get("vis_pred"), t.get("cyc"), rgb_filter_scale, exp_form)
    loss = 0
    for k, gv in g.items():
        if gv is not None and out.get(k) is not None:
            loss = loss + (out[k] * torch.from_numpy(np.array(gv)).to(dtype)).sum()
    loss.backward()
    return {k: (None if t.get(k) is None or t[k].grad is None else t[k].grad.double().numpy()) for k in GRAD_INPUTS}


def _analytic(inputs, g, rgb_filter_scale, absolute):
    c = _alpha_chain(inputs["rgbsigma"], inputs["z"], inputs["rays_d"], inputs["beta"], inputs.get("noise"), inputs.get("xyz"),
                     inputs.get("clip"), inputs.get("vis_pred"), exp_form=True)
    N, S, alpha = c["N"], c["S"], c["alpha"]
    A = np.abs if absolute else (lambda v: v)
    t = 1.0 - alpha + 1e-10
    T = _excl_cumprod(t)
    w = alpha * T
    wE, TE, tE = w, T, 0.0
    if absolute:                            # what an fp32 weight / transmittance / divisor may be off by: the forward's own bounds
        err = forward(inputs["rgbsigma"], None, inputs["z"], inputs["rays_d"], inputs["beta"], inputs.get("noise"), inputs.get("xyz"),
                      inputs.get("clip"), inputs.get("vis_pred"))["errors"]
        wE, TE, tE = err["E_w"] + U * w, err["E_T"] + U * T, (err["eps"] + 2.0 * U * t) / t
    sem, _ = _semantic(c, rgb_filter_scale)
    gz = lambda k, shape: np.zeros(shape) if g.get(k) is None else _f64(g[k])
    g_rgb, g_d, g_s, g_w = gz("rgb", (N, 3)), gz("depth", (N,)), gz("sil", (N,)), gz("weights", (N, S))
    feat, cyc = _f64(inputs.get("feat")), _f64(inputs.get("cyc"))
    g_f = None if (feat is None or g.get("feat") is None) else _f64(g["feat"])
    g_c = None if (cyc is None or g.get("cyc_out") is None) else _f64(g["cyc_out"])
    notlast = (np.arange(S)[None] < S - 1).astype(np.float64)
    grgb = A(g_rgb[:, None, :] * c["rs"][..., :3]).sum(-1)
    v = sem * grgb + A(g_d[:, None] * c["z"]) + notlast * A(g_s)[:, None] + A(g_w)
    if g_f is not None:
        v = v + A(g_f[:, None, :] * feat).sum(-1)
    suffix_of = lambda q: np.concatenate([np.cumsum(q[:, ::-1], -1)[:, ::-1][:, 1:], np.zeros((N, 1))], -1)
    if absolute:
        dalpha = v * TE + suffix_of(v * wE) / t + suffix_of(v * w) / t * tE
        dalpha_mag = np.where(c["masked"], 0.0, v * T + suffix_of(v * w) / t)
    else:
        dalpha = v * T - suffix_of(v * w) / t
    dalpha = np.where(c["masked"], 0.0, dalpha)
    ex = np.exp(c["x"])
    dens = (0.5 + 0.5 * np.abs(c["em"])) * c["ib"] if absolute else c["dens"]
    ddens = dalpha * A(c["delta"]) * c["ey"]
    ddelta = dalpha * dens * c["ey"]
    if absolute:                            # the factor 1 - alpha = expf(y) is off by eps in ABSOLUTE terms, like alpha itself: at the
        ddens = ddens + dalpha_mag * np.abs(c["delta"]) * err["eps"]      # last sample of a ray in empty space (delta = 1e10) fp32
        ddelta = ddelta + dalpha_mag * dens * err["eps"]                  # has it at 1 where it is 0, or the other way round
    dsig = np.where(c["sdf"] == 0, 0.0, ddens * 0.5 * c["ib"] ** 2 * ex)
    if rgb_filter_scale > 0:
        s10 = 1.0 / (1.0 + np.exp(10.0 * c["sraw"]))
        k = 10.0 * rgb_filter_scale * s10 * (1.0 - s10) * notlast
        dsig = dsig + wE * grgb * (k if absolute else -k)
    out = {"rgbsigma": np.concatenate([(wE * sem)[..., None] * A(g_rgb)[:, None, :], dsig[..., None]], -1)}
    out["feat"] = None if g_f is None else wE[..., None] * A(g_f)[:, None, :]
    out["cyc"] = None if g_c is None else A(g_c)[:, None] * wE
    dzl = ddelta * c["dnorm"] * notlast
    dz = wE * A(g_d)[:, None] + (dzl if absolute else -dzl)
    dz[:, 1:] += dzl[:, :-1]
    out["z"] = dz
    a_dn = (ddelta * A(c["zdiff"])).sum(-1)
    out["rays_d"] = a_dn[:, None] * A(c["rd"]) / c["dnorm"]
    xa = np.abs(c["sdf"]) * c["ib"]
    if absolute:
        ddib = (0.5 + 0.5 * np.abs(c["em"])) + 0.5 * xa * ex
    else:
        ddib = c["p"] - 0.5 * c["sgn"] * xa * ex
    b = float(np.asarray(inputs["beta"], np.float64).reshape(-1)[0])
    s_ = (ddens * ddib).sum() * c["ib"] ** 2
    out["beta"] = np.asarray([s_ if absolute else -np.sign(b) * s_])
    return out


def analytic(inputs, g, rgb_filter_scale=0.0):
    """The gradients by the closed form the kernel follows (float64); pinned to autograd by the CPU test."""
    return _analytic(inputs, g, rgb_filter_scale, False)


def condition(inputs, g, rgb_filter_scale=0.0):
    """analytic() with every term replaced by its absolute value and every weight, transmittance and divisor by what fp32 may have
    it off by: the scale each gradient element is judged on (module docstring)."""
    return {k: (None if v is None else v + TINY * (v > 0)) for k, v in _analytic(inputs, g, rgb_filter_scale, True).items()}


def backward_reference(inputs, g, rgb_filter_scale=0.0):
    """-> {input: None (nothing reaches it: the gradient must be absent or 0) or (truth, condition, of, bar)}: truth the float64
    gradient (zeros where autograd returns none), of the worst |g32 - truth| / condition of float32 torch autograd through the
    restatement, the smaller of its two forms (autograd differentiates expm1(x) as result + 1, which is 0 in fp32 past
    |sdf| / beta = 17 and puts that form's d sigma figure at 1 / u; a form that overflows counts as 0), bar = max(BWD_FLOOR,
    4 x of)."""
    truth = gradients(inputs, g, rgb_filter_scale=rgb_filter_scale)
    g32 = [gradients(inputs, g, dtype=torch.float32, rgb_filter_scale=rgb_filter_scale, exp_form=e) for e in (False, True)]
    cond = condition(inputs, g, rgb_filter_scale)
    out = {}
    for k in GRAD_INPUTS:
        if cond[k] is None:
            out[k] = None
            continue
        zero = lambda v: np.zeros_like(cond[k]) if v is None else v
        figs = [ratio(zero(q[k]), zero(truth[k]), cond[k]) for q in g32]
        of = min(float(np.where(np.isfinite(f), f, 0.0).max()) for f in figs)
        out[k] = (zero(truth[k]), cond[k], of, max(BWD_FLOOR[k], 4.0 * of))
    return out
