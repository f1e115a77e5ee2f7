"""GPU (-m gpu): compositing forward (csrc/moda_dev.h composite_ray through moda_composite_fwd, both instantiations) and backward
(csrc/train_kernels.hip composite_bwd_kernel through autograd.CompositeFn) PER ELEMENT against the float64 reference of
tests/composite_numpy.py, on the cases tests/test_composite_oracle.py builds and vets on the CPU.  fp32; u = 2^-24.

forward      S in {1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 200}, five ray kinds x nine rays (one launch per kind: beta is a
             launch-wide scalar) and one launch of a single ray; options all on (noise, clip, vis_pred, cyc), all on with
             rgb_filter_scale 1.3, all off.  Every weight, transmittance and sum: |got - ref| / bound <= max(1, 4 x the float32
             oracle's worst figure for that output on the same case, computed at run time).  The floor is 1 because the counted
             roundings are inside the bound (composite_numpy's docstring); the factor 4 covers the kernel's association (32-lane
             scan times carried prefix, butterfly sums) against the oracle's sequential ones.  Nothing is excluded: on empty rays
             the last weight's bound is its transmittance, and says so.
             F = 16 (16-byte loads), F = 3 (scalar loads), F = 16 from a buffer 4 bytes off alignment (bit for bit the aligned
             run) and feat = None (composite_kernel<false>: rgb, depth, sil, weights, visibility, vis_out, cyc_out bit for bit the
             F = 16 run).  Exact: masked samples weigh 0, a wholly masked ray has every sum 0 and visibility 1, and where the last
             alpha is 1 the weights add up to 1 within their bounds.
termination  term_tau: rays whose transmittance is exactly 1 in front of sample c - 1 (masked) and collapses there (alpha = 1), c in
             {1, 31, 32, 33, 63, 64, 65, 127, 128, S - 1}, and two rays that never terminate: n_used == c, weights in front of the
             cut bit-equal to the unterminated run, 0 behind, every sum within tau (times the coefficients' size).  feat and cyc
             behind the cut are NaN and reach no output.  rgbsigma, noise, xyz and vis_pred behind a tau cut ARE still loaded
             inside the cut's block of 64 (the cut is only known after the scan), so they stay finite.
             n_live in {0, 1, 32, 33, 64, 65, S, S + 5}: rgbsigma, feat, noise, xyz, vis_pred and cyc are NaN at and behind the
             bound and the depths are NaN behind z[n_live] (the last live sample's delta reads that one depth); outputs finite,
             n_used == min(n_live, S), weights in front of the bound bit-equal to the unterminated ones.
backward     S in {1, 2, 33, 64, 65, 129, 200}, the same cases; gradient sets all / weights only / sil only / depth + cyc / all
             with feat = None / all with F = 3 / all with rgb_filter_scale 1.3 / all with every option off.  Every element of
             d_rgbsigma, d_feat, d_z, d_cyc, d_rays_d and d_beta: |got - truth| / condition <= max(floor, 4 x the figure float32
             torch autograd through the restatement reaches on the same case).  truth = float64 autograd.  condition = the
             element's closed form with every term in absolute value and every weight, transmittance, divisor and expf(y) factor
             replaced by its fp32 error bound (composite_numpy.condition).  floor = composite_numpy.BWD_FLOOR, the relative
             roundings one term gathers in the kernel, counted there per output: d_feat and d_cyc 2, d_rgbsigma 63, d_z 65,
             d_rays_d 75, d_beta 86, whatever S.  The float32 figure is the smaller of the restatement's two forms: autograd
             differentiates expm1(x) as result + 1, which is 0 in fp32 past |sdf| / beta = 17 and puts that form's d sigma figure
             at 1 / u.  A condition of 0 is an exact statement: masked samples have d sigma = d rgb = 0.  d_feat from a buffer
             4 bytes off equals the aligned route bit for bit; two runs give bit-identical d_rgbsigma, d_feat and d_z (at most two
             atomic adds onto zero per d_z element); d_beta (atomics across rays) is held to its bar only.  Every gradient is
             finite, the saturated rays included.
             tests/test_composite_oracle.py holds an fp32 numpy model of composite_bwd_kernel to the same bar on the CPU: it stays
             under 10 (d_rgbsigma on the empty rays of S = 2, where float32 autograd reaches 9.3; under 1.01 everywhere else but
             3.6 on surface S = 2), and with `s + 1 < S` written as `s < S` in its sil term it fails on every kind, every S >= 2
             and both gradient sets that hold sil, at 513 (surface, S = 129, all outputs) and up.

Every test prints the worst figure per (S, kind, output) of the kernel beside the float32 reference's on the same case (forward:
the numpy oracle; backward: torch autograd; run with -s).  On the CPU the float32 oracle's forward figures are at most 0.93
(weights), 0.50 (visibility) and 0.56 (sums) of the bound outside the empty rays' last samples, where they reach 1.00.
Measured on an MI355X, worst over S and the option / gradient sets, kernel / float32 reference:
  forward  soft     weights 0.31 / 0.92, visibility 0.14 / 0.38, rgb 0.13 / 0.21, feat 0.14 / 0.23, depth 0.06 / 0.06, sil 0.17 / 0.33,
                    vis_out 0.04 / 0.06, cyc_out 0.06 / 0.13
  forward  surface  weights 0.50 / 0.76, visibility 0.50 / 0.50, rgb 0.10 / 0.51, feat 0.16 / 0.42, depth 0.07 / 0.07, sil 0.19 / 0.51,
                    vis_out 0.06 / 0.06, cyc_out 0.06 / 0.11
  forward  empty    weights 1.00 / 1.00, visibility 0.34 / 0.43, rgb 1.00 / 1.00, feat 1.00 / 1.00, depth 1.00 / 1.00, sil 0.56 / 0.56,
                    vis_out 1.00 / 1.00, cyc_out 1.00 / 1.00   (the last weight, 0 in fp32 and T in float64 or the other way round)
  forward  masked   weights 0.30 / 0.89, visibility 0.16 / 0.32, rgb 0.09 / 0.12, feat 0.14 / 0.36, depth 0.06 / 0.06, sil 0.12 / 0.43,
                    vis_out 0.06 / 0.07, cyc_out 0.03 / 0.07
  forward  ties     weights 0.29 / 0.91, visibility 0.10 / 0.21, rgb 0.03 / 0.06, feat 0.05 / 0.07, depth 0.02 / 0.02, sil 0.02 / 0.04,
                    vis_out 0.01 / 0.03, cyc_out 0.02 / 0.03
  backward soft     d_rgbsigma 0.50 / 0.50, d_feat 0.30 / 0.25, d_z 0.22 / 0.15, d_rays_d 0.37 / 0.31, d_beta 0.06 / 0.01, d_cyc 0.30 / 0.25
  backward surface  d_rgbsigma 3.63 / 3.63, d_feat 0.48 / 0.48, d_z 0.36 / 0.36, d_rays_d 0.55 / 0.27, d_beta 0.00 / 0.00, d_cyc 0.45 / 0.45
  backward empty    d_rgbsigma 9.34 / 9.34, d_feat 1.00 / 0.25, d_z 1.00 / 0.00, d_rays_d 0.04 / 0.00, d_beta 0.00 / 0.00, d_cyc 1.00 / 0.25
  backward masked   d_rgbsigma 0.36 / 0.41, d_feat 0.30 / 0.25, d_z 0.10 / 0.15, d_rays_d 0.21 / 0.15, d_beta 0.02 / 0.01, d_cyc 0.28 / 0.23
  backward ties     d_rgbsigma 0.30 / 0.25, d_feat 0.30 / 0.25, d_z 0.70 / 0.54, d_rays_d 0.01 / 0.01, d_beta 0.00 / 0.00, d_cyc 0.30 / 0.25
(d_rgbsigma 3.63 and 9.34: d sigma of the first sample at S = 2 under the sil-only set, kernel and float32 autograd alike.)"""
import numpy as np
import pytest
import torch

import composite_numpy as cn
import test_composite_oracle as C

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import moda_amd
    from moda_amd import rendering as R, autograd as A
    from gpu_helpers import DEV


def np_(t):
    return None if t is None else t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def T(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def off_by_4_bytes(a):
    """A contiguous device copy of `a` that starts 4 bytes past a 16-byte boundary."""
    buf = torch.zeros(a.size + 4, device=DEV)
    v = buf[1:1 + a.size].view(*a.shape)
    v.copy_(T(a))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.fixture(autouse=True)
def _fp32():
    moda_amd.set_precision("fp32")
    yield
    moda_amd.set_precision("fp32")


def run_forward(a, scale, feat_off=False, **term):
    with torch.no_grad():
        feat = None if a["feat"] is None else (off_by_4_bytes(a["feat"]) if feat_off else T(a["feat"]))
        o = R.composite(T(a["rgbsigma"]), feat, T(a["z"]), T(a["rays_d"]), T(a["beta"]), noise=T(a["noise"]), xyz=T(a["xyz"]),
                        clip_bound=None if a["clip"] is None else np.array(a["clip"]), vis_pred=T(a["vis_pred"]), cyc=T(a["cyc"]),
                        rgb_filter_scale=scale, **term)
    return {k: np_(v) for k, v in o.items()}


def check_forward(got, ref, o32, tag, worst):
    for k in cn.PER_SAMPLE + cn.SUMS:
        if ref[k] is None:
            assert got[k] is None, (tag, k)
            continue
        assert got[k].dtype == np.float32 and got[k].shape == ref[k][0].shape, (tag, k)
        fig = cn.ratio(got[k], *ref[k])
        kf, of = float(fig.max()), float(o32[k].max())
        w = worst.setdefault(k, [0.0, 0.0])
        w[0], w[1] = max(w[0], kf), max(w[1], of)
        assert kf <= max(cn.FWD_FLOOR, 4.0 * of), (tag, k, kf, of, np.unravel_index(np.argmax(fig), fig.shape))


def exact_statements(got, a, ref, tag):
    ch = cn._alpha_chain(a["rgbsigma"], a["z"], a["rays_d"], a["beta"], a["noise"], a["xyz"], a["clip"], a["vis_pred"])
    masked = ch["masked"]
    assert (got["weights"][masked] == 0).all(), tag
    whole = masked.all(-1)
    for k in cn.SUMS:
        if got[k] is not None:
            assert (got[k][whole] == 0).all(), (tag, k)
    assert (got["visibility"][whole] == 1).all(), tag
    closes = (np.float32(ch["alpha"][:, -1]) == 1)
    w, Ew = ref["weights"]
    gap = np.abs(got["weights"].astype(np.float64).sum(-1) - 1.0)
    assert (gap[closes] <= (Ew.sum(-1) + np.abs(1.0 - w.sum(-1)))[closes]).all(), (tag, gap[closes].max())


@pytest.mark.parametrize("S", C.CASE_S)
def test_forward_per_element_against_float64(S):
    for kind in C.KINDS:
        worst = {}
        for opt, noise, masks, cyc, scale in C.OPTIONS:
            tag = (S, kind, opt)
            c = C.case(S, kind)
            a16, a3, a0 = (C.select(c, noise, masks, cyc, F) for F in (16, 3, 0))
            g16, g3, g0 = run_forward(a16, scale), run_forward(a3, scale), run_forward(a0, scale)
            goff = run_forward(a16, scale, feat_off=True)
            check_forward(g16, C.reference(S, kind, opt, 16), C.oracle32_figures(S, kind, opt, 16), tag + (16,), worst)
            check_forward(g3, C.reference(S, kind, opt, 3), C.oracle32_figures(S, kind, opt, 3), tag + (3,), worst)
            for k in cn.PER_SAMPLE + cn.SUMS:
                if g16[k] is None:
                    continue
                assert np.array_equal(bits(goff[k]), bits(g16[k])), (tag, k, "4 bytes off")
                if k != "feat":
                    assert np.array_equal(bits(g0[k]), bits(g16[k])), (tag, k, "feat None")
                    assert np.array_equal(bits(g3[k]), bits(g16[k])), (tag, k, "F = 3")
            assert g0["feat"] is None
            exact_statements(g16, a16, C.reference(S, kind, opt, 16), tag)
        print(f"composite fwd S={S} {kind}: kernel / oracle32 " + ", ".join(f"{k} {v[0]:.3f} / {v[1]:.3f}" for k, v in worst.items()))
    # a launch of one ray: three idle waves in its workgroup
    worst = {}
    a = C.select(C.case(S, "soft", 1), True, True, True, 16)
    check_forward(run_forward(a, 0.0), C.reference(S, "soft", "all", 16, 1), C.oracle32_figures(S, "soft", "all", 16, 1), (S, "N=1"), worst)


# ----------------------------------------------------------------------------------------------------------------------- termination
TAU = 1e-3


def _cut_rays(S, cuts):
    """Rays whose transmittance is exactly 1 in front of sample c - 1 (masked by vis_pred) and collapses there (alpha = 1 in
    fp32), one per cut, then a wholly masked ray and a ray in empty space: those two never terminate."""
    rng = np.random.default_rng(4200 + S)
    N = len(cuts) + 2
    f32 = lambda x: np.ascontiguousarray(x, np.float32)
    z = f32(np.broadcast_to(np.linspace(0.1, 2.1, S), (N, S)))
    rd = rng.normal(size=(N, 3))
    rd = f32(rd / np.linalg.norm(rd, axis=-1, keepdims=True) * (50.0 * S / 200.0))       # delta / beta = 50 behind a surface
    rs = rng.uniform(0.1, 1.0, (N, S, 4))
    rs[..., 3] = 0.4                                            # sdf = -0.4: inside, density 1 / beta
    vis_pred = rng.uniform(0.55, 1.0, (N, S))
    for r, c in enumerate(cuts):
        vis_pred[r, :c - 1] = 0.2
    vis_pred[len(cuts)] = 0.1                                   # wholly masked: T = 1 throughout
    rs[len(cuts) + 1, :, 3] = -0.3                              # |sdf| / beta = 30 outside: alpha = 0 in fp32 up to the last sample
    return dict(rgbsigma=f32(rs), feat=f32(rng.normal(size=(N, S, 16))), z=z, rays_d=rd, beta=np.asarray([0.01], np.float32), noise=None,
                xyz=None, clip=None, vis_pred=f32(vis_pred), cyc=f32(rng.uniform(size=(N, S))))


@pytest.mark.parametrize("S", [200, 129])
def test_term_tau_cut_lands_on_the_chosen_sample(S):
    cuts = sorted({c for c in (1, 31, 32, 33, 63, 64, 65, 127, 128, S - 1) if 1 <= c < S})
    a = _cut_rays(S, cuts)
    want = np.asarray(cuts + [S, S], np.int32)
    behind = np.arange(S)[None] >= want[:, None]
    for F in (16, 3):
        full_in = dict(a, feat=np.ascontiguousarray(a["feat"][..., :F]))
        full = run_forward(full_in, 0.0)
        poisoned = dict(full_in, feat=full_in["feat"].copy(), cyc=a["cyc"].copy())
        poisoned["feat"][behind] = np.nan
        poisoned["cyc"][behind] = np.nan
        cut = run_forward(poisoned, 0.0, term_tau=TAU)
        assert np.array_equal(cut["n_used"], want), (S, F, cut["n_used"])
        assert np.array_equal(bits(cut["weights"][~behind]), bits(full["weights"][~behind])), (S, F)
        assert (cut["weights"][behind] == 0).all(), (S, F)
        coef = {"rgb": 1.0, "feat": float(np.abs(a["feat"]).max()), "depth": float(a["z"].max()), "sil": 1.0, "vis_out": 1.0, "cyc_out": 1.0}
        for k in cn.SUMS:
            assert np.isfinite(cut[k]).all(), (S, F, k)
            assert np.abs(cut[k].astype(np.float64) - full[k]).max() <= TAU * max(1.0, coef[k]), (S, F, k)


@pytest.mark.parametrize("S", [200, 65])
def test_n_live_bound_reads_nothing_behind_it(S):
    live = np.asarray([0, 1, 32, 33, 64, 65, S, S + 5], np.int32)
    c = C.case(S, "soft")
    a = {k: (v if v.ndim == 1 or k == "clip" else v[:len(live)]) for k, v in C.select(c, True, True, True, 16).items()}
    end = np.minimum(live, S)
    dead = np.arange(S)[None] >= end[:, None]
    for F in (16, 3):
        full_in = dict(a, feat=np.ascontiguousarray(a["feat"][..., :F]))
        full = run_forward(full_in, 0.0)
        p = {k: np.array(v) for k, v in full_in.items()}
        for k in ("rgbsigma", "feat", "noise", "xyz", "vis_pred", "cyc"):
            p[k][dead] = np.nan
        p["z"][np.arange(S)[None] > end[:, None]] = np.nan      # z[n_live] itself bounds the last live sample's delta
        lim = run_forward(p, 0.0, n_live=torch.from_numpy(live).to(DEV))
        assert np.array_equal(lim["n_used"], end), (S, F)
        for k in cn.PER_SAMPLE + cn.SUMS:
            assert np.isfinite(lim[k]).all(), (S, F, k)
        assert np.array_equal(bits(lim["weights"][~dead]), bits(full["weights"][~dead])), (S, F)
        assert (lim["weights"][dead] == 0).all(), (S, F)
        whole = end == S
        for k in cn.SUMS:
            assert np.array_equal(bits(lim[k][whole]), bits(full[k][whole])), (S, F, k)
            assert (lim[k][end == 0] == 0).all(), (S, F, k)


# -------------------------------------------------------------------------------------------------------------------------- backward
OUT_INDEX = {"rgb": 0, "feat": 1, "depth": 2, "sil": 3, "weights": 4, "cyc_out": 7}


def run_backward(a, g, scale, feat_off=False):
    """CompositeFn forward + backward of sum(g * out) -> {input: numpy gradient or None}."""
    leaf = lambda v: None if v is None else T(v).requires_grad_(True)
    rs, z, rd, beta, cyc = leaf(a["rgbsigma"]), leaf(a["z"]), leaf(a["rays_d"]), leaf(a["beta"]), leaf(a["cyc"])
    feat = feat_view = None
    if a["feat"] is not None:
        if feat_off:
            feat = torch.zeros(a["feat"].size + 4, device=DEV)
            feat[1:1 + a["feat"].size] = T(a["feat"]).reshape(-1)
            feat.requires_grad_(True)
            feat_view = feat[1:1 + a["feat"].size].view(*a["feat"].shape)
            assert feat_view.data_ptr() % 16 == 4
        else:
            feat = feat_view = leaf(a["feat"])
    o = A.CompositeFn.apply(rs, feat_view, z, rd, beta, T(a["noise"]), T(a["xyz"]), T(a["clip"]), T(a["vis_pred"]), cyc, scale)
    loss = None
    for k, gv in g.items():
        if gv is not None and o[OUT_INDEX[k]] is not None:
            term = (o[OUT_INDEX[k]] * T(gv)).sum()
            loss = term if loss is None else loss + term
    loss.backward()
    gf = None
    if feat is not None and feat.grad is not None:
        gf = np_(feat.grad[1:1 + a["feat"].size].view(*a["feat"].shape)) if feat_off else np_(feat.grad)
    grad = lambda t: None if t is None or t.grad is None else np_(t.grad)
    return {"rgbsigma": grad(rs), "feat": gf, "z": grad(z), "rays_d": grad(rd), "beta": grad(beta), "cyc": grad(cyc)}


def check_backward(got, a, g, scale, S, tag, worst):
    for k, r in cn.backward_reference(a, g, scale).items():
        if r is None:
            assert got[k] is None or not got[k].any(), (tag, k)
            continue
        truth, cond, of, bar = r
        gk = np.zeros_like(cond) if got[k] is None else got[k]
        assert np.isfinite(gk).all(), (tag, k)
        fig = cn.ratio(gk, truth, cond)
        kf = float(fig.max())
        w = worst.setdefault(k, [0.0, 0.0])
        w[0], w[1] = max(w[0], kf), max(w[1], of)
        assert kf <= bar, (tag, k, kf, of, np.unravel_index(np.argmax(fig), fig.shape))
    masked = cn._alpha_chain(a["rgbsigma"], a["z"], a["rays_d"], a["beta"], a["noise"], a["xyz"], a["clip"], a["vis_pred"])["masked"]
    assert (got["rgbsigma"][masked] == 0).all(), tag             # d rgb and d sigma of a masked sample: exactly 0


@pytest.mark.parametrize("S", C.BWD_S)
def test_backward_per_element_against_float64(S):
    for kind in C.KINDS:
        worst = {}
        c = C.case(S, kind)
        a16, a3, a0 = (C.select(c, True, True, True, F) for F in (16, 3, 0))
        for gset in C.GRAD_SETS:
            g = C.grads_for(S, kind, gset)
            got = run_backward(a16, g, 0.0)
            check_backward(got, a16, g, 0.0, S, (S, kind, gset), worst)
            if gset == "all":
                again = run_backward(a16, g, 0.0)
                for k in ("rgbsigma", "feat", "z"):
                    assert np.array_equal(bits(again[k]), bits(got[k])), (S, kind, k, "two runs")
                off = run_backward(a16, g, 0.0, feat_off=True)
                assert np.array_equal(bits(off["feat"]), bits(got["feat"])), (S, kind, "d_feat, 4 bytes off")
                check_backward(off, a16, g, 0.0, S, (S, kind, "4 bytes off"), worst)
        check_backward(run_backward(a0, C.grads_for(S, kind, "all", 0), 0.0), a0, C.grads_for(S, kind, "all", 0), 0.0, S,
                       (S, kind, "feat None"), worst)
        g3 = C.grads_for(S, kind, "all", 3)
        check_backward(run_backward(a3, g3, 0.0), a3, g3, 0.0, S, (S, kind, "F = 3"), worst)
        g = C.grads_for(S, kind, "all")
        check_backward(run_backward(a16, g, 1.3), a16, g, 1.3, S, (S, kind, "filter"), worst)
        plain = C.select(c, False, False, False, 16)
        gp = {k: v for k, v in g.items() if k != "cyc_out"}
        check_backward(run_backward(plain, gp, 0.0), plain, gp, 0.0, S, (S, kind, "plain"), worst)
        print(f"composite bwd S={S} {kind}: kernel / torch32 " + ", ".join(f"d_{k} {v[0]:.2f} / {v[1]:.2f}" for k, v in worst.items()))
