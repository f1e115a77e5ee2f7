"""CPU: the float64 reference of compositing (tests/composite_numpy.py) against oracle/moda_oracle.py::composite run in float64, the
G5 golden and float64 autograd through oracle/torch_ref.py::composite; the case builder tests/test_gpu_composite.py runs on the
device; and the conditions those cases must meet for its per-element bars to mean something.

Cases: S in CASE_S (a single sample, one ragged group, the group seams 32 / 64 / 96 / 128 and one past each, four blocks), RAYS = 9
rays of one kind per launch (not a multiple of the four waves of a workgroup; beta is one scalar per launch, so every kind is a
launch of its own), five kinds:
  soft     beta 0.1, sigma 0.05 N(0, 1): translucent fog, every sample matters.
  surface  beta 0.01, the sdf crosses zero once along the ray (slope 1 in depth, 0.002 of noise).  |d| is set per ray so that
           delta / beta behind the crossing is about 0.3, 3 and 30 (three rays each): at 30 alpha is EXACTLY 1 in fp32, t = 1e-10
           and the transmittance behind is round-off.  (The rays at 30 cross within the first tenth of their samples, those at 3
           within the first half: in front of the crossing every sample adds its delta u / beta of cancellation error to the
           bound.)
  empty    beta 0.01, sdf > 0 throughout with |sdf| / beta uniform in [2, 30]: the last sample's bound reaches its transmittance.
  masked   the soft rays with vis_pred < 0.5 on a prefix (1, S / 2, S - 1 samples), the clip mask on runs that straddle samples
           32 and 64, both masks on a third run, wholly masked rays (one by vis_pred, one by clip) and an alternating mask.
  ties     beta 0.1, every third depth equal to its predecessor (delta = 0, alpha exactly 0), sigma_raw exactly +0.0 and -0.0 at
           fixed samples and one noise value that cancels its sigma exactly (sdf = 0: the sign(0) = 0 branch).
Conditions asserted here: no bound of a soft / surface / masked / ties weight exceeds 1e-4 of its ray's largest weight, no bound of
a transmittance 1e-4 (of T_0 = 1), no bound of a sum 1e-4 of the larger of that weight and the sum of its terms' magnitudes (200 fog
samples of weight 0.003 add up to a silhouette of 0.5 whose summation alone is allowed 200 u); on empty rays only the last sample
and the sums that hold it may; the float32 oracle's own |oracle32 - ref| / bound is at most 8 outside those last samples (the bound
is a worst case, so it stays under 1)."""
import functools

import numpy as np
import pytest
import torch

import composite_numpy as cn
from oracle import moda_oracle as orc
from oracle import torch_ref as tr
from moda_amd import synth
from helpers import golden, oracle_scene, rel_err

CASE_S = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 200)
BWD_S = (1, 2, 33, 64, 65, 129, 200)
KINDS = ("soft", "surface", "empty", "masked", "ties")
RAYS = 9
FEAT = 16
BETA = {"soft": 0.1, "surface": 0.01, "empty": 0.01, "masked": 0.1, "ties": 0.1}
CLIP = np.asarray([0.5, 0.6, 0.7], np.float32)
ORACLE_CAP = 8.0
BOUND_CAP = 1e-4
# option sets: (name, noise, masks (clip + vis_pred), cyc, rgb_filter_scale)
OPTIONS = (("all", True, True, True, 0.0), ("filter", True, True, True, 1.3), ("plain", False, False, False, 0.0))


def _run_mask(S, lo, hi):
    m = np.zeros(S, bool)
    m[min(lo, S - 1):min(hi, S)] = True
    return m


@functools.lru_cache(maxsize=None)
def case(S, kind, N=RAYS):
    """-> dict of float32 arrays: rgbsigma (N, S, 4), feat (N, S, 16), z (N, S), rays_d (N, 3), beta (1,), noise (N, S),
    xyz (N, S, 3), clip (3,), vis_pred (N, S), cyc (N, S).  Read-only: shared between tests."""
    rng = np.random.default_rng(7000 + 31 * S + KINDS.index(kind))
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    z = f32(np.sort(0.1 + 0.4 * rng.uniform(size=(N, S)), -1))
    rd = rng.normal(size=(N, 3))
    rgb = rng.uniform(size=(N, S, 3))
    noise = f32(0.02 * rng.normal(size=(N, S)))
    vis_pred = rng.uniform(0.55, 1.0, (N, S))
    xyz = rng.uniform(-0.45, 0.45, (N, S, 3))                   # inside CLIP unless a mask moves it out
    beta = BETA[kind]
    if kind in ("soft", "masked", "ties"):
        sig = 0.05 * rng.normal(size=(N, S))
    elif kind == "surface":
        tau = np.asarray([0.3, 3.0, 30.0])[np.arange(N) % 3]
        frac = np.where(tau > 10, rng.uniform(0.0, 0.1, N), np.where(tau > 1, rng.uniform(0.1, 0.5, N), rng.uniform(0.1, 0.9, N)))
        zc = 0.1 + 0.4 * frac
        sdf = (zc[:, None] - z) + 0.002 * rng.normal(size=(N, S))
        sdf[:, -1] = -np.abs(sdf[:, -1]) - 0.02                 # every ray ends inside, however few samples it has
        sig = -sdf
        rd = rd / np.linalg.norm(rd, axis=-1, keepdims=True) * (tau * beta * S / 0.4)[:, None]
        noise = f32(0.1 * noise)
    else:                                                       # empty
        sig = -beta * rng.uniform(2.0, 30.0, (N, S))
        noise = f32(0.01 * noise)
    sig = f32(sig)
    if kind == "masked":
        r = lambda i: i % N
        for i, n in enumerate((1, S // 2, S - 1)):
            vis_pred[r(i), :n] = rng.uniform(0.0, 0.45, n)
        for i, (lo, hi) in zip((3, 4), ((30, 35), (60, 69))):
            xyz[r(i), _run_mask(S, lo, hi), i % 3] = 0.9
        m = _run_mask(S, 28, 70)
        xyz[r(5), m, 2] = -0.95
        vis_pred[r(5), m] = 0.2
        vis_pred[r(6)] = 0.1
        xyz[r(7), :, 0] = 0.51
        vis_pred[r(8), ::2] = 0.3
        xyz[r(8), 1::4, 1] = -0.61
    if kind == "ties":
        z[:, 1::3] = z[:, 0:-1:3][:, :z[:, 1::3].shape[1]]
        sig[:, 2::7] = 0.0
        sig[:, 5::7] = -0.0
        noise[:, 2::14] = 0.0                                   # sdf exactly 0 with the noise on, too
        k = min(4, S - 1)
        noise[0, k] = -sig[0, k]                                # one noise value that cancels its sigma exactly
        assert (np.diff(z, axis=-1) >= 0).all() and (S < 2 or (np.diff(z, axis=-1) == 0).any())
    out = dict(rgbsigma=f32(np.concatenate([rgb, sig[..., None]], -1)), feat=f32(rng.normal(size=(N, S, FEAT))), z=z, rays_d=f32(rd),
               beta=np.asarray([beta], np.float32), noise=noise, xyz=f32(xyz), clip=CLIP, vis_pred=f32(vis_pred),
               cyc=f32(rng.uniform(size=(N, S))))
    for v in out.values():
        v.setflags(write=False)
    return out


def select(c, noise, masks, cyc, F=FEAT):
    """The arguments of one option set: absent inputs are None; F = 0 drops the features, F < 16 keeps the first F channels."""
    return dict(rgbsigma=c["rgbsigma"], feat=None if F == 0 else np.ascontiguousarray(c["feat"][..., :F]), z=c["z"],
                rays_d=c["rays_d"], beta=c["beta"], noise=c["noise"] if noise else None, xyz=c["xyz"] if masks else None,
                clip=c["clip"] if masks else None, vis_pred=c["vis_pred"] if masks else None, cyc=c["cyc"] if cyc else None)


@functools.lru_cache(maxsize=None)
def reference(S, kind, opt, F=FEAT, N=RAYS):
    """composite_numpy.forward on one (case, option set); computed once, shared, not to be modified."""
    _, noise, masks, cyc, scale = next(o for o in OPTIONS if o[0] == opt)
    return cn.forward(**select(case(S, kind, N), noise, masks, cyc, F), rgb_filter_scale=scale)


def oracle_outputs(a, scale, dtype):
    """oracle/moda_oracle.py::composite in `dtype` on the arguments `a` -> the entry point's outputs by name (vis_out and cyc_out,
    which the oracle's tail composes from the weights, included)."""
    c = lambda v: None if v is None else np.asarray(v, dtype)
    rs, feat = c(a["rgbsigma"]), c(a["feat"])
    N, S = a["z"].shape
    oob = None if a["clip"] is None else (np.abs(c(a["xyz"])) > c(a["clip"])).sum(-1) > 0
    rgb, ft, depth, w, T, sil = orc.composite(rs[..., :3], rs[..., 3], np.zeros((N, S, 1), dtype) if feat is None else feat, c(a["z"]),
                                              c(a["rays_d"]), dtype(a["beta"][0]), noise=c(a["noise"]), oob=oob,
                                              vis_pred=c(a["vis_pred"]), rgb_filter_scale=scale)
    return {"weights": w, "visibility": T, "rgb": rgb, "feat": None if feat is None else ft, "depth": depth, "sil": sil,
            "vis_out": None if a["vis_pred"] is None else (w * c(a["vis_pred"])).sum(-1),
            "cyc_out": None if a["cyc"] is None else (w * c(a["cyc"])).sum(-1)}


@functools.lru_cache(maxsize=None)
def oracle32_figures(S, kind, opt, F=FEAT, N=RAYS):
    """{output: |oracle32 - ref| / bound per element} of the float32 oracle on one (case, option set)."""
    _, noise, masks, cyc, scale = next(o for o in OPTIONS if o[0] == opt)
    o32 = oracle_outputs(select(case(S, kind, N), noise, masks, cyc, F), scale, np.float32)
    ref = reference(S, kind, opt, F, N)
    return {k: cn.ratio(o32[k], *ref[k]) for k in cn.PER_SAMPLE + cn.SUMS if ref[k] is not None}


def last_sample_excluded(kind, name, fig):
    """The figures a cap applies to: on empty rays the last sample, and the sums that contain it, are set by whether fp32 sees a
    density at all (composite_numpy: eps reaches 1 there); everything else of every kind is held."""
    if kind != "empty":
        return fig
    if name in cn.PER_SAMPLE:
        return fig[:, :-1] if name == "weights" else fig
    return fig if name == "sil" else np.zeros(0)


GRAD_SETS = {
    "all": ("rgb", "feat", "depth", "sil", "weights", "cyc_out"),
    "weights": ("weights",),
    "sil": ("sil",),
    "depth+cyc": ("depth", "cyc_out"),
}


@functools.lru_cache(maxsize=None)
def output_grads(S, kind, N=RAYS):
    rng = np.random.default_rng(9000 + 31 * S + KINDS.index(kind))
    g = {"rgb": rng.normal(size=(N, 3)), "feat": rng.normal(size=(N, FEAT)), "depth": rng.normal(size=(N,)), "sil": rng.normal(size=(N,)),
         "weights": rng.normal(size=(N, S)), "cyc_out": rng.normal(size=(N,))}
    return {k: np.ascontiguousarray(v, np.float32) for k, v in g.items()}


def grads_for(S, kind, gset, F=FEAT):
    g = {k: v for k, v in output_grads(S, kind).items() if k in GRAD_SETS[gset]}
    if "feat" in g:
        g["feat"] = None if F == 0 else np.ascontiguousarray(g["feat"][:, :F])
    return g


# ------------------------------------------------------------------------------------------------------------ vetting the restatement
@pytest.mark.parametrize("kind", KINDS)
def test_reference_equals_the_oracle_in_float64(kind):
    for S in CASE_S:
        for opt, noise, masks, cyc, scale in OPTIONS:
            for F in (FEAT, 3, 0):
                a = select(case(S, kind), noise, masks, cyc, F)
                ref = reference(S, kind, opt, F)
                o64 = oracle_outputs(a, scale, np.float64)
                for k in cn.PER_SAMPLE + cn.SUMS:
                    if ref[k] is None:
                        assert o64[k] is None, k
                        continue
                    assert np.abs(ref[k][0] - o64[k]).max() <= 1e-12 * max(1.0, np.abs(o64[k]).max()), (S, kind, opt, F, k)
                assert (ref["n_used"] == S).all()


def test_reference_reproduces_the_g5_golden():
    g = golden("g5_composite")
    N, S = 9, 12
    scene = oracle_scene(5, 0)
    rays = synth.make_rays(5, N, 0)
    z, xyz = g["z"], g["xyz"]
    d_emb = orc.embedding(rays["rays_d"], 4, 10.0)
    fn = lambda x, sigma_only=False: orc.nerf_forward(scene.coarse, x, in_channels_dir=91)
    out = orc.evaluate_mlp(fn, xyz, embed_fn=lambda x: orc.embedding(x, 10, 10.0),
                           dir_embedded=np.broadcast_to(d_emb[:, None], (N, S, 27)), code=rays["env_code"], chunk=4096)
    beta = np.asarray([0.1], np.float32)
    o1 = cn.forward(out, np.zeros((N, S, 3), np.float32), z, rays["rays_d"], beta, noise=g["noise_randn"] * np.float32(0.5))
    vis_pred = synth.uniform(5, "g5/vis", (N, S))
    o2 = cn.forward(out, np.zeros((N, S, 3), np.float32), z, rays["rays_d"], beta, xyz=xyz, clip=np.asarray([0.12, 0.12, 0.25], np.float32),
                    vis_pred=vis_pred)
    names = {"rgb": "rgb", "feat": "feat", "depth": "depth", "weights": "weights", "vis": "visibility", "sil": "sil"}
    for tag, o in (("noise", o1), ("mask", o2)):
        for n, k in names.items():
            assert rel_err(o[k][0], g[f"{tag}_{n}"]) < 2e-5, (tag, n)


@pytest.mark.parametrize("kind", ("soft", "surface", "empty", "ties"))
def test_gradients_equal_float64_autograd_through_torch_ref(kind):
    """Unmasked cases (oracle/torch_ref.py::composite has no masks): composite_numpy.gradients == autograd through torch_ref in
    float64 to 1e-10 of each gradient's largest magnitude; and the closed form behind condition() == autograd, masks included."""
    TC = lambda a: torch.from_numpy(np.array(a)).double()
    for S in BWD_S:
        for scale in (0.0, 1.3):
            c = case(S, kind)
            a = select(c, True, False, True)
            g = grads_for(S, kind, "all")
            got = cn.gradients(a, g, rgb_filter_scale=scale, exp_form=False)      # torch_ref's own expm1 form
            rs, feat, z, rd, beta, cyc = (TC(a[k]).requires_grad_(True) for k in ("rgbsigma", "feat", "z", "rays_d", "beta", "cyc"))
            rgb, fo, depth, w, _, sil = tr.composite(rs[..., :3], rs[..., 3], feat, z, rd, beta, TC(a["noise"]), rgb_filter_scale=scale)
            co = (cyc * w.detach()).sum(-1)
            loss = sum((o * TC(g[k])).sum() for k, o in (("rgb", rgb), ("feat", fo), ("depth", depth), ("sil", sil), ("weights", w),
                                                        ("cyc_out", co)))
            loss.backward()
            for k, leaf in (("rgbsigma", rs), ("feat", feat), ("z", z), ("rays_d", rd), ("beta", beta), ("cyc", cyc)):
                want = leaf.grad.numpy()
                assert np.abs(got[k] - want).max() <= 1e-10 * max(np.abs(want).max(), 1e-30), (S, kind, scale, k)


@pytest.mark.parametrize("kind", KINDS)
def test_closed_form_behind_the_condition_figure_equals_autograd(kind):
    for S in BWD_S:
        for gset in GRAD_SETS:
            for scale, masks in ((0.0, True), (1.3, kind == "masked")):
                a = select(case(S, kind), True, masks, True)
                g = grads_for(S, kind, gset)
                want = cn.gradients(a, g, rgb_filter_scale=scale)
                got = cn.analytic(a, g, scale)
                cond = cn.condition(a, g, scale)
                for k in cn.GRAD_INPUTS:
                    if got[k] is None:
                        assert want[k] is None or not want[k].any(), (S, kind, gset, k)
                        continue
                    w_ = np.zeros_like(got[k]) if want[k] is None else want[k]
                    # to 1e-9 of what the element's own cancellation allows (cond / u = the sum of the terms' magnitudes)
                    assert (np.abs(got[k] - w_) <= 1e-9 * cond[k] / cn.U + 1e-300).all(), (S, kind, gset, scale, k)
                    assert (np.abs(w_) <= cond[k] / cn.U * (1 + 1e-9) + 1e-300).all(), (S, kind, gset, k)


# -------------------------------------------------------------------------------------------------------- conditions on the cases
@pytest.mark.parametrize("kind", KINDS)
def test_bounds_stay_small_and_the_float32_oracle_stays_inside_them(kind):
    worst = {}
    for S in CASE_S:
        for opt, *_ in OPTIONS:
            for F in (FEAT, 3):
                ref = reference(S, kind, opt, F)
                fig = oracle32_figures(S, kind, opt, F)
                wmax = np.abs(ref["weights"][0]).max(-1)
                whole = wmax == 0                                        # a wholly masked ray: every bound is 0
                for k in cn.PER_SAMPLE + cn.SUMS:
                    if ref[k] is None:
                        continue
                    val, bound = ref[k]
                    scale = wmax.reshape((-1,) + (1,) * (bound.ndim - 1))
                    if k in cn.SUMS:          # a sum of S spread weights is not of the size of one of them: at least its terms' magnitudes
                        scale = np.maximum(scale, ref["abs_sums"][k])
                    elif k == "visibility":   # transmittances start at 1
                        scale = np.ones_like(scale)
                    rel = np.where(whole.reshape((-1,) + (1,) * (bound.ndim - 1)), 0.0, bound / np.where(scale > 0, scale, 1.0))
                    assert k == "visibility" or (bound[whole] == 0).all(), (S, kind, opt, k)   # (T = (1 + 1e-10)^i rounds to 1)
                    held = last_sample_excluded(kind, k, rel)
                    assert held.size == 0 or held.max() <= BOUND_CAP, (S, kind, opt, F, k, float(held.max()))
                    f = last_sample_excluded(kind, k, fig[k])
                    if f.size:
                        worst[k] = max(worst.get(k, 0.0), float(f.max()))
                        assert f.max() <= ORACLE_CAP, (S, kind, opt, F, k, float(f.max()))
    print(f"composite {kind}: float32 oracle, worst |o32 - ref| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_empty_rays_last_sample_bound_reaches_the_transmittance():
    """The reference's formula in fp32 loses the density of a far sample (0.5 + 0.5 expm1(-|sdf| / beta) cancels to 0 past
    |sdf| / beta = 17) and the last delta is 1e10: the bound of that weight must be of the order of its transmittance on some ray,
    and the float32 oracle must actually differ from float64 by that much on some ray -- the bound says so, nothing is excluded."""
    ref = reference(64, "empty", "plain")
    w, Ew = ref["weights"]
    T = ref["visibility"][0]
    assert (Ew[:, -1] >= 0.5 * np.minimum(T[:, -1], 1.0)).any()
    o32 = oracle_outputs(select(case(64, "empty"), False, False, False), 0.0, np.float32)
    assert (np.abs(o32["weights"][:, -1] - w[:, -1]) > 0.01 * T[:, -1]).any()
    assert (cn.ratio(o32["weights"], w, Ew) <= 1.0).all()


def test_cases_hold_what_they_promise():
    for S in CASE_S:
        m = reference(S, "masked", "all")
        assert (m["weights"][0][6 % RAYS] == 0).all() and (m["weights"][0][7 % RAYS] == 0).all()
        c = case(S, "ties")
        sdf = -(c["rgbsigma"][..., 3] + c["noise"])
        if S > 4:
            assert sdf[0, 4] == 0 and c["rgbsigma"][0, 4, 3] != 0
            assert (reference(S, "ties", "all")["weights"][0][:, 0:-1:3][:, :c["z"][:, 1::3].shape[1]] == 0).all()
        if S >= 33:
            s = case(S, "surface")
            a = cn._alpha_chain(s["rgbsigma"], s["z"], s["rays_d"], s["beta"], None, None, None, None)["alpha"]
            assert (np.float32(a[:, :-1]) == 1).any(), S                 # saturated in front of the last sample


# ------------------------------------------------------------------------------------------- the bars against a wrong association
F32 = np.float32


def alpha32(a):
    """comp_alpha and its callers in fp32 numpy, operation for operation -> dict of float32 (N, S) arrays alpha (0 where masked), t,
    delta, zdiff, sdf, sgn, masked and the scalars ib, dnorm (N, 1)."""
    rs, z, rd = a["rgbsigma"], a["z"], a["rays_d"]
    N, S = z.shape
    dnorm = np.sqrt(rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1] + rd[:, 2] * rd[:, 2])[:, None]
    zdiff = np.concatenate([z[:, 1:] - z[:, :-1], np.full((N, 1), 1e10, F32)], -1)
    delta = zdiff * dnorm
    ib = F32(1) / (np.abs(a["beta"][0]) + F32(1e-9))
    sg = rs[..., 3] if a["noise"] is None else rs[..., 3] + a["noise"]
    sdf = -sg
    sgn = np.sign(sdf)
    dens = (F32(0.5) + F32(0.5) * sgn * np.expm1(-np.abs(sdf) * ib)) * ib
    alpha = F32(1) - np.exp(-delta * dens)
    masked = np.zeros((N, S), bool)
    if a["clip"] is not None:
        masked |= (np.abs(a["xyz"]) > a["clip"].reshape(1, 1, 3)).any(-1)
    if a["vis_pred"] is not None:
        masked |= a["vis_pred"] < F32(0.5)
    alpha = np.where(masked, F32(0), alpha)
    out = dict(alpha=alpha, t=F32(1) - alpha + F32(1e-10), delta=delta, zdiff=zdiff, sdf=sdf, sgn=sgn, masked=masked, ib=ib, dnorm=dnorm)
    assert all(np.asarray(v).dtype in (np.float32, np.bool_) for v in out.values())
    return out


def kernel_model(a, mutation=None):
    """fp32 numpy model of composite_ray's association on alpha32's alphas: groups of 32, T_i = carry_g * excl_i with excl the
    exclusive product inside the group and carry_g the earlier groups' totals multiplied in order.  Mutations:
    'carry'  -- the second group of every block of 64 takes the block's incoming carry instead of carry * total of the first group;
    'lane32' -- the exclusive value of that group's first lane is the first group's last inclusive product instead of 1.
    -> weights, visibility (float32)."""
    f = np.float32
    ch = alpha32(a)
    alpha, t = ch["alpha"], ch["t"]
    N, S = alpha.shape
    T = np.ones((N, S), f)
    carry = np.ones(N, f)
    for g0 in range(0, S, 32):
        tg = t[:, g0:g0 + 32]
        incl = np.cumprod(tg, -1, dtype=f)
        excl = np.concatenate([np.ones((N, 1), f), incl[:, :-1]], -1)
        second = (g0 // 32) % 2 == 1
        use = carry
        if second and mutation == "carry":
            use = prev_carry
        if second and mutation == "lane32":
            excl = excl.copy()
            excl[:, 0] = prev_last
        T[:, g0:g0 + 32] = use[:, None] * excl
        prev_carry, prev_last = carry, incl[:, -1]
        carry = (carry * incl[:, -1]).astype(f)
    return (alpha * T).astype(f), T


@pytest.mark.parametrize("kind", ("soft", "surface", "ties"))
def test_forward_bar_passes_the_kernels_association_and_fails_a_wrong_one(kind):
    """The assertion of the GPU test (|got - ref| / bound <= max(1, 4 x oracle32's figure)) on a numpy model of the kernel's
    association: it holds as the kernel multiplies, and fails at every S past one group when the second group of a block is given
    the wrong carry or the wrong first exclusive value -- both errors sit at samples 32 ... 63, 96 ... of a ray."""
    for S in CASE_S:
        a = select(case(S, kind), False, False, False)
        ref, fig32 = reference(S, kind, "plain"), oracle32_figures(S, kind, "plain")
        bar = {k: max(cn.FWD_FLOOR, 4.0 * float(fig32[k].max())) for k in cn.PER_SAMPLE}
        w, T = kernel_model(a)
        assert cn.ratio(w, *ref["weights"]).max() <= bar["weights"] and cn.ratio(T, *ref["visibility"]).max() <= bar["visibility"], S
        for mutation in ("carry", "lane32"):
            w, T = kernel_model(a, mutation)
            caught = cn.ratio(w, *ref["weights"]).max() > bar["weights"] or cn.ratio(T, *ref["visibility"]).max() > bar["visibility"]
            assert caught == (S > 32), (S, kind, mutation)


def backward_model(a, g, scale=0.0, mutation=None):
    """fp32 numpy model of composite_bwd_kernel on kernel_model's weights and transmittances, in the kernel's association: blocks of
    64 samples from the back, v w summed behind each sample by a six-step shift-and-add scan plus the carried suffix,
    dalpha = v T - excl / t, per-lane accumulators for |d| and beta closed by a butterfly, the rays' d_beta added in order.
    mutation 'sil': the silhouette gradient also reaches the last sample (`s + 1 < S` written as `s < S`).
    -> {input: float32 gradient or None}, as the entry point returns them."""
    f = F32
    ch = alpha32(a)
    w, T = kernel_model(a)
    N, S = w.shape
    rs, z, rd, ib, dnorm, delta, sdf, t = a["rgbsigma"], a["z"], a["rays_d"], ch["ib"], ch["dnorm"], ch["delta"], ch["sdf"], ch["t"]
    gz = lambda k, shape: np.zeros(shape, f) if g.get(k) is None else g[k]
    g_rgb, g_d, g_s, g_w = gz("rgb", (N, 3)), gz("depth", (N,)), gz("sil", (N,)), gz("weights", (N, S))
    g_f = None if (a["feat"] is None or g.get("feat") is None) else g["feat"]
    g_c = None if (a["cyc"] is None or g.get("cyc_out") is None) else g["cyc_out"]
    notlast = np.arange(S)[None] < S - 1
    sem, sg10 = np.ones((N, S), f), np.zeros((N, S), f)
    if scale > 0:
        sg10 = f(1) / (f(1) + np.exp(f(10) * rs[..., 3]))
        sem = np.where(notlast, f(scale) * sg10, f(0))
    grgb = g_rgb[:, None, 0] * rs[..., 0] + g_rgb[:, None, 1] * rs[..., 1] + g_rgb[:, None, 2] * rs[..., 2]
    v = sem * grgb + g_d[:, None] * z + (g_s[:, None] if mutation == "sil" else np.where(notlast, g_s[:, None], f(0))) + g_w
    if g_f is not None:
        for k in range(a["feat"].shape[-1]):
            v = v + g_f[:, None, k] * a["feat"][..., k]
    nblk = (S + 63) // 64
    pad = lambda q: np.concatenate([q, np.zeros((N, nblk * 64 - S), f)], -1)
    vw = pad(v * w)
    excl = np.zeros((N, nblk * 64), f)
    suffix = np.zeros((N, 1), f)
    for b in range(nblk - 1, -1, -1):
        x = vw[:, b * 64:b * 64 + 64]
        p = x.copy()
        for o in (1, 2, 4, 8, 16, 32):
            p = np.concatenate([p[:, :64 - o] + p[:, o:], p[:, 64 - o:]], -1)
        excl[:, b * 64:b * 64 + 64] = p - x + suffix
        suffix = suffix + p[:, :1]
    excl = excl[:, :S]
    dalpha = np.where(ch["masked"], f(0), v * T - excl / t)
    e = np.exp(-np.abs(sdf) * ib)
    dens = (f(0.5) + f(0.5) * ch["sgn"] * (e - f(1))) * ib
    one_m_a = np.exp(-delta * dens)
    ddens = dalpha * delta * one_m_a
    ddelta = dalpha * dens * one_m_a
    dsig = np.where(sdf == 0, f(0), ddens * f(0.5) * ib * ib * e)
    if scale > 0:
        dsig = np.where(notlast, dsig + w * grgb * (f(-10) * f(scale) * sg10 * (f(1) - sg10)), dsig)
    out = {"rgbsigma": np.concatenate([(w * sem)[..., None] * g_rgb[:, None, :], dsig[..., None]], -1)}
    out["feat"] = None if g_f is None else w[..., None] * g_f[:, None, :]
    out["cyc"] = None if g_c is None else g_c[:, None] * w
    xa = np.abs(sdf) * ib
    ddib = np.where(sdf > 0, f(0.5) * e * (f(1) - xa), np.where(sdf < 0, (f(1) - f(0.5) * e) + f(0.5) * xa * e, f(0.5)))

    def lanes(q):       # a lane's accumulator over its blocks from the back, then the 64-lane butterfly
        q = pad(q).reshape(N, nblk, 64)
        acc = np.zeros((N, 64), f)
        for b in range(nblk - 1, -1, -1):
            acc = acc + q[:, b]
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, np.arange(64) ^ o]
        return acc[:, 0]

    a_ib, a_dn = lanes(ddens * ddib), lanes(ddelta * ch["zdiff"])
    dzl = np.where(notlast, ddelta * dnorm, f(0))
    dz = w * g_d[:, None] - dzl
    dz[:, 1:] += dzl[:, :-1]
    out["z"] = dz
    out["rays_d"] = a_dn[:, None] * rd / dnorm
    k = -np.sign(a["beta"][0]) * ib * ib
    db = f(0)
    for n in range(N):
        db = db + a_ib[n] * k
    out["beta"] = np.asarray([db], f)
    assert all(v is None or v.dtype == np.float32 for v in out.values())
    return out


def _figures(got, ref):
    return {k: float(cn.ratio(np.zeros_like(r[1]) if got[k] is None else got[k], r[0], r[1]).max()) for k, r in ref.items() if r is not None}


@pytest.mark.parametrize("kind", KINDS)
def test_backward_bar_passes_the_kernels_association_and_fails_a_wrong_sil_term(kind):
    """The assertion of the GPU test (|got - truth| / condition <= max(BWD_FLOOR, 4 x float32 autograd's figure)) on the fp32 model
    of composite_bwd_kernel.  On every (S, gradient set, rgb_filter) the float32 autograd and the model stay under the floor
    itself.  With the silhouette gradient let through to the last sample the model fails the bar on every S >= 2 and every
    gradient set that holds sil -- but for the masked rays at S = 2, none of which has two live samples: the last sample's own
    d alpha is multiplied by delta expf(-delta dens) = 0 and a masked one takes no gradient, so the wrong term changes nothing
    there, and the test says so.  A set without sil is unchanged bit for bit.  (At S = 1 the only sample is the last one and
    the same factor 0 stands in front of the wrong term: nothing is asserted.  Nor with rgb_filter on: its d sigma term w k g.rgb
    brings the weight's whole forward bound, times k of about 3, into the condition of a sample whose gradient is 1e-10 on the
    empty rays, and at S = 2 the wrong term reaches 48 of that against a floor of 63.)"""
    worst = {}
    for S in BWD_S:
        for gset, scale in [(s, 0.0) for s in GRAD_SETS] + [("all", 1.3)]:
            a, g = select(case(S, kind), True, True, True), grads_for(S, kind, gset)
            ref = cn.backward_reference(a, g, scale)
            model = backward_model(a, g, scale)
            fig = _figures(model, ref)
            for k, f in fig.items():
                worst[k] = max(worst.get(k, 0.0), f)
                assert f <= cn.BWD_FLOOR[k] and ref[k][2] <= cn.BWD_FLOOR[k], (S, kind, gset, scale, k, f, ref[k][2])
            if scale > 0:
                continue
            wrong = backward_model(a, g, scale, mutation="sil")
            if "sil" not in GRAD_SETS[gset]:
                assert all(np.array_equal(wrong[k], model[k]) for k in fig), (S, kind, gset)
                continue
            caught = any(f > ref[k][3] for k, f in _figures(wrong, ref).items())
            live = (~alpha32(a)["masked"]).sum(-1)
            if S >= 2:
                assert caught == bool((live >= 2).any()), (S, kind, gset, scale)
                assert (live >= 2).any() or (kind, S) == ("masked", 2)
    print(f"composite bwd model {kind}: worst |model - truth| / condition: " + ", ".join(f"d_{k} {v:.2f}" for k, v in worst.items()))
