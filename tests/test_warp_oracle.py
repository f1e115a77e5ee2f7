"""CPU: the cases tests/test_gpu_warp.py runs, built and vetted here, and the float64 closed form of tests/warp_numpy.py pinned to
float64 torch autograd through oracle/torch_ref.py.

closed form   warp() / warp_bwd() against float64 autograd through warp_numpy.torch_warp (oracle/torch_ref.skinning's operations
              from prepared bones on, then oracle/torch_ref.dqs): forward and every gradient, every case and gradient set, 1e-12
              of the element's condition.  The whole chain bones, rts -> bone_transform -> bone_prep -> skinning -> dqs of
              dq_inverse(rts) against oracle/torch_ref's own functions, leaf gradients included (d_prep and d_q carried back
              through bone_prep_bwd, bone_transform_bwd and dq_inverse_bwd), 1e-12 of the condition carried the same way.
generator     deterministic (moda_amd.synth); |bl[:4]| >= 0.1 everywhere, |p.w| >= 1e-3 for every bone_transform orientation, both
              signs in every bone_transform case with B >= 7, nothing excluded.  "saturated": skin_aux[0] = 3 and bone centres
              spread three times as wide: one weight exactly 1.0 in fp32 on at least a quarter of the samples, several exactly 0.
mutants       six ways the kernels could be wrong, applied to the float64 reference's own outputs: each is rejected by the bar.
figures       float32 autograd's worst figure per (case kind, output), printed (-s): the yardstick of the GPU test."""
import functools

import numpy as np
import pytest
import torch

import warp_numpy as wn
from moda_amd import synth
from oracle import torch_ref as tr

B_LIST = (1, 7, 25, 32, 33, 36, 48, 49, 64, 65)
NS_LIST = ((1, 1), (1, 3), (5, 8), (5, 9), (3, 21), (3, 85), (4, 64), (1, 257), (9, 70), (2, 300))
SHAPES = tuple(sorted({(B, N, S) for B in B_LIST for N, S in ((9, 70), (1, 257))} | {(B, N, S) for B in (25, 33) for N, S in NS_LIST}))
GRAD_SETS = ("out", "cyc", "skin", "all", "all_noref", "all_nodskin", "all_tf")
FWD, BWD = ("out", "cyc", "skin"), ("d_pts", "d_pts_tf", "d_dskin", "d_q", "d_prep", "d_aux0", "d_ref")
SEED = 41


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def make_bones(tag, B, spread=0.1):
    """Centres ~ N(0, spread^2), orientations of any direction and length (both signs of the real part), log scales ~ 0.3 N."""
    b = np.zeros((B, 10), np.float32)
    b[:, :3] = np.float32(spread) * synth.normal(SEED, tag + "/c", (B, 3))
    b[:, 3:7] = synth.normal(SEED, tag + "/q", (B, 4))
    b[:, 7:10] = np.float32(0.3) * synth.normal(SEED, tag + "/s", (B, 3))
    return b


@functools.lru_cache(maxsize=None)
def case(B, N, S, per_ray, kind="plain"):
    """Every input and upstream gradient of one case, float32."""
    tag = f"warp/{kind}/{B}/{N}/{S}/{int(per_ray)}"
    sat = kind == "saturated"
    rts = synth.frame_dual_quats(SEED, tag + "/rts", N, B).reshape(N, B, 8)
    for salt in range(16):          # the first draw whose transformed orientations all keep |p.w| >= 1e-3: the sign is fp32-safe
        bones = make_bones(f"{tag}/{salt}", B, 0.3 if sat else 0.1)
        if np.abs(wn.orient_real(bones, rts)).min() >= 1e-3:
            break
    if per_ray:
        bones_t = f32(wn.bone_transform(bones, rts))
        prep, q = f32(wn.bone_prep(bones_t)), f32(wn.dq_inverse(rts))
    else:
        prep, q = f32(wn.bone_prep(bones[None])), rts
    nrm = lambda name, shape, k=1.0: f32(np.float32(k) * synth.normal(SEED, tag + name, shape))
    # plain cases: G = -1000 e^-1 and points ~ 0.1 N keep the logits' absolute terms under about 2e3, where float64's own 2^-53
    # of a logit still lies under the 1e-12 the closed form is pinned at (d_q: sum_s skin_b dbl carries the weights' error)
    pts = nrm("/x", (N, S, 3), 0.1)
    return dict(B=B, N=N, S=S, per_ray=per_ray, kind=kind, bones=bones, rts=rts, prep=prep, q=q, pts=pts,
                pts_tf=f32(pts + nrm("/tf", (N, S, 3), 0.02)), dskin=nrm("/ds", (N, S, B)),
                skin_aux=np.asarray([3.0 if sat else -1.0, 10], np.float32), cyc_ref=nrm("/ref", (N, S, 3), 0.1),
                g_out=nrm("/go", (N, S, 3)), g_cyc=nrm("/gc", (N, S)), g_skin=nrm("/gs", (N, S, B)))


def select(c, gset):
    """-> (inputs, upstream gradients) of one gradient set."""
    a = {k: c[k] for k in ("prep", "q", "pts", "dskin", "skin_aux", "cyc_ref")}
    a["pts_tf"] = c["pts_tf"] if gset == "all_tf" else None
    if gset == "all_noref":
        a["cyc_ref"] = None
    if gset == "all_nodskin":
        a["dskin"] = None
    every = gset.startswith("all")
    g = {"out": c["g_out"] if every or gset == "out" else None,
         "cyc": c["g_cyc"] if (every or gset == "cyc") and a["cyc_ref"] is not None else None,
         "skin": c["g_skin"] if every or gset == "skin" else None}
    return a, g


def np_forward(c, a):
    return wn.warp(a["prep"], c["per_ray"], a["q"], a["pts"], a["pts_tf"], a["dskin"], a["skin_aux"], a["cyc_ref"])


def np_backward(c, a, g, **kw):
    return wn.warp_bwd(a["prep"], c["per_ray"], a["q"], a["pts"], a["pts_tf"], a["dskin"], a["skin_aux"], a["cyc_ref"], g["out"],
                       g["cyc"], g["skin"], **kw)


def worst(got, ref):
    """The worst figure of `got` (None or absent: zeros) against ref = (truth, condition)."""
    truth, cond = ref
    return float(wn.ratio(np.zeros_like(truth) if got is None else got, truth, cond).max())


@functools.lru_cache(maxsize=None)
def reference(B, N, S, per_ray, gset, kind="plain"):
    """-> dict output -> (truth, condition, of, bar), forward outputs and gradients of one (case, gradient set): of the worst
    figure of float32 torch autograd, bar = max(FLOOR, 4 of).  None where the output does not exist (or, for d_dskin, where no
    dskin was given: the kernel's logit gradient is then not returned)."""
    c = case(B, N, S, per_ray, kind)
    a, g = select(c, gset)
    fw, bw = np_forward(c, a), np_backward(c, a, g)
    f32_fw, f32_bw = wn.torch_warp_grads(a, g, torch.float32)
    fl = wn.floors(B, S, N, shared=not per_ray)
    out = {}
    for k in FWD + BWD:
        r = fw[k] if k in FWD else bw[k]
        if r is None or (k == "d_dskin" and a["dskin"] is None) or (k == "d_ref" and g["cyc"] is None):
            out[k] = None
            continue
        of = worst((f32_fw if k in FWD else f32_bw)[k], r)
        out[k] = (r[0], r[1], of, max(fl[k], 4.0 * of))
    return out


# ------------------------------------------------------------------------------------------------------ closed form against autograd
def rel(got, truth, cond):
    d = np.abs(np.zeros_like(truth) if got is None else got - truth)
    return float(np.where(cond > 0, d / np.where(cond > 0, cond, 1.0), np.where(d == 0, 0.0, np.inf)).max())


@pytest.mark.parametrize("B,N,S", SHAPES)
def test_closed_form_matches_float64_autograd(B, N, S):
    kinds = ("plain", "saturated") if (N, S) == (9, 70) and B in (7, 33) else ("plain",)
    for kind in kinds:
        for per_ray in (True, False):
            c = case(B, N, S, per_ray, kind)
            for gset in GRAD_SETS:
                a, g = select(c, gset)
                fw, bw = np_forward(c, a), np_backward(c, a, g)
                t_fw, t_bw = wn.torch_warp_grads(a, g, torch.float64)
                for k in FWD:
                    assert (fw[k] is None) == (t_fw[k] is None), (kind, per_ray, gset, k)
                    if fw[k] is not None:
                        assert rel(t_fw[k], *fw[k]) <= 1e-12, (kind, per_ray, gset, k, rel(t_fw[k], *fw[k]))
                for k in BWD:
                    if bw[k] is None:
                        assert t_bw[k] is None, (kind, per_ray, gset, k)
                    elif not (k == "d_dskin" and a["dskin"] is None):
                        assert rel(t_bw[k], *bw[k]) <= 1e-12, (kind, per_ray, gset, k, rel(t_bw[k], *bw[k]))


@pytest.mark.parametrize("B,N,S", [(7, 5, 9), (33, 3, 21), (65, 2, 11)])
def test_chain_matches_torch_ref_autograd(B, N, S):
    """bones, rts -> out, cyc, skin through oracle/torch_ref's own functions, float64, against the numpy chain."""
    c = case(B, N, S, True)
    T = lambda v: torch.from_numpy(np.array(v)).double().requires_grad_(True)
    bones, rts, pts, dskin, aux, ref = (T(c[k]) for k in ("bones", "rts", "pts", "dskin", "skin_aux", "cyc_ref"))
    bt = tr.bone_transform(bones, rts)
    skin = tr.skinning(bt, pts, dskin, aux)
    out = tr.dqs(tr.dq_inverse(rts), skin, pts)
    cyc = (ref - out).norm(dim=-1)
    G = lambda k: torch.from_numpy(c[k]).double()
    ((out * G("g_out")).sum() + (cyc * G("g_cyc")).sum() + (skin * G("g_skin")).sum()).backward()

    n_bt = wn.bone_transform(c["bones"], c["rts"])
    n_prep, n_q = wn.bone_prep(n_bt), wn.dq_inverse(c["rts"])
    assert rel(bt.detach().numpy(), n_bt, np.abs(n_bt) + 1.0) <= 1e-12
    fw = wn.warp(n_prep, True, n_q, c["pts"], None, c["dskin"], c["skin_aux"], c["cyc_ref"])
    for k, t in (("out", out), ("cyc", cyc), ("skin", skin)):
        assert rel(t.detach().numpy(), *fw[k]) <= 1e-12, k
    bw = wn.warp_bwd(n_prep, True, n_q, c["pts"], None, c["dskin"], c["skin_aux"], c["cyc_ref"], c["g_out"], c["g_cyc"], c["g_skin"])
    for k, t in (("d_pts", pts), ("d_dskin", dskin), ("d_ref", ref)):
        assert rel(t.grad.numpy(), *bw[k]) <= 1e-12, k
    assert rel(aux.grad.numpy()[:1], *bw["d_aux0"]) <= 1e-12
    # d_prep and d_q back to the leaves, values and conditions alike
    d_bt, c_bt = wn.bone_prep_bwd(n_bt, bw["d_prep"][0])
    c_bt = wn.bone_prep_bwd(n_bt, bw["d_prep"][1])[1] + c_bt * 0
    tb, tbc = wn.bone_transform_bwd(c["bones"], c["rts"], d_bt), wn.bone_transform_bwd(c["bones"], c["rts"], c_bt)
    di, dic = wn.dq_inverse_bwd(c["rts"], bw["d_q"][0]), wn.dq_inverse_bwd(c["rts"], bw["d_q"][1])
    assert rel(bones.grad.numpy(), tb["d_bones"][0], tbc["d_bones"][1]) <= 1e-12
    assert rel(rts.grad.numpy(), tb["d_rts"][0] + di[0], tbc["d_rts"][1] + dic[1]) <= 1e-12


# --------------------------------------------------------------------------------------------------------------------- prep kernels
BONE_PREP_N = (1, 255, 256, 257)
BONE_TRANSFORM_NB = ((1, 1), (5, 51), (8, 32), (1, 257), (9, 36))
DQ_INVERSE_N = (1, 257)


@functools.lru_cache(maxsize=None)
def prep_case(which, *shape):
    """-> (inputs, g, {output: (truth, condition, of, bar)}) of one prep-kernel case; of from float32 torch autograd."""
    tag = f"prep/{which}/{shape}"
    T = lambda v, dt: torch.from_numpy(np.array(v)).to(dt).requires_grad_(True)
    if which == "bone_prep":
        (n,) = shape
        ins = (make_bones(tag, n),)
        g = f32(synth.normal(SEED, tag + "/g", (n, 16)))
        ref = {"d_bones": wn.bone_prep_bwd(ins[0], g)}
        fn, floor = (lambda b: wn.torch_bone_prep(b)), {"d_bones": wn.PREP_FLOOR["bone_prep"]}
        names = ("d_bones",)
    elif which == "bone_transform":
        N, B = shape
        ins = (make_bones(tag, B), synth.frame_dual_quats(SEED, tag + "/rts", N, B, rot=0.5).reshape(N, B, 8))
        g = f32(synth.normal(SEED, tag + "/g", (N, B, 10)))
        r = wn.bone_transform_bwd(ins[0], ins[1], g)
        ref = {"d_bones": r["d_bones"], "d_rts": r["d_rts"]}
        fn = tr.bone_transform
        floor = {"d_bones": wn.PREP_FLOOR["bone_transform_bones"] + N, "d_rts": wn.PREP_FLOOR["bone_transform_rts"]}
        names = ("d_bones", "d_rts")
    else:
        (n,) = shape
        dq = synth.frame_dual_quats(SEED, tag + "/dq", n, 1, rot=0.5).reshape(n, 8)
        ins = (f32(dq * (np.float32(0.5) + synth.uniform(SEED, tag + "/len", (n, 1)))),)      # |real part| in [0.5, 1.5)
        g = f32(synth.normal(SEED, tag + "/g", (n, 8)))
        ref = {"d_dq": wn.dq_inverse_bwd(ins[0], g)}
        fn, floor, names = tr.dq_inverse, {"d_dq": wn.PREP_FLOOR["dq_inverse"]}, ("d_dq",)
    grads = {}
    for dt in (torch.float64, torch.float32):
        leaves = [T(v, dt) for v in ins]
        (fn(*leaves) * torch.from_numpy(g).to(dt)).sum().backward()
        grads[dt] = {k: l.grad.double().numpy() for k, l in zip(names, leaves)}
    out = {}
    for k in names:
        of = worst(grads[torch.float32][k], ref[k])
        out[k] = ref[k] + (of, max(floor[k], 4.0 * of))
    return ins, g, out, grads[torch.float64]


def test_prep_closed_forms_match_float64_autograd():
    cases = [("bone_prep", n) for n in BONE_PREP_N] + [("bone_transform",) + nb for nb in BONE_TRANSFORM_NB] + \
            [("dq_inverse", n) for n in DQ_INVERSE_N]
    for cs in cases:
        ins, g, ref, g64 = prep_case(*cs)
        for k, (truth, cond, of, bar) in ref.items():
            assert rel(g64[k], truth, cond) <= 1e-12, (cs, k, rel(g64[k], truth, cond))
            print(f"{cs} {k}: float32 autograd {of:.2f}, bar {bar:.1f}")
    # forward: bone_prep and dq_inverse
    b = make_bones("prep/fwd", 37)
    assert np.abs(wn.bone_prep(b) - wn.torch_bone_prep(torch.from_numpy(b).double()).numpy()).max() <= 1e-13
    dq = prep_case("dq_inverse", 257)[0][0]
    assert np.abs(wn.dq_inverse(dq) - tr.dq_inverse(torch.from_numpy(dq).double()).numpy()).max() <= 1e-13


# ------------------------------------------------------------------------------------------------------------------------ generator
def test_generator_conditions_hold_on_every_case():
    for B, N, S in SHAPES:
        for per_ray in (True, False):
            c = case(B, N, S, per_ray)
            for gset in ("all", "all_nodskin"):
                bl = np_forward(c, select(c, gset)[0])["bl"]
                assert np.sqrt((bl[..., :4] ** 2).sum(-1)).min() >= 0.1, (B, N, S, per_ray, gset)
            if per_ray:
                w = wn.orient_real(c["bones"], c["rts"])
                assert np.abs(w).min() >= 1e-3, (B, N, S, np.abs(w).min())
    for N, B in BONE_TRANSFORM_NB:
        (bones, rts), _, _, _ = prep_case("bone_transform", N, B)
        w = wn.orient_real(bones, rts)
        assert np.abs(w).min() >= 1e-3, (N, B, np.abs(w).min())
        if B >= 7:
            assert (w < 0).any() and (w > 0).any(), (N, B)
    for B, N, S in SHAPES:
        if B >= 7:
            w = wn.orient_real(case(B, N, S, True)["bones"], case(B, N, S, True)["rts"])
            assert (w < 0).any() and (w > 0).any(), (B, N, S)


SATURATED = ((7, 9, 70), (33, 9, 70))


def test_saturated_cases_saturate_in_fp32():
    for B, N, S in SATURATED:
        for per_ray in (True, False):
            c = case(B, N, S, per_ray, "saturated")
            a, g = select(c, "all")
            skin32 = wn.torch_warp_grads(a, g, torch.float32)[0]["skin"]
            one = (skin32 == 1.0).any(-1)
            assert one.mean() >= 0.25, (B, per_ray, one.mean())
            assert ((skin32 == 0.0).sum(-1) >= 3).all(), (B, per_ray)
            bw = np_backward(c, a, g)
            zero = bw["d_dskin"][1] == 0                       # a weight that is 0 in float64 too: the element must be exactly 0
            assert zero.mean() > 0.25 and (bw["d_dskin"][0][zero] == 0).all(), (B, per_ray, zero.mean())
            for k, r in reference(B, N, S, per_ray, "all", "saturated").items():
                if r is not None:
                    assert np.isfinite(r[0]).all() and np.isfinite(r[2]), (B, per_ray, k)


# -------------------------------------------------------------------------------------------------------------------------- mutants
def test_mutants_are_rejected_by_the_bar():
    """Case B = 36, (N, S) = (9, 70), all three upstream gradients.  Each mutant is the float64 reference's own output with one
    thing a kernel could get wrong; its worst figure must be above the bar."""
    B, N, S = 36, 9, 70
    fails = lambda ref, mutant: worst(mutant, ref[:2]) > ref[3]
    for per_ray in (True, False):
        c = case(B, N, S, per_ray)
        a, g = select(c, "all")
        ref = reference(B, N, S, per_ray, "all")
        bw = np_backward(c, a, g)
        for k in BWD:                                                             # (the unmutated outputs pass)
            if ref[k] is not None:
                assert not fails(ref[k], bw[k][0]), k
        for k in ("d_q", "d_prep"):                                               # the reduce kernel's second pass dropped
            m = bw[k][0].copy()
            m[:, 32:] = 0
            assert fails(ref[k], m), (per_ray, k)
        m = bw["d_aux0"][0] - bw["aux_terms"][:, 7::8].sum()                      # sample slice g = 7 missing
        assert fails(ref["d_aux0"], m), per_ray
        mb = np_backward(c, a, g, sdot_without_g_skin=True)                       # sdot without the direct gradient
        assert fails(ref["d_dskin"], mb["d_dskin"][0]) and fails(ref["d_pts"], mb["d_pts"][0]), per_ray
        m = bw["d_dskin"][0].copy()                                               # a dead lane stored onto the last live sample
        m[-1, -1] *= 2
        assert fails(ref["d_dskin"], m), per_ray
    c = case(B, N, S, True)                                                       # per-ray bones read from ray 0's prep
    a, g = select(c, "all")
    a0 = dict(a, prep=np.ascontiguousarray(np.broadcast_to(a["prep"][:1], a["prep"].shape)))
    m = np_backward(c, a0, g)["d_prep"][0]
    assert fails(reference(B, N, S, True, "all")["d_prep"], m)
    (bones, rts), gg, ref, _ = prep_case("bone_transform", 9, 36)                 # sg forced to +1
    mut = wn.bone_transform_bwd(bones, rts, gg, force_sg=1.0)
    assert fails(ref["d_bones"], mut["d_bones"][0]) and fails(ref["d_rts"], mut["d_rts"][0])


# -------------------------------------------------------------------------------------------------------------------------- figures
def test_float32_autograd_figures():
    """Prints float32 autograd's worst figure per (case kind, output) over every shape and gradient set, with the floors'
    range; asserts only that every figure is finite (nothing is excluded, so a non-finite one would void the bar)."""
    table = {}
    runs = [(B, N, S, "plain") for B, N, S in SHAPES] + [(B, N, S, "saturated") for B, N, S in SATURATED]
    for B, N, S, kind in runs:
        for per_ray in (True, False):
            for gset in GRAD_SETS:
                for k, r in reference(B, N, S, per_ray, gset, kind).items():
                    if r is None:
                        continue
                    assert np.isfinite(r[2]), (B, N, S, kind, per_ray, gset, k)
                    key = (kind, "per-ray" if per_ray else "shared", k)
                    table[key] = max(table.get(key, 0.0), r[2])
    for kind in ("plain", "saturated"):
        for pr in ("per-ray", "shared"):
            print(f"float32 autograd, {kind} {pr}: " + ", ".join(f"{k} {table[(kind, pr, k)]:.1f}" for k in FWD + BWD if (kind, pr, k) in table))
