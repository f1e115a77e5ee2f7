"""GPU (-m gpu): the skinning warp (autograd.WarpFn: warp_staged_kernel / warp_kernel<true, true> forward, warp_bwd_kernel<STAGE> and
warp_bwd_reduce_kernel backward) and the prep kernels behind BonePrepFn, BoneTransformFn and DqInverseFn PER ELEMENT against the
float64 closed form of tests/warp_numpy.py, on the cases tests/test_warp_oracle.py builds and vets on the CPU.  fp32; u = 2^-24.

shapes       B in {1, 7, 25, 32, 33, 36, 48, 49, 64, 65} at (N, S) = (9, 70) and (1, 257); (N, S) in {(1, 1), (1, 3), (5, 8), (5, 9),
             (3, 21), (3, 85), (4, 64), (1, 257), (9, 70), (2, 300)} at B = 25 and 33; per-ray and shared bones at each; two
             "saturated" cases (one weight exactly 1.0 in fp32 on a quarter of the samples and more).
gradient     out only / cyc only / skin only / all three / all with cyc_ref = None / all with dskin = None / all with pts_tf.
sets         prep and q are leaves: d_prep and d_q are checked themselves, not through the prep kernels.
bar          every element of out, cyc, skin, d_pts, d_pts_tf, d_dskin, d_q, d_prep, d_aux0, d_ref:
             |got - truth| / (u condition) <= max(FLOOR, 4 x the figure of float32 torch autograd on the same case, computed at run
             time on the CPU).  condition and FLOOR: warp_numpy's docstring.  The factor 4 covers the kernel's association (the
             8-slice tree, fma chains over the bones) against autograd's.  A condition of 0 is an exact statement.
identities   bit for bit for d_pts, d_dskin, d_q, d_prep (d_aux0: atomics, held to its bar): two runs; g_skin as a contiguous view
             4 bytes past a 16-byte boundary against the aligned one; dskin = None against a zero dskin (the dskin gradient is
             then None).
routes       staged / unstaged backward on either side of B = 32 | 33 (with g_skin) and B = 64 | 65 (without): both sides within
             their bars, and the worst figure per output on one side within 4 x the other's (figures under 1, a single rounding,
             count as 1).
cycle        cyc_ref = the forward's own out on every fifth sample: d_ref exactly 0 there, d_pts there bit-equal to the run whose
             g_cyc is 0 on those samples, everything finite.
prep         bone_prep backward n in {1, 255, 256, 257}; bone_transform backward N B in {1, 255, 256, 257, 9 x 36};
             dq_inverse backward n in {1, 257}: the same bar with warp_numpy.PREP_FLOOR.

Every test prints (-s) the worst figure per output of the kernel beside float32 autograd's on the same case.
Float32 autograd on the CPU, worst over every shape and gradient set (tests/test_warp_oracle.py::test_float32_autograd_figures; it
moves with the CPU it runs on, by a factor of 2.5 on single cases):
  plain per-ray      out 3.7, cyc 1.0, skin 6.6, d_pts 46.1, d_pts_tf 33.1, d_dskin 409.7, d_q 286.9, d_prep 159.9, d_aux0 1.9, d_ref 21.6
  plain shared       out 3.3, cyc 1.1, skin 6.4, d_pts 31.0, d_pts_tf 50.3, d_dskin 447.7, d_q 148.3, d_prep 137.2, d_aux0 0.7, d_ref 12.9
  saturated per-ray  out 3.3, cyc 1.1, skin 2.4, d_pts 441.1, d_pts_tf 175.4, d_dskin 6974.1, d_q 6580.5, d_prep 4023.3, d_aux0 0.0, d_ref 378.4
  saturated shared   out 3.4, cyc 1.0, skin 1.8, d_pts 385.5, d_pts_tf 892.1, d_dskin 4498.8, d_q 1692.8, d_prep 159.3, d_aux0 0.0, d_ref 347.9
(the gradients' conditions hold the terms' magnitudes, not what the saved fp32 weights are off by: a logit of 1e3 is off by 1e3 u,
and kernel and autograd alike carry that into every gradient.)
Measured on an MI355X, worst over the shapes and gradient sets, kernel / float32 autograd:
  plain per-ray      out 4.1 / 3.7, cyc 0.9 / 1.0, skin 5.4 / 6.6, d_pts 31.9 / 46.1, d_pts_tf 25.8 / 33.1, d_dskin 377.7 / 409.7,
                     d_q 123.4 / 286.9, d_prep 119.9 / 159.9, d_aux0 1.9 / 1.9, d_ref 13.9 / 22.3
  plain shared       out 4.5 / 3.5, cyc 1.1 / 1.1, skin 6.0 / 6.4, d_pts 16.1 / 31.0, d_pts_tf 20.8 / 49.3, d_dskin 378.3 / 447.7,
                     d_q 161.4 / 148.3, d_prep 117.1 / 137.2, d_aux0 1.4 / 0.7, d_ref 13.6 / 12.3
  saturated per-ray  out 2.8 / 3.3, cyc 1.1 / 1.1, skin 2.0 / 2.4, d_pts 451.5 / 441.1, d_pts_tf 156.9 / 175.0, d_dskin 9896.8 / 6974.1,
                     d_q 3283.0 / 6581.4, d_prep 1517.6 / 4023.3, d_aux0 0.0 / 0.0, d_ref 337.2 / 378.4
  saturated shared   out 2.8 / 3.4, cyc 1.0 / 1.0, skin 2.2 / 1.8, d_pts 259.7 / 385.5, d_pts_tf 357.7 / 892.1, d_dskin 7116.1 / 4498.8,
                     d_q 2313.8 / 1692.8, d_prep 160.4 / 159.3, d_aux0 0.0 / 0.0, d_ref 67.1 / 347.9
  bone_prep d_bones 2.5 / 3.1; bone_transform d_bones 8.5 / 7.3, d_rts 2.4 / 3.5; dq_inverse d_dq 4.2 / 5.7
The zero-length cycle test found WarpFn returning a unit vector of rounding noise times g_cyc as d_ref (and carrying it into every
other gradient) where the forward's cyc is exactly 0: the backward kernel recomputes out an ulp off the forward's.  WarpFn.backward
now drops g_cyc on those samples."""
import numpy as np
import pytest
import torch

import warp_numpy as wn
import test_warp_oracle as C

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import moda_amd
    from moda_amd import autograd as A
    from gpu_helpers import DEV

BIT_EXACT = ("d_pts", "d_pts_tf", "d_dskin", "d_q", "d_prep")


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


def run(a, g, g_skin_off=False):
    """WarpFn forward + backward with the upstream gradients handed to it as they are -> {output or gradient: numpy or None}."""
    leaf = {k: (None if a[k] is None else T(a[k]).requires_grad_(True)) for k in wn.WARP_LEAVES}
    out, cyc, skin = A.WarpFn.apply(leaf["prep"], leaf["q"], leaf["pts"], leaf["dskin"], leaf["skin_aux"], leaf["cyc_ref"], leaf["pts_tf"])
    res = {"out": np_(out), "cyc": np_(cyc), "skin": np_(skin)}
    outs, gos = [], []
    for o, k in ((out, "out"), (cyc, "cyc"), (skin, "skin")):
        if o is not None and g.get(k) is not None:
            outs.append(o)
            gos.append(off_by_4_bytes(g[k]) if (k == "skin" and g_skin_off) else T(g[k]))
    names = [k for k in wn.WARP_LEAVES if leaf[k] is not None]
    grads = dict(zip(names, torch.autograd.grad(outs, [leaf[k] for k in names], gos, allow_unused=True)))
    gr = lambda k: np_(grads.get(k))
    res.update({"d_prep": gr("prep"), "d_q": gr("q"), "d_pts": gr("pts"), "d_pts_tf": gr("pts_tf"), "d_dskin": gr("dskin"),
                "d_aux0": None if gr("skin_aux") is None else gr("skin_aux")[:1], "d_ref": gr("cyc_ref")})
    if res["d_aux0"] is not None:
        assert gr("skin_aux")[1] == 0, "skin_aux[1] has no gradient"
    return res


def check(got, ref, tag, table):
    """Every output of one run against its bar; the worst figures go into `table` {output: [kernel, float32 autograd]}."""
    figs = {}
    for k, r in ref.items():
        if r is None:
            if k == "d_dskin":
                assert got[k] is None, (tag, k)
            continue
        truth, cond, of, bar = r
        gk = np.zeros_like(truth) if got[k] is None else got[k]
        assert gk.shape == truth.shape and np.isfinite(gk).all(), (tag, k)
        fig = wn.ratio(gk, truth, cond)
        kf = float(fig.max())
        w = table.setdefault(k, [0.0, 0.0])
        w[0], w[1] = max(w[0], kf), max(w[1], of)
        figs[k] = kf
        assert kf <= bar, (tag, k, kf, of, bar, np.unravel_index(np.argmax(fig), fig.shape))
    return figs


def show(title, table):
    print(f"{title}: kernel / torch32 " + ", ".join(f"{k} {v[0]:.1f} / {v[1]:.1f}" for k, v in table.items()))


def same_bits(x, y, tag, keys=BIT_EXACT):
    for k in keys:
        assert (x[k] is None) == (y[k] is None), (tag, k)
        if x[k] is not None:
            assert np.array_equal(bits(x[k]), bits(y[k])), (tag, k)


def one_case(B, N, S, kind, table_of):
    for per_ray in (True, False):
        c = C.case(B, N, S, per_ray, kind)
        table = table_of(per_ray)
        for gset in C.GRAD_SETS:
            a, g = C.select(c, gset)
            tag = (B, N, S, kind, per_ray, gset)
            ref = C.reference(B, N, S, per_ray, gset, kind)
            got = run(a, g)
            check(got, ref, tag, table)
            if gset == "all":
                same_bits(run(a, g), got, tag + ("two runs",))
                off = run(a, g, g_skin_off=True)
                same_bits(off, got, tag + ("g_skin 4 bytes off",))
                check(off, ref, tag + ("g_skin 4 bytes off",), table)
            if gset == "all_nodskin":
                assert got["d_dskin"] is None, tag
                zero = run(dict(a, dskin=np.zeros((N, S, B), np.float32)), g)
                same_bits(zero, got, tag + ("zero dskin",), ("d_pts", "d_q", "d_prep", "d_ref"))
                same_bits(zero, got, tag + ("zero dskin",), ("out", "cyc", "skin"))
            if kind == "saturated" and gset == "all":
                zero = ref["d_dskin"][1] == 0
                assert zero.any() and (got["d_dskin"][zero] == 0).all(), tag


@pytest.mark.parametrize("B,N,S", C.SHAPES)
def test_warp_per_element_against_float64(B, N, S):
    tables = {}
    one_case(B, N, S, "plain", lambda pr: tables.setdefault(pr, {}))
    for pr, t in tables.items():
        show(f"warp B={B} N={N} S={S} {'per-ray' if pr else 'shared'}", t)


@pytest.mark.parametrize("B,N,S", C.SATURATED)
def test_saturated_weights_stay_finite_and_within_the_bar(B, N, S):
    tables = {}
    one_case(B, N, S, "saturated", lambda pr: tables.setdefault(pr, {}))
    for pr, t in tables.items():
        show(f"warp saturated B={B} N={N} S={S} {'per-ray' if pr else 'shared'}", t)


@pytest.mark.parametrize("lo,hi,gset", [(32, 33, "all"), (64, 65, "out")])
def test_staged_and_unstaged_routes_agree(lo, hi, gset):
    """The tile is (g_skin ? 2 : 1) x 256 x B x 4 bytes against 64 KiB: staged up to B = 32 with g_skin and 64 without."""
    N, S = 9, 70
    for per_ray in (True, False):
        figs = []
        for B in (lo, hi):
            c = C.case(B, N, S, per_ray)
            a, g = C.select(c, gset)
            figs.append(check(run(a, g), C.reference(B, N, S, per_ray, gset), (B, per_ray, gset), {}))
        for k in figs[0]:
            x, y = max(figs[0][k], 1.0), max(figs[1][k], 1.0)
            print(f"routes {gset} {'per-ray' if per_ray else 'shared'} {k}: B={lo} {figs[0][k]:.1f}, B={hi} {figs[1][k]:.1f}")
            assert max(x, y) <= 4.0 * min(x, y), (per_ray, k, figs[0][k], figs[1][k])


@pytest.mark.parametrize("B,N,S", [(25, 9, 70), (33, 2, 300)])
def test_zero_length_cycle_residual(B, N, S):
    for per_ray in (True, False):
        c = C.case(B, N, S, per_ray)
        a, g = C.select(c, "all")
        fwd = run(a, g)["out"]
        hit = (np.arange(N * S) % 5 == 0).reshape(N, S)
        ref = a["cyc_ref"].copy()
        ref[hit] = fwd[hit]
        a = dict(a, cyc_ref=ref)
        got = run(a, g)
        assert (got["cyc"][hit] == 0).all(), "the forward reproduces its own out"
        assert (got["d_ref"][hit] == 0).all()
        for k, v in got.items():
            assert v is None or np.isfinite(v).all(), (per_ray, k)
        g0 = dict(g, cyc=np.where(hit, np.float32(0), g["cyc"]))
        base = run(a, g0)
        assert np.array_equal(bits(got["d_pts"][hit]), bits(base["d_pts"][hit])), per_ray
        same_bits(base, got, (B, per_ray, "cycle"), ("d_dskin", "d_q", "d_prep"))
        bw = C.np_backward(c, a, g)                     # and the whole run against float64, d_ref = 0 where |ref - out| == 0
        t_ref = bw["d_ref"][0][~hit]
        fig = wn.ratio(got["d_ref"][~hit], t_ref, bw["d_ref"][1][~hit])
        of = C.reference(B, N, S, per_ray, "all")["d_ref"]
        assert fig.max() <= of[3], (per_ray, fig.max(), of[3])


# ----------------------------------------------------------------------------------------------------------------------- prep kernels
def _prep_check(which, shape, fn, table):
    ins, g, ref, _ = C.prep_case(which, *shape)
    leaves = [T(v).requires_grad_(True) for v in ins]
    grads = torch.autograd.grad([fn(*leaves)], leaves, [T(g)])
    for (k, (truth, cond, of, bar)), gd in zip(ref.items(), grads):
        gk = np_(gd)
        assert gk.shape == truth.shape and np.isfinite(gk).all(), (which, shape, k)
        fig = wn.ratio(gk, truth, cond)
        w = table.setdefault(k, [0.0, 0.0])
        w[0], w[1] = max(w[0], float(fig.max())), max(w[1], of)
        assert fig.max() <= bar, (which, shape, k, float(fig.max()), of, bar, np.unravel_index(np.argmax(fig), fig.shape))


def test_bone_prep_backward_per_element():
    table = {}
    for n in C.BONE_PREP_N:
        _prep_check("bone_prep", (n,), lambda b: A.bone_prep(b), table)
        b = C.prep_case("bone_prep", n)[0][0]
        fwd = np_(A.bone_prep(T(b)))
        assert np.abs(fwd - wn.bone_prep(b)).max() <= 16 * wn.U * 4 and (fwd[:, 15] == 0).all()     # entries of size <= 4
    show("bone_prep", table)


def test_bone_transform_backward_per_element():
    table = {}
    for nb in C.BONE_TRANSFORM_NB:
        _prep_check("bone_transform", nb, lambda b, r: A.bone_transform(b, r), table)
    show("bone_transform", table)


def test_dq_inverse_backward_per_element():
    table = {}
    for n in C.DQ_INVERSE_N:
        _prep_check("dq_inverse", (n,), lambda q: A.dq_inverse(q), table)
    show("dq_inverse", table)
