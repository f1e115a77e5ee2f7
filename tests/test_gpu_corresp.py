"""GPU (-m gpu): the correspondence heads and per-ray sums of the training route through their autograd Functions -- ProjectFn
(project_fwd_kernel, project_bwd_kernel), FlowRenderFn (flow_render_kernel, both directions), PtsExpFn (pts_exp_kernel, both),
PointsFn (sample_rays4_kernel<false> / points_kernel, points_bwd_kernel), ExpandRowsFn (segsum_kernel through moda_segsum_f32) and
VisPairLossFn (logsig_loss_kernel, two launches each way) -- PER ELEMENT against the float64 reference of tests/corresp_numpy.py, on
the cases tests/test_corresp_oracle.py builds and vets on the CPU.  fp32; u = 2^-24.

per element  every forward output and every gradient (d_xyz, d_rtk; d_w, d_proj; d_w_pts, d_pts; d_o, d_d, d_z; dx_rows; dx_vis):
             |got - truth| / (u condition) <= max(FLOOR, 4 x the float32 reference's figure on the same case, computed at run time).
             truth = the float64 closed form (pinned to float64 autograd on the CPU); condition = that closed form with every term in
             absolute value, divisors included; FLOOR = the relative roundings one term gathers in the kernel, counted per output in
             corresp_numpy's docstring; the float32 reference is numpy fp32 (forward) and torch fp32 autograd through the
             restatement (backward); the factor 4 is test_gpu_composite.py's allowance for butterfly versus sequential association.
             S in {1, 2, 63, 64, 65, 128, 129, 200} (a second, third and fourth lane trip, whole and partial), N in {9, 5, 1} (the
             last workgroup is never full).  Nothing is excluded: a condition of 0 is an exact statement, and every value is finite.
exact, flow  `valid` equals the reference's count test; an all-invalid ray has flo == 0, valid == 0 and d_w, d_proj all zero;
             d_w and d_proj are exactly 0 at every invalid sample; d_proj[..., 2] is exactly 0; with NaN / Inf / -Inf in w, u, v at
             samples invalid by depth every output and gradient is finite and bit for bit the run on benign values there.
exact, proj  d_rtk[:, (13, 15, 18, 19, 20)] is exactly 0; with d_rtk and d_xyz pre-filled with NaN (moda_project_bwd called
             directly) every element is written, bit for bit what the Function returns.
routes       PointsFn's forward at S % 4 == 0 from an aligned z (four samples per thread, 16-byte accesses) and from the same data
             4 bytes off (the scalar kernel): bit for bit.  VisPairLossFn with n_neg odd against moda_logsig_loss on separately
             allocated halves: dx bit for bit, and the loss too where each half is one workgroup (more than one: their atomic adds
             onto the sum come in any order; the loss is then held to its bar).  ExpandRowsFn's backward at R = 65537 frames (two
             launches: 65535 + 2 rows of grid.y), k = 2, C = 3, against moda_segsum_f32 on the two pieces: bit for bit, and
             against float64.
repeatable   two runs of every backward give bit-identical gradients.  Read from the code: project_bwd, flow_render, pts_exp,
             segsum and logsig_loss write their gradients with plain stores, one thread per element.  points_bwd_kernel adds with
             atomicAdd, but each d_z element from the one lane that owns sample (n, s) and each d_o / d_d element from lane 0 of
             ray n's wave, once, onto buffers PointsFn.backward takes from the zero pool (a slice is never handed out twice): no
             element receives more than one atomic add onto zero, so the result is that one term, exactly.

tests/test_corresp_oracle.py holds fp32 numpy models of the kernels to the same bars on the CPU: they stay under 4.6 (d_w of flow
mixed; float32 autograd 3.6 there), far below every floor, and fail with lanes that stop after one trip, a dropped `common` in
either backward, den for den * den in dZ and `ninv` read from lane 0 (the cases and outputs that catch each are listed there).

Every test prints the figure per (kind, S, N, output) of the kernel beside the float32 reference's, and the worst per kind (run with
-s).  The figures are in units of u condition, the floors 2 ... 38 are worst cases of a linear count: both the kernels and the
float32 reference sit at a few units.  No test here exposed a kernel or wrapper bug.
Measured on an MI355X, worst over S and N, kernel / float32 reference:
  project front         proj 2.75 / 2.75, d_xyz 3.33 / 3.58, d_rtk 2.74 / 6.92
  project grazing       proj 3.10 / 3.10, d_xyz 2.74 / 3.30, d_rtk 0.81 / 0.81
  flow valid            flo 2.84 / 2.97, d_w 2.01 / 2.77, d_proj 3.77 / 3.54
  flow mixed            flo 2.75 / 2.37, d_w 4.56 / 3.32, d_proj 3.77 / 3.96
  flow edge             flo 2.56 / 4.24, d_w 2.62 / 3.30, d_proj 3.48 / 3.40
  flow all_invalid      flo 1.31 / 3.64, d_w 1.81 / 2.62, d_proj 2.10 / 3.10      (the last ray, the valid one)
  flow single_valid     flo 3.02 / 3.02, d_w 1.10 / 1.19, d_proj 2.47 / 1.95
  flow poison           flo 3.06 / 2.33, d_w 3.37 / 3.56, d_proj 3.22 / 3.21
  pts_exp soft          pts_exp 2.24 / 3.91, d_w_pts 1.69 / 3.26, d_pts 2.93 / 3.49
  pts_exp onehot        pts_exp 0.02 / 0.02, d_w_pts 1.44 / 1.44, d_pts 0.02 / 0.02
  pts_exp zero          pts_exp 2.45 / 1.66, d_w_pts 2.27 / 2.44, d_pts 3.30 / 2.70
  points                xyz 0.98 / 1.83, d_o 2.12 / 2.48, d_d 1.90 / 2.65, d_z 1.93 / 1.93
  rows                  rows 0.00 / 0.00 (a copy), dx_rows 1.63 / 2.06
  vis                   vis_loss 0.82 / 1.87, dx_vis 3.77 / 3.28
The whole file takes under 4 s."""
import numpy as np
import pytest
import torch

import corresp_numpy as cn
import test_corresp_oracle as C

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import moda_amd
    from moda_amd import autograd as A, _lib as L
    from gpu_helpers import DEV


def np_(t):
    return None if t is None else t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def leaf(a):
    return T(a).requires_grad_(True)


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


def run(op, c):
    """One forward and backward of sum(g * out) through the autograd Function of `op` -> {name: numpy array}."""
    g = T(c["g"])
    if op == "project":
        xyz, rtk = leaf(c["xyz"]), leaf(c["rtk"])
        out = A.ProjectFn.apply(xyz, rtk)
        (out * g).sum().backward()
        return {"proj": np_(out), "d_xyz": np_(xyz.grad), "d_rtk": np_(rtk.grad)}
    if op == "flow":
        w, proj = leaf(c["w"]), leaf(c["proj"])
        flo, valid = A.FlowRenderFn.apply(w, proj, T(c["xys"]), c["img"])
        (flo * g).sum().backward()
        return {"flo": np_(flo), "valid": np_(valid), "d_w": np_(w.grad), "d_proj": np_(proj.grad)}
    if op == "pts_exp":
        w, pts = leaf(c["w"]), leaf(c["pts"])
        out = A.PtsExpFn.apply(w, pts)
        (out * g).sum().backward()
        return {"pts_exp": np_(out), "d_w_pts": np_(w.grad), "d_pts": np_(pts.grad)}
    if op == "points":
        o, d, z = leaf(c["o"]), leaf(c["d"]), leaf(c["z"])
        out = A.PointsFn.apply(o, d, z)
        (out * g).sum().backward()
        return {"xyz": np_(out), "d_o": np_(o.grad), "d_d": np_(d.grad), "d_z": np_(z.grad)}
    if op == "rows":
        x = leaf(c["x"])
        out = A.ExpandRowsFn.apply(x, c["k"])
        (out * g).sum().backward()
        return {"rows": np_(out), "dx_rows": np_(x.grad)}
    x = leaf(c["x"])
    out = A.VisPairLossFn.apply(x, T(c["w_pos"]), c["n_neg"])
    (out * g[0]).backward()
    return {"vis_loss": np_(out).reshape(1), "dx_vis": np_(x.grad)}


def check(op, tag, c, got, worst):
    for k, (truth, cond, of, bar) in C.reference(op, tag, c).items():
        assert got[k].dtype == np.float32 and got[k].shape == truth.shape, (tag, k)
        assert np.isfinite(got[k]).all(), (tag, k)
        fig = cn.ratio(got[k], truth, cond)
        kf = float(fig.max())
        w = worst.setdefault((tag[1], k), [0.0, 0.0])
        w[0], w[1] = max(w[0], kf), max(w[1], of)
        print(f"corresp {tag} {k}: kernel {kf:.3f} / float32 reference {of:.3f}")
        assert kf <= bar, (tag, k, kf, of, np.unravel_index(np.argmax(fig), fig.shape))


def exact_flow(tag, c, got):
    ref = cn.flow(c["w"], c["proj"], c["xys"], c["img"])
    inv = cn.invalid_mask(c["proj"], c["img"])
    assert np.array_equal(got["valid"], ref["valid"].astype(np.float32)), tag        # the reference's count test
    dead = inv.all(-1)
    assert (got["flo"][dead] == 0).all() and (got["valid"][dead] == 0).all(), tag
    assert (got["d_w"][dead] == 0).all() and (got["d_proj"][dead] == 0).all(), tag
    assert (got["d_w"][inv] == 0).all() and (got["d_proj"][inv] == 0).all(), tag
    assert (got["d_proj"][..., 2] == 0).all(), tag
    if "clean" in c:                                                                 # poison reaches nothing
        clean = run("flow", c["clean"])
        for k, v in got.items():
            assert np.isfinite(v).all() and np.array_equal(bits(v), bits(clean[k])), (tag, k, "poison")


def exact_project(tag, c, got):
    assert (got["d_rtk"][:, [13, 15, 18, 19, 20]] == 0).all(), tag
    N, S, _ = c["xyz"].shape
    x, r, g = T(c["xyz"]), T(c["rtk"]), T(c["g"])
    dx, dr = torch.full_like(x, float("nan")), torch.full_like(r, float("nan"))
    L.call("moda_project_bwd", L.ptr(x), L.ptr(r), L.ptr(g), N, S, L.ptr(dx), L.ptr(dr), L.stream())
    assert np.array_equal(bits(np_(dx)), bits(got["d_xyz"])) and np.array_equal(bits(np_(dr)), bits(got["d_rtk"])), tag


@pytest.mark.parametrize("op", list(cn.OPS))
def test_per_element_against_float64(op):
    worst = {}
    diff = tuple(cn.OPS[op][1].values())
    for tag, c in C.all_cases(op):
        got = run(op, c)
        check(op, tag, c, got, worst)
        again = run(op, c)
        for k in diff:
            assert np.array_equal(bits(again[k]), bits(got[k])), (tag, k, "two runs")
        if op == "flow":
            exact_flow(tag, c, got)
        if op == "project":
            exact_project(tag, c, got)
    for (kind, k), v in worst.items():
        print(f"corresp {op} {kind} worst over S, N: {k} {v[0]:.2f} / {v[1]:.2f}")


@pytest.mark.parametrize("S,N", [sn for sn in C.SN if sn[0] % 4 == 0])
def test_points_forward_routes_agree_bit_for_bit(S, N):
    c = C.case("points", "rays", S, N)
    o, d, z = T(c["o"]), T(c["d"]), T(c["z"])
    assert z.data_ptr() % 16 == 0
    with torch.no_grad():
        wide = A.PointsFn.apply(o, d, z)
        narrow = A.PointsFn.apply(o, d, off_by_4_bytes(c["z"]))
    assert np.array_equal(bits(np_(wide)), bits(np_(narrow)))


def _logsig(x, w, sign, scale, out=None, g=None, dx=None):
    L.call("moda_logsig_loss", L.ptr(x), L.ptr(w), x.numel(), sign, scale, L.ptr(out), L.ptr(g), L.ptr(dx), L.stream())


@pytest.mark.parametrize("n_neg,n_pos", C.VIS_CASES)
def test_vis_pair_equals_its_two_halves_evaluated_separately(n_neg, n_pos):
    assert n_neg % 2 == 1
    c = C.vis_case(n_neg, n_pos)
    got = run("vis", c)
    xn, xp, w, g = T(c["x"][:n_neg].copy()), T(c["x"][n_neg:].copy()), T(c["w_pos"]), T(c["g"])
    assert xn.data_ptr() % 16 == 0 and xp.data_ptr() % 16 == 0
    out = torch.zeros(1, device=DEV)
    _logsig(xn, None, -1.0, 0.1 / n_neg, out=out)
    _logsig(xp, w, 1.0, 1.0 / n_neg, out=out)
    dn, dp = torch.full_like(xn, float("nan")), torch.full_like(xp, float("nan"))
    _logsig(xn, None, -1.0, 0.1 / n_neg, g=g, dx=dn)
    _logsig(xp, w, 1.0, 1.0 / n_neg, g=g, dx=dp)
    assert np.array_equal(bits(np.concatenate([np_(dn), np_(dp)])), bits(got["dx_vis"]))
    if max(n_neg, n_pos) <= 256:
        assert np.array_equal(bits(np_(out)), bits(got["vis_loss"]))


def test_expand_rows_backward_past_the_row_limit_of_one_launch():
    F, k, Ccol, LIMIT = 65537, 2, 3, 65535
    rng = np.random.default_rng(6300)
    g = np.ascontiguousarray(rng.normal(size=(F * k, Ccol)), np.float32)
    x = torch.zeros((F, Ccol), device=DEV, requires_grad=True)
    gt = T(g)
    A.ExpandRowsFn.apply(x, k).backward(gt)
    got = np_(x.grad)
    by_hand = torch.full((F, Ccol), float("nan"), device=DEV)
    for r0, r1 in ((0, LIMIT), (LIMIT, F)):
        L.call("moda_segsum_f32", L.ptr(gt[r0 * k:r1 * k]), r1 - r0, k, Ccol, Ccol, L.ptr(by_hand[r0:r1]), Ccol, L.stream())
    assert np.array_equal(bits(got), bits(np_(by_hand)))
    c = dict(x=np.zeros((F, Ccol), np.float32), k=k, g=g)
    truth, cond = cn.rows_grads(c["x"], k, g)["dx_rows"], cn.rows_condition(c["x"], k, g)["dx_rows"]
    assert cn.ratio(got, truth, cond).max() <= cn.FLOOR["dx_rows"]
