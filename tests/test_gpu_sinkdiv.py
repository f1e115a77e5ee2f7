"""GPU (-m gpu): the device-resident Sinkhorn divergence (moda_amd/csrc/sinkdiv_kernels.hip, moda_amd.samples_loss) against the
float64 restatement of tests/sinkdiv_numpy.py, and the bone-location term threaded through bone_loc_loss, forward_loss and the
training harness.

Parity bar: the same restatement run in torch float32 on the CPU over the whole case family measures what fp32 arithmetic itself
loses against float64; the kernels may lose at most 4 x the family-wide maximum of that (a different summation order, the
hardware exp / log).  For the loss the bar is not below 4 * 2^-24 * P, P the largest absolute final potential: one rounding of a
potential does not average out of a mean of differences.

The gradient's family is split by conditioning, so that an outlier does not set everybody's bar.  The last softmin's exponent
h_k - C_rk / eps is a difference of two terms of size d^2 / (2 blur^2), each rounded to fp32 before any exponential, so one ulp
of it is 2^-23 d^2 / (2 blur^2): 1e-3 at the workload's diameter 7.3 and 2e-3 at 9 (10 steps), but 0.1 for the two clouds 60
apart and 0.5 at diameter 145 (14 steps) -- there a softmax weight is wrong by ten per cent and more in ANY fp32 evaluation, and
the fp32 restatement loses 1e-2 and 5e-4 where it loses 1e-6 - 3e-5 elsewhere.  COARSE_ULP = 2^-6 separates the two classes
from the float64 diameter alone, not from any result.  Well-conditioned cases, bone_loc_loss and the harness: 4 x the maximum
over the well-conditioned class.  A coarse case: 4 x its own fp32 error (never above the family-wide figure)."""
import types

import numpy as np
import pytest
import torch

import sinkdiv_numpy as sn

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import moda_amd
    from moda_amd import synth, feeders as FD, loss_utils as LU
    from moda_amd.samples_loss import SamplesLoss, BAD_DIAMETER, TOO_MANY_STEPS
    from gpu_helpers import T, DEV, make_models

SHAPES = ((1, 1), (1, 65), (3, 70), (25, 1000), (36, 1000), (63, 64), (64, 64), (65, 129), (70, 1000), (1000, 25))
STEP_DIAMETERS = {8: 0.05 * 2 ** 5.5, 10: 0.05 * 2 ** 7.5, 14: 0.05 * 2 ** 11.5}


def make_case(name):
    """-> (x (N,3), y (M,3)) float32, the joint diameter placed where frac(log2(d / blur)) is far from 0 and 1."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("shape"):
        N, M = (int(v) for v in name.split("_")[1:])
        if (N, M) == (1, 1):
            x, y = np.array([[0.3, -0.2, 0.1]]), np.array([[-0.4, 0.5, -0.3]])
        else:
            x, y = sn.gaussian_bones(rng, N), sn.squashed_sphere(rng, M)
        x, y = sn.with_diameter(x, y, 7.3)
    elif name == "far":                                          # two clouds 60 apart: C / eps ~ 7e5 at the last step
        x, y = sn.gaussian_bones(rng, 25), sn.squashed_sphere(rng, 200, centre=(6.0, 0.0, 0.0))
        x, y = sn.with_diameter(x, y, 66.0)
    elif name == "duplicates":
        x, y = sn.gaussian_bones(rng, 12), sn.squashed_sphere(rng, 90)
        x, y = np.concatenate([x, x[:5], x[:1]]), np.concatenate([y, y[:40]])
        x, y = sn.with_diameter(x, y, 7.3)
    elif name == "subset":
        y = sn.squashed_sphere(rng, 130)
        x = y[:20].copy()
        x, y = sn.with_diameter(x, y, 7.3)
    elif name == "same":
        y = sn.squashed_sphere(rng, 70)
        y, _ = sn.with_diameter(y, y, 7.3)
        x = y.copy()
    elif name.startswith("steps"):
        x, y = sn.gaussian_bones(rng, 25), sn.squashed_sphere(rng, 150)
        x, y = sn.with_diameter(x, y, STEP_DIAMETERS[int(name.split("_")[1])])
    else:
        raise KeyError(name)
    return x.astype(np.float32), y.astype(np.float32)


CASES = tuple(f"shape_{n}_{m}" for n, m in SHAPES) + ("far", "duplicates", "subset", "same", "steps_8", "steps_10", "steps_14")


COARSE_ULP = 2.0 ** -6


def exponent_ulp(d, blur=0.05):
    """One fp32 ulp of the last softmin's exponent terms, of size d^2 / (2 blur^2)."""
    return 2.0 ** -23 * d * d / (2 * blur * blur)


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


@pytest.fixture(scope="module")
def family():
    """Per case: inputs, the float64 restatement, and the fp32 restatement's own errors; plus their family-wide maxima."""
    fam = {}
    for name in CASES:
        x, y = make_case(name)
        ref = sn.sinkdiv(x, y)
        assert 0.05 <= sn.frac_log2(ref["d"]) <= 0.95, (name, ref["d"])
        tx, ty = torch.tensor(x, requires_grad=True), torch.tensor(y, requires_grad=True)
        loss32, info = sn.sinkdiv_torch(tx, ty)
        gx32, gy32 = torch.autograd.grad(loss32, (tx, ty))
        assert info["n"] == ref["n"]
        P = max(np.abs(ref[k]).max() for k in ("a_x", "b_x", "a_y", "b_y"))
        e = dict(P=P)
        if name != "same":                                        # loss 0, gradients 0: no relative error to measure
            e["loss"] = abs(float(loss32.detach()) - ref["loss"]) / abs(ref["loss"])
            e["gx"] = rel_l2(gx32.numpy(), ref["grad_x"])
            e["gy"] = rel_l2(gy32.numpy(), ref["grad_y"])
        fam[name] = dict(x=x, y=y, ref=ref, fp32=e)
    loss_bar = 4 * max(c["fp32"]["loss"] for c in fam.values() if "loss" in c["fp32"])
    own = {name: max(c["fp32"]["gx"], c["fp32"]["gy"]) for name, c in fam.items() if "gx" in c["fp32"]}
    coarse = {name for name, c in fam.items() if exponent_ulp(c["ref"]["d"]) > COARSE_ULP}
    assert coarse == {"far", "steps_14"}, coarse
    grad_bar = 4 * max(e for name, e in own.items() if name not in coarse)
    case_bar = {name: (4 * own[name] if name in coarse else grad_bar) for name in own}
    assert all(b <= 4 * max(own.values()) for b in case_bar.values())      # nowhere above 4 x the family-wide maximum
    print(f"\nfp32 restatement vs float64 over the family: loss bar {loss_bar:.3e} (rel), gradient bar {grad_bar:.3e} (rel L2; "
          + ", ".join(f"{name}: {case_bar[name]:.3e}" for name in sorted(coarse)) + f"; family-wide {4 * max(own.values()):.3e})")
    return dict(cases=fam, loss_bar=loss_bar, grad_bar=grad_bar, case_bar=case_bar)


def run(x, y, **kw):
    """-> (loss float, grad_x, grad_y numpy, status numpy) of one eager call."""
    fn = SamplesLoss("sinkhorn", p=2, blur=.05, **kw)
    tx, ty = T(x).requires_grad_(True), T(y).requires_grad_(True)
    loss = fn(tx, ty)
    gx, gy = torch.autograd.grad(loss, (tx, ty))
    return loss.detach().cpu().numpy(), gx.cpu().numpy(), gy.cpu().numpy(), fn.status.cpu().numpy()


@pytest.mark.parametrize("name", [c for c in CASES if c != "same"])
def test_parity_with_the_float64_restatement(family, name):
    c = family["cases"][name]
    ref = c["ref"]
    loss, gx, gy, status = run(c["x"], c["y"])
    assert status[0] == 0 and status[1] == ref["n"], (status, ref["n"])
    d_dev = float(np.array([status[2]], np.int32).view(np.float32)[0])
    assert abs(d_dev - ref["d"]) <= 2e-7 * ref["d"]
    bar_loss = max(family["loss_bar"] * abs(ref["loss"]), 4 * 2.0 ** -24 * c["fp32"]["P"])
    e_loss, e_gx, e_gy = abs(float(loss) - ref["loss"]), rel_l2(gx, ref["grad_x"]), rel_l2(gy, ref["grad_y"])
    bar = family["case_bar"][name]
    print(f"\n{name}: n {ref['n']} loss {ref['loss']:.6e} |err| {e_loss:.3e} = {e_loss / bar_loss:.3f} of the bar; grad_x {e_gx:.3e}, "
          f"grad_y {e_gy:.3e} = {e_gx / bar:.3f}, {e_gy / bar:.3f} of the bar {bar:.3e} "
          f"(fp32 restatement: {c['fp32']['loss']:.3e}, {c['fp32']['gx']:.3e}, {c['fp32']['gy']:.3e})")
    assert e_loss <= bar_loss
    assert e_gx <= bar and e_gy <= bar


def test_identical_clouds(family):
    c = family["cases"]["same"]
    ref = c["ref"]
    loss, gx, gy, status = run(c["x"], c["y"])
    assert status[0] == 0 and status[1] == ref["n"]
    assert abs(float(loss) - ref["loss"]) <= 4 * 2.0 ** -24 * c["fp32"]["P"]
    # absolute: each gradient is the difference of two softmax-weighted means of offsets no longer than d, over the weight 1 / N
    scale = ref["d"] / c["x"].shape[0]
    assert np.abs(gx - ref["grad_x"]).max() <= family["grad_bar"] * scale and np.abs(gy - ref["grad_y"]).max() <= family["grad_bar"] * scale


def test_two_runs_are_bit_identical(family):
    for name in ("shape_36_1000", "shape_65_129"):
        c = family["cases"][name]
        a, b = run(c["x"], c["y"]), run(c["x"], c["y"])
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes()


def test_status_flags():
    x = np.full((5, 3), 0.25, np.float32)
    loss, gx, gy, status = run(x, np.full((9, 3), 0.25, np.float32))                     # d = 0
    assert status[0] == BAD_DIAMETER and np.isnan(loss) and not gx.any() and not gy.any()
    xr, yr = make_case("shape_3_70")
    loss, gx, gy, status = run(xr, yr, diameter=0.05 * 2.0 ** 22.5)                      # 25 steps: one more than the capacity
    assert status[0] == TOO_MANY_STEPS and status[1] == 0 and np.isnan(loss) and not gx.any() and not gy.any()
    loss, gx, gy, status = run(xr, yr, diameter=0.05 * 2.0 ** 21.5)                      # 24 steps: the capacity
    assert status[0] == 0 and status[1] == 24 and np.isfinite(loss)
    bad = xr.copy()
    bad[1, 2] = np.nan
    for kw in (dict(), dict(diameter=7.3)):                       # a given diameter does not switch the coordinate check off
        loss, gx, gy, status = run(bad, yr, **kw)
        assert status[0] == BAD_DIAMETER and status[1] == 0 and np.isnan(loss) and not gx.any() and not gy.any(), kw
    bad = yr.copy()
    bad[69, 0] = np.inf
    loss, gx, gy, status = run(xr, bad, diameter=7.3)
    assert status[0] == BAD_DIAMETER and np.isnan(loss) and not gx.any() and not gy.any()


def test_diameter_option_is_honoured(family):
    c = family["cases"]["shape_3_70"]
    ref = sn.sinkdiv(c["x"], c["y"], diameter=15.0)
    loss, gx, gy, status = run(c["x"], c["y"], diameter=15.0)
    assert status[1] == ref["n"] == c["ref"]["n"] + 1
    assert abs(float(loss) - ref["loss"]) <= max(family["loss_bar"] * abs(ref["loss"]), 4 * 2.0 ** -24 * c["fp32"]["P"])
    assert rel_l2(gx, ref["grad_x"]) <= family["grad_bar"]


def test_replay_follows_the_schedule_length_of_new_inputs(family):
    """One capture; inputs of 8 and then 14 schedule steps written into the same buffers: the schedule is decided on the device."""
    c8, c14 = family["cases"]["steps_8"], family["cases"]["steps_14"]
    fn = SamplesLoss("sinkhorn", p=2, blur=.05)
    xs, ys = T(c8["x"]).requires_grad_(True), T(c8["y"]).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(fn(xs, ys), (xs, ys))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = fn(xs, ys)
        gx, gy = torch.autograd.grad(loss, (xs, ys))
    for c in (c8, c14, c8):
        with torch.no_grad():
            xs.copy_(T(c["x"]))
            ys.copy_(T(c["y"]))
        graph.replay()
        torch.cuda.synchronize()
        got = (loss.detach().cpu().numpy(), gx.cpu().numpy(), gy.cpu().numpy())
        assert int(fn.status[1]) == c["ref"]["n"]
        want = run(c["x"], c["y"])
        for u, v in zip(got, want[:3]):
            assert u.tobytes() == v.tobytes()


def test_backward_scales_by_the_upstream_gradient(family):
    c = family["cases"]["shape_3_70"]
    _, gx1, gy1, _ = run(c["x"], c["y"])
    tx, ty = T(c["x"]).requires_grad_(True), T(c["y"]).requires_grad_(True)
    (SamplesLoss()(tx, ty) * -2.5).backward()
    assert np.array_equal(tx.grad.cpu().numpy(), gx1 * np.float32(-2.5)) and np.array_equal(ty.grad.cpu().numpy(), gy1 * np.float32(-2.5))
    tx2 = T(c["x"]).requires_grad_(True)                           # no gradient asked for y: none is computed
    SamplesLoss()(tx2, T(c["y"])).backward()
    assert np.array_equal(tx2.grad.cpu().numpy(), gx1)


def tiny_model(B=4, C=32):
    hk = dict(D=8, W=256, in_channels_xyz=C, in_channels_dir=0, out_channels=7 * B)
    head_p = synth.nerf_params(31, "sinkdiv/head", **hk)
    head_p["rgb.0.weight"] = head_p["rgb.0.weight"] * np.float32(0.05)
    head_p["rgb.0.bias"] = np.tile(np.asarray([0, 0, 0, 1, 0, 0, 0], np.float32), B) + np.float32(0.1) * synth.normal(31, "sinkdiv/b", (7 * B,))
    head = FD.DQ_RTHead(use_quat=True, in_channels_xyz=C, in_channels_dir=0, out_channels=7 * B, raw_feat=True)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in head_p.items()})
    model = types.SimpleNamespace(device=DEV)
    model.nerf_body_rts = torch.nn.Sequential(torch.nn.Identity(), head.to(DEV).train())
    model.bones = torch.nn.Parameter(T(synth.make_bones(31, B)))
    model.rest_pose_code = torch.nn.Embedding(1, C).to(DEV)
    model.rest_pose_code.weight.data = T(np.float32(0.3) * synth.normal(31, "sinkdiv/code", (1, C)))
    return model, head


def test_bone_loc_loss_reaches_the_model_and_matches_autograd(family):
    model, head = tiny_model()
    v, f = synth.make_rest_mesh(2)
    mesh = moda_amd.TriMesh(T(v), torch.from_numpy(f).to(DEV))
    u = T(synth.uniform(31, "sinkdiv/u", (128, 3)))
    params = [model.bones, model.rest_pose_code.weight, head.rgb[0].weight, head.rgb[0].bias]
    fn = SamplesLoss("sinkhorn", p=2, blur=.05)
    loss = LU.bone_loc_loss(model, mesh, num_samples=128, u=u, samples_loss=fn)
    status = fn.status.cpu().numpy()                               # the caller's instance: its status tells of a flagged term
    got = torch.autograd.grad(loss, params)
    plain = types.SimpleNamespace(vertices=v, faces=f)             # numpy vertices / faces, as a trimesh.Trimesh holds them
    loss_np = LU.bone_loc_loss(model, plain, num_samples=128, u=u)
    assert torch.equal(loss_np.detach(), loss.detach())
    for g, h in zip(got, torch.autograd.grad(loss_np, params)):
        assert torch.equal(g, h)
    # the float32 restatement in torch on the same bones and samples, through torch's own autograd
    bones_rst, _ = FD.correct_bones(model, model.bones)
    samp = moda_amd.sample_points_from_meshes(mesh, u=u)
    ref_loss, info = sn.sinkdiv_torch(bones_rst[:, :3] * 10, samp * 10)
    want = torch.autograd.grad(ref_loss, params)
    assert status[0] == 0 and status[1] == info["n"]
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= max(family["loss_bar"] * abs(float(ref_loss.detach())),
                                                                       4 * 2.0 ** -24 * info["P"])
    for name, g, w in zip(("bones", "rest_pose_code", "head weight", "head bias"), got, want):
        assert float(w.norm()) > 0, name
        e = float((g - w).norm() / w.norm())
        print(f"\nbone_loc_loss d {name}: rel L2 {e:.3e} ({e / family['grad_bar']:.3f} of the bar)")
        assert e <= family["grad_bar"], (name, e)


def test_forward_loss_adds_the_weighted_term():
    rng = np.random.default_rng(3)
    n = 96
    rendered = {k: T(rng.random((n, c)).astype(np.float32)) for k, c in
                (("img_loss_samp", 3), ("sil_loss_samp", 1), ("frnd_loss_samp", 1), ("feat_err", 1), ("proj_err", 1), ("sil_coarse", 1))}
    rendered["sil_at_samp"] = T((rng.random((n, 1)) > 0.3).astype(np.float32))
    rendered["vis_at_samp"] = T((rng.random((n, 1)) > 0.2).astype(np.float32))
    base = dict(loss_flt=False, root_sm=False, use_corresp=False, total_wt=0.7)
    xr, yr = make_case("shape_3_70")
    x = T(xr).requires_grad_(True)
    t = SamplesLoss()(x, T(yr))
    total0, aux0 = LU.forward_loss(rendered, dict(base, bone_loc_reg=0.0))
    total1, aux1 = LU.forward_loss(rendered, dict(base), bone_loc=t)                     # the default bone_loc_reg = 0.1
    skipped, aux2 = LU.forward_loss(rendered, dict(base), bone_loc=False)
    assert "bone_loc_loss" not in aux0 and "bone_loc_loss" not in aux2 and float(skipped) == float(total0)
    tv = float(t.detach())
    assert abs(float(aux1["bone_loc_loss"]) - 0.1 * tv) <= 2.0 ** -22 * abs(0.1 * tv)
    want = float(total0.detach()) + 0.1 * tv * 0.7
    assert abs(float(total1.detach()) - want) <= 2.0 ** -21 * abs(want)
    keys = list(aux1)
    assert keys.index("bone_loc_loss") < keys.index("total_loss")
    total1.backward()
    _, gx, _, _ = run(xr, yr)
    assert np.abs(x.grad.cpu().numpy() - gx * np.float32(0.1 * 0.7)).max() <= 2.0 ** -21 * np.abs(gx).max() * 0.07
    with pytest.raises(NotImplementedError, match="bone_loc_reg"):
        LU.forward_loss(rendered, dict(base))


def test_harness_step_with_the_term_replays_as_eager(family):
    """The term inside the training step.  (a) From one initial state and one set of draws, the bone gradient of the harness with
    the term differs from that of the harness without it by 0.1 * the term's gradient (float64 restatement).  (b) The captured
    step, replayed, is the eager step: the term bit for bit (it depends on the bones and the uniforms alone), the loss, the loss
    terms and every gradient within the bounds tests/test_gpu_train.py holds the step to (the networks' split-K sums use fp32
    atomics whose order varies: 1e-5 on the loss, 1e-3 relative L2 per gradient tensor, between two eager launches too)."""
    from moda_amd.bench_support import TrainHarness
    kw = dict(N=256, S=16, precision="fp32", lr=5e-4, default_losses=True)
    h, h0 = TrainHarness(bone_loc=True, **kw), TrainHarness(bone_loc=False, **kw)
    grads = {}
    for key, hh in ((True, h), (False, h0)):
        hh.draw()
        hh.zero_grad()
        hh.fwd_bwd()
        grads[key] = hh.models["bones_rst"].grad.detach().clone()
    term = grads_term(h)
    diff = grads[True] - grads[False]
    e = float((diff[:, :3] - term).norm() / term.norm())
    ratio = float(grads[False][:, :3].norm() / term.norm())
    print(f"\nharness: bone gradient difference vs the term's gradient: rel L2 {e:.3e} (rendering gradient / term = {ratio:.3e})")
    # the term within the gradient bar; the two rendering gradients each within the step's run-to-run bound of 1e-3 of their norm
    # (two launches of the rendering backward, whose per-bone sums are fp32 atomics: that allowance cannot be taken out of a
    # difference of two steps, so the term of the harness's own objects is also held to the bar alone, at the end)
    assert e <= family["grad_bar"] + 2e-3 * ratio
    assert float(diff[:, 3:].abs().max()) <= 2e-3 * float(grads[False][:, 3:].abs().max())
    del h0

    h.eager_step()                                                # (the first step builds the gradient bucket)
    h.draw()
    h.zero_grad()
    loss_e = float(h.fwd_bwd())
    terms_e, value_e = h.terms.clone(), h.bone_loc_value.clone()
    grads_e = [None if p.grad is None else p.grad.detach().clone() for p in h.params]
    h.capture(warm=0)
    h.graph.replay()
    torch.cuda.synchronize()
    assert h.graph_form == "one graph"
    assert torch.equal(h.bone_loc_value, value_e) and int(h.samples_loss.status[0]) == 0
    assert abs(h.loss() - loss_e) < 1e-5 * abs(loss_e), (h.loss(), loss_e)
    assert torch.allclose(h.terms, terms_e, rtol=1e-4, atol=1e-7), (h.terms, terms_e)
    for i, (p, ge) in enumerate(zip(h.params, grads_e)):
        assert (p.grad is None) == (ge is None)
        if ge is not None and float(ge.norm()) > 0:
            assert float((p.grad - ge).norm() / ge.norm()) < 1e-3, i
    term = grads_term(h)                                          # (the bones and the uniforms of the replayed step)
    bones = h.models["bones_rst"]
    samp = moda_amd.sample_points_from_meshes(h.mesh_rest, u=h.bone_u)
    own, = torch.autograd.grad(0.1 * h.samples_loss(bones[:, :3] * 10, samp * 10), bones)
    e_own = float((own[:, :3] - term).norm() / term.norm())
    print(f"harness: the term's gradient alone, from the harness's mesh, uniforms and SamplesLoss: rel L2 {e_own:.3e} "
          f"({e_own / family['grad_bar']:.3f} of the bar)")
    assert e_own <= family["grad_bar"] and not own[:, 3:].any()


def grads_term(h):
    """0.1 * d SamplesLoss(bones * 10, samples * 10) / d bones of the harness's current bones and uniforms (float64 restatement)."""
    samp = moda_amd.sample_points_from_meshes(h.mesh_rest, u=h.bone_u)
    x = (h.models["bones_rst"].detach()[:, :3] * 10).cpu().numpy()
    ref = sn.sinkdiv(x, (samp * 10).cpu().numpy())
    return T((ref["grad_x"] * 10 * 0.1).astype(np.float32))
