"""GPU: the optimiser stage (moda_amd/optim.py, csrc/optim_kernels.hip) against the oracle of tests/optim_numpy.py, which
tests/test_optim_oracle.py holds against torch on the CPU.

Parameters and moments are compared BIT FOR BIT with the fp32 restatement: the kernel performs the same fp32 operations in the same
order (contraction is off for the file, divide and square root are the correctly rounded ones), and the per-segment scalars are
float64 expressions rounded once.  The learning-rate tables are compared with the float64 schedule rounded to fp32.

The shared case (optim_numpy.TENSORS): sizes 1, 5, 4096 (one chunk), 4097 and 9000; one parameter and gradient 4 bytes off 16-byte
alignment; two tensors in one group; empty groups; 10x groups and a root-pose group; a parameter whose gradient appears in step 3;
a gradient of zeros in step 5; gradient magnitudes from 1 to 1e-6; a name in no group; 14 steps across the schedule's peak."""
import functools

import numpy as np
import pytest
import torch

import optim_numpy as on
from moda_amd import optim as OP, train_utils as TU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = len(TU.GRAD_GROUPS)


@pytest.fixture(autouse=True)
def _restore_precision():
    """TrainHarness sets the process-wide training precision (bf16 here); the tests of other files must not inherit it."""
    import moda_amd
    prev_train, prev = moda_amd.get_train_precision(), moda_amd.get_precision()
    yield
    moda_amd.set_train_precision(prev_train)
    moda_amd.set_precision(prev)


def np_(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


GROUPS = {n: TU.grad_group(n) for n, _, _, _ in on.TENSORS if TU.grad_group(n) is not None}
MAX_LR = [f * on.LEARNING_RATE for f in OP.group_lr_factors(on.ROOT_BASIS)]


@functools.lru_cache(maxsize=None)
def oracle_run(late_from=3, total_steps=on.TOTAL_STEPS, pct_start=on.PCT_START, n_steps=on.N_STEPS):
    """The oracle over the shared case, once per variant: per step (lr applied, lr after scheduler.step(), parameters), and the
    oracle itself at the end.  Nothing here is changed by the tests."""
    o = on.Oracle({n: a for n, a in on.make_params().items() if n in GROUPS}, GROUPS, MAX_LR, total_steps, pct_start)
    steps = []
    for step in range(1, n_steps + 1):
        lr, nxt = o.step({n: g for n, g in on.make_grads(step, late_from=late_from).items() if n in GROUPS})
        steps.append((np.asarray(lr, np.float64).astype(np.float32), np.asarray(nxt, np.float64).astype(np.float32),
                      {n: a.copy() for n, a in o.p.items()}))
    return steps, o


class Scene:
    """The shared case on the device: parameters, and one static gradient buffer per tensor (what a GradBucket's views are), the
    'misaligned' ones one float into their buffers."""

    def __init__(self, params=None):
        self.p, self.gbuf = {}, {}
        start = on.make_params() if params is None else params
        for n, numel, _, flag in on.TENSORS:
            k = 1 if flag == "misaligned" else 0
            pb, gb = torch.zeros(numel + k, device=DEV), torch.zeros(numel + k, device=DEV)
            pb[k:].copy_(torch.from_numpy(np.asarray(start[n], np.float32)))
            self.p[n] = torch.nn.Parameter(pb[k:])
            self.gbuf[n] = gb[k:]
            if flag == "misaligned":
                assert self.p[n].data_ptr() % 16 == 4 and self.gbuf[n].data_ptr() % 16 == 4
        self.named = list(self.p.items())

    def load(self, step, late_from=3):
        for n, g in on.make_grads(step, late_from=late_from).items():
            if g is None:
                self.p[n].grad = None
            else:
                self.gbuf[n].copy_(torch.from_numpy(g))
                self.p[n].grad = self.gbuf[n]

    def optimizer(self, total_steps=on.TOTAL_STEPS, pct_start=on.PCT_START, **kw):
        return OP.DeviceAdamW(self.named, on.LEARNING_RATE, total_steps, pct_start, root_basis=on.ROOT_BASIS, **kw)

    def params(self):
        return {n: np_(p) for n, p in self.p.items()}


def check_params(scene, want, tag=""):
    got = scene.params()
    for n, a in want.items():
        assert same_bits(got[n], a), (tag, n, float(np.abs(got[n].astype(np.float64) - a).max()))
    assert same_bits(got["mystery.weight"], on.make_params()["mystery.weight"])       # in no group: never touched


def test_kernel_matches_the_oracle_bit_for_bit():
    steps, o = oracle_run()
    scene = Scene()
    scene.load(1)
    opt = scene.optimizer()
    assert opt.skipped == ["mystery.weight"] and opt.rebuilds == 1 and "skin_aux" not in opt.seg_names
    for step, (lr, nxt, params) in enumerate(steps, start=1):
        scene.load(step)
        got_lr, status = opt.step()
        assert same_bits(np_(got_lr), lr), (step, np_(got_lr), lr)
        assert same_bits(np_(opt.lr_next), nxt) and same_bits(np.asarray([float(v) for v in opt.lr_views], np.float32), nxt)
        check_params(scene, params, f"step {step}")
        assert np_(status).tolist() == [0, 0, 0, 0] and int(opt.step_count) == step
    assert opt.rebuilds == 2 and "skin_aux" in opt.seg_names              # once more, when skin_aux gained its gradient in step 3
    assert int(np.argmax([s[0][0] for s in steps])) == 7                   # the run crossed the peak
    ks = dict(zip(opt.seg_names, np_(opt.seg_step).tolist()))
    assert ks == {n: o.k[n] for n in opt.seg_names} and ks["skin_aux"] == on.N_STEPS - 2 and ks["bones"] == on.N_STEPS
    for n, off, numel in zip(opt.seg_names, opt._moff, opt._numel):
        assert same_bits(np_(opt.exp_avg[off:off + numel]), o.m[n]) and same_bits(np_(opt.exp_avg_sq[off:off + numel]), o.v[n]), n
        assert same_bits(np_(scene.gbuf[n]), on.make_grads(on.N_STEPS)[n])     # zero_grad is off: the gradients are only read
    # the 10x groups and the root-pose group ('cnn': 0.2x) at the peak, against the plain ones
    peak, gi = steps[7][0], TU.GROUP_INDEX
    assert peak[gi["nerf_coarse"]] == np.float32(on.LEARNING_RATE) and peak[gi["skin_aux"]] == np.float32(10 * on.LEARNING_RATE)
    assert peak[gi["nerf_root_rts"]] == np.float32(0.2 * on.LEARNING_RATE)


def test_zero_gradient_step_moves_parameters_by_decay_and_momentum():
    steps, _ = oracle_run()
    before, after = steps[3][2]["bones"], steps[4][2]["bones"]            # step 5 has an all-zero gradient for `bones`
    assert not on.make_grads(5)["bones"].any() and (before != after).all()


def test_zero_grad_writes_literal_zeros_and_changes_nothing_else():
    steps, _ = oracle_run()
    scene = Scene()
    scene.load(1)
    opt = scene.optimizer(zero_grad=True)
    for step in range(1, 5):
        scene.load(step)
        scene.gbuf["mystery.weight"].fill_(3.0)
        opt.step()
        for n in opt.seg_names:
            assert not bits(np_(scene.gbuf[n])).any(), (step, n)           # +0.0 everywhere, the misaligned and tail quads included
        assert float(scene.gbuf["mystery.weight"].min()) == 3.0            # not this optimiser's tensor
        check_params(scene, steps[step - 1][2], f"step {step}")
    scene.load(5)
    opt.step(zero_grad=False)                                              # the per-call argument overrides the default
    assert bool(scene.gbuf["nerf_coarse.beta"].any())
    check_params(scene, steps[4][2], "step 5")


def test_captured_step_follows_the_schedule():
    """One step captured, replayed 13 times across the peak: the learning rate moves with the device counter, and the parameters are
    the eager run's bit for bit.  (torch's scheduler writes Python floats on the host: a replayed graph keeps the captured rate.)"""
    steps, _ = oracle_run(late_from=1)
    scene = Scene()
    scene.load(1, late_from=1)
    opt = scene.optimizer()
    opt.step()                                                             # step 1, eager
    check_params(scene, steps[0][2], "eager step 1")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lr, status = opt.step()
    assert opt.rebuilds == 1 and int(opt.step_count) == 1                  # the capture executed nothing
    seen = []
    for step in range(2, on.N_STEPS + 1):
        scene.load(step, late_from=1)
        graph.replay()
        assert same_bits(np_(lr), steps[step - 1][0]), step
        assert same_bits(np_(opt.lr_next), steps[step - 1][1]), step
        seen.append(float(lr[0]))
        check_params(scene, steps[step - 1][2], f"replayed step {step}")
    assert int(np.argmax(seen)) == 6 and len(set(seen)) == len(seen)       # warm-up to step 8 (t = 7), then the anneal
    assert int(opt.step_count) == on.N_STEPS and np_(status).tolist() == [0, 0, 0, 0]
    # the same 14 steps eagerly
    eager = Scene()
    e_opt = None
    for step in range(1, on.N_STEPS + 1):
        eager.load(step, late_from=1)
        e_opt = e_opt or eager.optimizer()
        e_opt.step()
    for n in GROUPS:
        assert same_bits(np_(scene.p[n]), np_(eager.p[n])), n


def test_state_dict_round_trip():
    steps, _ = oracle_run()
    scene = Scene()
    scene.load(1)
    opt = scene.optimizer()
    for step in range(1, 8):
        scene.load(step)
        opt.step()
    sd = opt.state_dict()
    assert sd["step"] == 7 and sd["state"]["skin_aux"]["step"] == 5 and sd["state"]["bones"]["exp_avg"].shape == (on.CHUNK + 5,)
    fresh = Scene(params=scene.params())
    fresh.load(8)
    opt2 = fresh.optimizer()
    opt2.load_state_dict(sd)
    for step in range(8, on.N_STEPS + 1):
        fresh.load(step)
        opt2.step()
    check_params(fresh, steps[-1][2], "7 steps, save, load, 7 steps")
    assert int(opt2.step_count) == on.N_STEPS
    with pytest.raises(ValueError, match="nobody"):
        opt2.load_state_dict({"step": 0, "state": {"nobody": sd["state"]["bones"]}})


def test_past_total_steps_the_rate_is_held_and_counted():
    total, pct, n = 4, 0.5, 8
    steps, o = oracle_run(total_steps=total, pct_start=pct, n_steps=n)
    scene = Scene()
    scene.load(1)
    opt = scene.optimizer(total_steps=total, pct_start=pct)
    for step, (lr, nxt, params) in enumerate(steps, start=1):
        scene.load(step)
        got_lr, status = opt.step()
        assert same_bits(np_(got_lr), lr) and same_bits(np_(opt.lr_next), nxt), step
        check_params(scene, params, f"step {step}")
        assert int(status[0]) == max(0, step - 1 - total)                  # the steps whose counter t = step - 1 was past total_steps
    held = np.asarray([on.one_cycle_lr(mx, total, pct, total)[0] for mx in MAX_LR]).astype(np.float32)
    assert same_bits(steps[-1][0], held) and same_bits(steps[4][0], held) and o.overrun == 3
    torch.cuda.synchronize()                                               # no fault


def test_moved_gradient_rebuilds_eagerly_and_raises_under_capture():
    steps, _ = oracle_run()
    scene = Scene()
    scene.load(1)
    opt = scene.optimizer()
    opt.step()
    p = scene.p["bones"]
    scene.load(2)
    scene.gbuf["bones"] = scene.gbuf["bones"].clone()                      # what zero_grad(set_to_none=True) + backward does
    p.grad = scene.gbuf["bones"]
    opt.step()
    assert opt.rebuilds == 2
    check_params(scene, steps[1][2], "step 2 after a rebuild")             # the state was carried over by name
    scene.gbuf["bones"] = scene.gbuf["bones"].clone()
    p.grad = scene.gbuf["bones"]
    x = torch.zeros(4, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x.add_(1.0)
        with pytest.raises(RuntimeError, match="has moved"):
            opt.step()
    assert opt.rebuilds == 2 and int(opt.step_count) == 2


def test_device_tensors_of_another_kind_are_refused_by_name():
    good = torch.nn.Parameter(torch.zeros(8, device=DEV))
    good.grad = torch.zeros(8, device=DEV)
    strided = torch.nn.Parameter(torch.zeros(4, 2, device=DEV))
    strided.grad = torch.zeros(4, 4, device=DEV)[:, :2]
    with pytest.raises(ValueError, match="the gradient of nerf_vis.w"):
        OP.DeviceAdamW([("bones", good), ("nerf_vis.w", strided)], 5e-4, 40, 0.2)
    # (a gradient of another dtype than its parameter is refused by torch itself at the assignment)
    half = torch.nn.Parameter(torch.zeros(4, device=DEV, dtype=torch.float16))
    with pytest.raises(ValueError, match="parameter nerf_vis.h"):
        OP.DeviceAdamW([("bones", good), ("nerf_vis.h", half)], 5e-4, 40, 0.2)


# ---- build_optimizer / optimizer_step: the drop-in ------------------------------------------------------------------------------------
class TinyModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.nerf_coarse = torch.nn.Linear(3, 2)
        self.nerf_root_rts = torch.nn.Linear(2, 2)
        self.near_far = torch.nn.Parameter(torch.zeros(4, 2))              # falls through the name chain: not optimised
        self.skin_aux = torch.nn.Parameter(torch.zeros(2))
        self.root_basis = "exp"


def test_build_optimizer_and_optimizer_step_fill_aux_out():
    import types
    model = TinyModel().to(DEV)
    opts = types.SimpleNamespace(learning_rate=5e-4)
    opt = OP.build_optimizer(model, opts, final_steps=80, num_epochs=10, accu_steps=2)
    assert opt.total_steps == 40 and opt.pct_start == 0.2 and opt.skipped == ["near_far"] and opt.root_basis == "exp"
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    near_far = model.near_far.detach().clone()
    aux = {}
    assert OP.optimizer_step(model, aux) is opt
    torch.cuda.synchronize()
    want = np.asarray([on.one_cycle_lr(f * 5e-4, 40, 0.2, 1)[0] for f in OP.group_lr_factors("exp")]).astype(np.float32)
    assert sorted(aux) == ["lr_%02d" % i for i in range(G)]
    assert same_bits(np.asarray([float(aux["lr_%02d" % i]) for i in range(G)], np.float32), want)      # after scheduler.step()
    assert want[10] == want[18] > 9 * want[0]                               # root_basis 'exp' and skin_aux: both 10x
    assert torch.equal(model.near_far.detach(), near_far) and bool(model.near_far.grad.all())           # untouched, its grad too
    assert not model.skin_aux.grad.any() and not model.nerf_coarse.weight.grad.any()                   # optimizer.zero_grad()
    assert bool((model.skin_aux.detach() != 0).all())


# ---- the harness ------------------------------------------------------------------------------------------------------------------
H_KW = dict(N=256, S=16, default_losses=True, root_pose=True, clip_grad=True)


def record_grads(h):
    """After every fwd_bwd of `h`, its gradients are copied into static tensors (a capturable copy)."""
    rec, inner = {}, h.fwd_bwd

    def fwd_bwd():
        loss = inner()
        for i, p in enumerate(h.params):
            if p.grad is not None:
                if i not in rec:
                    rec[i] = torch.empty_like(p.grad)
                rec[i].copy_(p.grad)
        return loss
    h.fwd_bwd = fwd_bwd
    return rec


def feed_grads(h, rec):
    """After every fwd_bwd of `h`, its gradients are REPLACED by the recorded ones: the stages behind it see the same input."""
    inner = h.fwd_bwd

    def fwd_bwd():
        loss = inner()
        for i, p in enumerate(h.params):
            assert (p.grad is not None) == (i in rec)
            if p.grad is not None:
                p.grad.copy_(rec[i])
        return loss
    h.fwd_bwd = fwd_bwd


def test_harness_with_the_device_optimizer_eager_and_captured():
    """The captured and the eager form of the step agree on the parameters after 6 steps.  The backward's per-bone sums are fp32
    atomics, so two runs of it differ in the last bits; as in tests/test_gpu_clip_grad.py the eager harness is therefore fed the
    gradients the captured one produced, and the stages behind fwd_bwd -- clip, optimiser -- must then agree within that test's bar,
    steps * (64 u * lr + ulp(p)) with lr the largest rate any group reaches.  (This optimiser has no reduction: they agree exactly.)"""
    from gpu_helpers import TrainHarness
    kw = dict(device_optimizer=True, total_steps=40, num_epochs=10, **H_KW)
    a, b = TrainHarness(**kw), TrainHarness(**kw)
    assert a.opt is None and isinstance(a.dev_opt, OP.DeviceAdamW) and a.dev_opt.skipped == []
    assert a.dev_opt.total_steps == 40 and a.dev_opt.pct_start == 0.2
    rec = record_grads(a)
    feed_grads(b, rec)
    start = [p.detach().clone() for p in a.params]
    a.eager_step()
    b.eager_step()
    assert a.dev_opt.rebuilds == 2                                         # built without gradients, rebuilt over the bucket's views
    a.capture(warm=0)
    assert a.graph_form == "one graph" and a.dev_opt.rebuilds == 2
    lrs = [float(a.dev_opt.lr_views[0])]
    for _ in range(5):
        a.step()
        b.eager_step()
        lrs.append(float(a.dev_opt.lr_views[0]))
    torch.cuda.synchronize()
    assert a.dev_opt.rebuilds == 2 and int(a.dev_opt.step_count) == int(b.dev_opt.step_count) == 6
    assert np.isfinite(a.loss()) and np.isfinite(b.loss())
    want = [float(np.float32(on.one_cycle_lr(2e-5, 40, 0.2, t)[0])) for t in range(1, 7)]
    assert lrs == want and all(x < y for x, y in zip(lrs, lrs[1:]))        # warm-up, in the captured step too
    assert np_(a.dev_opt.status).tolist() == [0, 0, 0, 0]
    u, lr_max, worst, exact = 2.0 ** -24, 10 * 2e-5, 0.0, True
    for p, q in zip(a.params, b.params):
        p, q = p.detach(), q.detach()
        bar = 6 * (64 * u * lr_max + torch.from_numpy(np.spacing(np.abs(np_(q)).astype(np.float32))).to(q.device))
        worst = max(worst, float(((p - q).abs() / bar).max()))
        exact = exact and torch.equal(p, q)
    print(f"captured against eager after 6 steps: worst parameter difference / bar = {worst:.3f}, bit-identical: {exact}")
    assert worst <= 1.0
    assert [id(p) for _, p in a.named_params()] == [id(p) for p in a.params]
    moved = [n for (n, p), q in zip(a.named_params(), start) if not torch.equal(p.detach(), q)]
    assert any(n.startswith("nerf_root_rts.") for n in moved) and any(n.startswith("nerf_coarse.") for n in moved) and "bones" in moved


def test_harness_needs_the_schedule_and_a_group_for_every_parameter():
    from gpu_helpers import TrainHarness
    with pytest.raises(ValueError, match="total_steps"):
        TrainHarness(N=64, S=16, device_optimizer=True)


def test_harness_default_path_is_unchanged():
    """With the flag off the harness is what it was: torch's AdamW at a constant rate, no device optimiser, no optimiser launch."""
    from gpu_helpers import TrainHarness
    from moda_amd import _lib as L
    calls, real_call = [], L.call
    h = TrainHarness(N=64, S=16)
    assert h.dev_opt is None and type(h.opt) is torch.optim.AdamW and h.opt.defaults["lr"] == 2e-5
    assert h.opt.defaults["weight_decay"] == 1e-4 and h.opt.defaults["capturable"] and h.opt.defaults["betas"] == (0.9, 0.999)
    stepped = []
    inner = h.opt.step
    h.opt.step = lambda *a, **k: (stepped.append(1), inner(*a, **k))[1]
    L.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        h.eager_step()
    finally:
        L.call = real_call
    torch.cuda.synchronize()
    assert stepped == [1] and "moda_adamw_step" not in calls and np.isfinite(h.loss())
