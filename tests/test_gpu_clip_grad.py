"""GPU (-m gpu): device-resident gradient clipping (moda_amd/train_utils.py, csrc/clip_kernels.hip) against the float64 oracle
tests/clip_numpy.py, on the cases tests/test_clip_oracle.py defines and vets on the CPU (no group norm within 1e-3 of its
threshold, so the kernel must take the oracle's side of every clamp; clamped, unclamped, empty and frozen groups all occur).
Fourteen tensors with numels {1, 3, 4, 5, 7, 4096, 4097, 2 * 4096 + 3}: one- and multi-chunk tensors, tails of 1 and 3 elements,
nerf_coarse and nerf_skin interleaved in parameter order, one gradient 4 bytes off 16-byte alignment (the scalar path), one
parameter without a gradient, one that matches no group; in two layouts, a GradBucket's views and separate tensors.

Every bar is derived, with u = 2^-24 (fp32 unit round-off):

  norms     each fp32 square carries 1 u, so the exact sum of the rounded squares is within 1 u of the true sum; the float64
            accumulation adds n 2^-53, negligible; the square root halves the error and (float)sqrt rounds once more: a norm is
            within 2 u relative of the float64 oracle.
  scaled    coef = min(1, max / (norm + 1e-6)): the norm's 2 u, the addition 1 u, the division 1 u (the oracle takes the SAME
            fp32 thresholds), so coef is within 4 u; the product rounds once: a scaled gradient is within 6 u relative.
  others    a group with coef == 1 and an ungrouped tensor are not written: bit-identical to their input.  Frozen groups are
            exactly 0 and report norm 0.  Empty groups report norm 0.
  invalid   one NaN or +inf anywhere -- the last element of a tail chunk, inside a frozen group, in an ungrouped tensor --
            and every gradient is exactly 0.0, `status` = [1, #NaN, #inf, 0]; in the bucket layout the bucket's `extra` floats
            and the padding between its views keep their bits.
  repeat    no float atomics and a fixed summation tree: two runs agree bit for bit, and so do a captured graph's replay and
            the eager call, and the two layouts (the element-to-lane map does not depend on alignment).
  harness   TrainHarness(N=64, S=16, clip_grad=True), one eager and one captured step, against the same harness with the
            torch restatement (clip_numpy.clip_grad_torch) in the clipper's place.  The backward kernels' split-K sums use fp32
            atomics, so two runs of one step differ by ~1e-4 in the gradients: the second harness is FED the first one's
            gradients, which leaves the clipping stage and AdamW as the only difference.  Propagation of the 6 u gradient
            bound through AdamW (lr, betas (0.9, 0.999), eps 1e-8, decoupled decay): the update is lr * mhat / (sqrt(vhat) +
            eps).  In step 1 mhat = g and vhat = g^2: the update lr g / (|g| + eps) moves by at most lr * delta / 4 under a
            relative change delta of g (the derivative g eps / (|g| + eps)^2 peaks at 1/4).  In step 2 m and sqrt(v) each carry
            the two steps' 6 u, and |mhat| / sqrt(vhat) <= 1.05 for two steps (b1 |g1| + |g2| over 1.9 sqrt((g1^2 + g2^2) / 2)
            with |g1| + |g2| <= 2 sqrt((g1^2 + g2^2) / 2)): 1.05 * 2 * 12 u = 26 u.  The fused kernel's own ~10 fp32 operations
            may each round differently on inputs that differ: 10 u more.  The parameter update p (1 - lr wd) - update then rounds
            once: inputs that differ by d give results that differ by at most d + ulp(p).  Per step: 36 u lr + ulp(p) -- taken as
            64 u lr + ulp(p) to cover clip_grad_norm_'s own fp32 norm (its error is common to a whole group, and AdamW is
            invariant to a common factor in step 1, so only step 2 sees it) -- and the bars of the two steps add.
            With clip_grad=False the harness launches no clipping kernel and its parameters equal, bit for bit, those of the
            step with nothing between the exchange and AdamW."""
import types

import numpy as np
import pytest
import torch

import clip_numpy as cn
from test_clip_oracle import (TENSORS, NAMES, GROUPS, FACTORS, MAX_NORM, GPU_CASES, POISON_AT, CLIP_SCALE, make_grads, frozen_ids,
                              oracle)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import moda_amd
    from moda_amd import _lib as L, train_utils as TU
    from gpu_helpers import DEV, TrainHarness

U = 2.0 ** -24
LAYOUTS = ("bucket", "separate")
SENTINEL = 123.0
EXTRA = (3.25, -7.5)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def np_(t):
    return t.detach().cpu().numpy()


class Scene:
    """The test tensors as parameters on the GPU with their gradients in `layout`."""

    def __init__(self, layout, grads):
        self.named = [(name, torch.nn.Parameter(torch.zeros(n, device=DEV))) for name, n, _, _ in TENSORS]
        self.bucket = None
        if layout == "bucket":      # everything the bucket can hold (its views are 16-byte aligned: the misaligned one stays out)
            self.bucket = moda_amd.GradBucket([p for (_, p), t in zip(self.named, TENSORS) if t[3] is None], extra=len(EXTRA))
            self.bucket.flat.fill_(SENTINEL)
            self.bucket.extra.copy_(torch.tensor(EXTRA))
        self.keep = []
        for (name, p), t in zip(self.named, TENSORS):
            if t[3] == "misaligned":
                buf = torch.zeros(t[1] + 1, device=DEV)
                self.keep.append(buf)
                p.grad = buf[1:]
                assert p.grad.data_ptr() % 16 == 4
            elif t[3] is None and self.bucket is None:
                p.grad = torch.zeros(t[1], device=DEV)
        self.load(grads)

    def load(self, grads):
        for (_, p), g in zip(self.named, grads):
            if g is not None:
                p.grad.copy_(torch.from_numpy(g))

    def grads(self):
        return [None if p.grad is None else np_(p.grad) for _, p in self.named]

    def check_bucket_rest(self):
        """The bucket's floats that are no gradient: padding and `extra`, bit for bit."""
        if self.bucket is None:
            return
        flat = np_(self.bucket.flat)
        mask = np.ones(flat.size, bool)
        for p, off in zip(self.bucket.params, self.bucket.offsets):
            mask[off:off + p.numel()] = False
        want = np.full(flat.size, SENTINEL, np.float32)
        want[self.bucket.n_grad:self.bucket.n_grad + len(EXTRA)] = EXTRA
        assert mask.sum() > len(EXTRA)                       # there IS padding (numels 1, 3, 5 ...)
        assert np.array_equal(bits(flat[mask]), bits(want[mask]))


def check_valid(scene, grads_in, ref, norms, status, frozen):
    norms, status = np_(norms).astype(np.float64), np_(status)
    assert status.tolist() == [0, 0, 0, 0]
    worst_n = worst_g = 0.0
    for gi, (got, want) in enumerate(zip(norms, ref["norms"])):
        if want == 0.0:
            assert got == 0.0, TU.GRAD_GROUPS[gi][0]        # frozen or empty
        else:
            worst_n = max(worst_n, abs(got - want) / want)
    for (name, _), got, g_in, want, gi in zip(scene.named, scene.grads(), grads_in, ref["grads"], GROUPS):
        if want is None:
            assert got is None
            continue
        if gi in frozen:
            assert not got.any(), name                       # exactly 0
        elif gi is None or ref["coef"][gi] == 1.0:
            assert np.array_equal(bits(got), bits(g_in)), name
        else:
            assert ref["coef"][gi] < 1.0
            err = np.abs(got.astype(np.float64) - want) / np.abs(want).clip(1e-300)
            worst_g = max(worst_g, float(err.max()))
    print("worst norm error / u:", worst_n / U, " worst scaled-gradient error / u:", worst_g / U)
    assert worst_n <= 2 * U
    assert worst_g <= 6 * U
    scene.check_bucket_rest()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", sorted(GPU_CASES))
def test_clip_matches_oracle(case, layout):
    c = GPU_CASES[case]
    grads, ref = oracle(c)
    scene = Scene(layout, grads)
    if case == "vis_frozen":
        clipper = TU.GradClipper(scene.named, CLIP_SCALE, frozen=c["frozen"])
    else:                           # the same through set_frozen, by index
        clipper = TU.GradClipper(scene.named, CLIP_SCALE)
        clipper.set_frozen(sorted(frozen_ids(c)))
    assert np.array_equal(bits(np_(clipper.max_norm)), bits(MAX_NORM))
    norms, status = clipper()
    check_valid(scene, grads, ref, norms, status, frozen_ids(c))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("where", sorted(POISON_AT))
@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_nonfinite_rejects_the_step(kind, where, layout):
    c = GPU_CASES["vis_frozen"]
    grads, ref = oracle(c, poison=(kind, where))
    assert ref["invalid"] and (ref["n_nan"], ref["n_inf"]) == ((1, 0) if kind == "nan" else (0, 1))
    scene = Scene(layout, grads)
    clipper = TU.GradClipper(scene.named, CLIP_SCALE, frozen=c["frozen"])
    _, status = clipper()
    assert np_(status).tolist() == [1, ref["n_nan"], ref["n_inf"], 0]
    for (name, _), got in zip(scene.named, scene.grads()):
        if got is not None:
            assert np.array_equal(bits(got), np.zeros(got.size, np.uint32)), name      # +0.0, every one
    scene.check_bucket_rest()


def test_two_runs_and_two_layouts_give_the_same_bits():
    c = GPU_CASES["shape_frozen"]
    grads, _ = oracle(c)
    outs = []
    for layout in ("bucket", "bucket", "separate"):
        scene = Scene(layout, grads)
        norms, _ = TU.GradClipper(scene.named, CLIP_SCALE, frozen=c["frozen"])()
        outs.append((bits(np_(norms)), [None if g is None else bits(g) for g in scene.grads()]))
    for norms, gs in outs[1:]:
        assert np.array_equal(norms, outs[0][0])
        for a, b in zip(gs, outs[0][1]):
            assert (a is None and b is None) or np.array_equal(a, b)


def test_graph_capture_replays_on_new_gradients():
    """Captured once (a call inside capture succeeds: it synchronises nothing and allocates nothing), replayed on gradients
    written afterwards -- a valid step, then a poisoned one -- bit for bit the eager results.  One linear chain of launches."""
    c1, c2 = GPU_CASES["vis_frozen"], GPU_CASES["shape_frozen"]
    g1, g2 = make_grads(c1["seed"]), make_grads(c2["seed"])
    g3, _ = oracle(c2, poison=("inf", "tail"))
    scene = Scene("bucket", g1)
    clipper = TU.GradClipper(scene.named, CLIP_SCALE, frozen=c2["frozen"])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        norms, status = clipper()
    assert clipper.rebuilds == 1
    for g_in in (g2, g3):
        scene.load(g_in)
        graph.replay()
        eager = Scene("bucket", g_in)
        e_norms, e_status = TU.GradClipper(eager.named, CLIP_SCALE, frozen=c2["frozen"])()
        assert np.array_equal(bits(np_(norms)), bits(np_(e_norms)))
        assert np_(status).tolist() == np_(e_status).tolist()
        for a, b in zip(scene.grads(), eager.grads()):
            assert (a is None and b is None) or np.array_equal(bits(a), bits(b))
    assert np_(status).tolist() == [1, 0, 1, 0]


def test_moved_gradient_rebuilds_eagerly_and_raises_under_capture():
    c = GPU_CASES["vis_frozen"]
    grads, ref = oracle(c)
    scene = Scene("separate", grads)
    clipper = TU.GradClipper(scene.named, CLIP_SCALE, frozen=c["frozen"])
    clipper()
    p = scene.named[2][1]
    p.grad = torch.zeros_like(p.grad)                       # what zero_grad(set_to_none=True) + backward does
    scene.load(grads)
    norms, status = clipper()
    assert clipper.rebuilds == 2
    check_valid(scene, grads, ref, norms, status, frozen_ids(c))
    p.grad = torch.zeros_like(p.grad)
    x = torch.zeros(4, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x.add_(1.0)
        with pytest.raises(RuntimeError, match="has moved"):
            clipper()
    assert clipper.rebuilds == 2


class TinyModel(torch.nn.Module):
    """The attributes clip_grad reads off the reference's model, on networks small enough for a unit test."""

    def __init__(self, skips):
        super().__init__()
        kw = dict(D=2, W=16, in_channels_xyz=9, in_channels_dir=0, out_channels=1, raw_feat=True, skips=skips)
        self.nerf_coarse, self.nerf_skin, self.nerf_feat, self.nerf_vis = (moda_amd.NeRF(**kw) for _ in range(4))
        self.nerf_root_rts = torch.nn.Linear(5, 3)
        self.root_code = torch.nn.Embedding(2, 4)
        self.bones = torch.nn.Parameter(torch.zeros(5, 10))
        self.skin_aux = torch.nn.Parameter(torch.zeros(2))
        self.near_far = torch.nn.Parameter(torch.zeros(3, 2))
        self.root_update, self.body_update, self.shape_update, self.cvf_update = 0, 1, 0, 0


def fill_grads(model, seed, scale=0.05):
    gen = torch.Generator().manual_seed(seed)
    for p in model.parameters():
        g = (torch.randn(p.shape, generator=gen) * scale).to(p.device)
        if p.grad is None:
            p.grad = g
        else:
            p.grad.copy_(g)                                  # in place: the gradient tensors stay where they are


@pytest.mark.parametrize("freeze_coarse", [False, True])
def test_clip_grad_drop_in(freeze_coarse):
    """clip_grad(model, aux_out, opts) against the torch restatement given the same frozen sets: root_update == 0 freezes
    root_code and nerf_root_rts; freeze_coarse freezes bones, skin_aux, nerf_vis and, of nerf_coarse / nerf_skin / nerf_feat,
    every tensor but the input layer's weight.  The second call runs inside stream capture: no host synchronisation."""
    model = TinyModel(skips=[]).to(DEV)
    opts = types.SimpleNamespace(clip_scale=0.2, freeze_body_mlp=False, freeze_coarse=freeze_coarse)
    fill_grads(model, 5)
    twin = TinyModel(skips=[]).to(DEV)
    for p, q in zip(model.parameters(), twin.parameters()):
        q.grad = p.grad.clone()
    groups = {"root_code", "nerf_root_rts"} | ({"bones", "skin_aux", "nerf_vis"} if freeze_coarse else set())
    tensors = [n for n, _ in twin.named_parameters() if freeze_coarse and n.split(".")[0] in ("nerf_coarse", "nerf_skin", "nerf_feat")
               and n != n.split(".")[0] + ".xyz_encoding_1.0.weight"]
    ref_norms, invalid = cn.clip_grad_torch(twin.named_parameters(), TU.grad_group, FACTORS, opts.clip_scale,
                                            frozen_groups=[TU.GROUP_INDEX[g] for g in groups], frozen_tensors=tensors)
    assert not invalid
    aux_out = {}
    clipper = TU.clip_grad(model, aux_out, opts)
    assert sorted(aux_out) == sorted(n + "_g" for n, _ in TU.GRAD_GROUPS)
    assert np_(clipper.status).tolist() == [0, 0, 0, 0]
    lo = clipper.norms.data_ptr()
    clamped = 0
    for gi, (name, _) in enumerate(TU.GRAD_GROUPS):
        v = aux_out[name + "_g"]
        assert v.dim() == 0 and v.is_cuda and v.data_ptr() == lo + 4 * gi           # a view of `norms`
        want = float(ref_norms[gi])
        assert abs(float(v) - want) <= 64 * U * want, name    # torch's own fp32 norm of < 1000 elements: a few u
        clamped += want > FACTORS[gi] * opts.clip_scale
    assert clamped >= 2 and float(aux_out["root_code_g"]) == 0.0 and float(aux_out["nerf_root_rts_g"]) == 0.0
    for (name, p), q in zip(model.named_parameters(), twin.parameters()):
        assert torch.allclose(p.grad, q.grad, rtol=64 * U, atol=0.0), name
        if name in tensors or name.startswith(("root_code", "nerf_root_rts")):
            assert not p.grad.any(), name
    assert bool(model.nerf_coarse.xyz_encoding_1[0].weight.grad.any()) and bool(model.near_far.grad.any())
    fill_grads(model, 6)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert TU.clip_grad(model, {}, opts) is clipper
    assert clipper.rebuilds == 1                             # the tables were built once


def test_clip_grad_refuses_a_partial_tensor_freeze():
    """freeze_coarse on a network with a skip layer zeroes columns [63:] of that layer's weight (train_utils.py:1339): part of a
    tensor.  Refused, not approximated."""
    model = TinyModel(skips=[1]).to(DEV)
    fill_grads(model, 7)
    opts = types.SimpleNamespace(clip_scale=1.0, freeze_body_mlp=False, freeze_coarse=True)
    with pytest.raises(NotImplementedError, match="part of a tensor"):
        TU.clip_grad(model, {}, opts)


# ---- the training harness ---------------------------------------------------------------------------------------------------
H_KW = dict(N=64, S=16, precision="bf16", lr=5e-4)
H_CLIP_SCALE = 0.01     # thresholds 0.01 / 0.001 / 1: small enough that groups of the synthetic scene clamp


def ulp32(x):
    return torch.from_numpy(np.spacing(np.abs(np_(x)).astype(np.float32))).to(x.device)


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


def compare_params(a, b, steps, lr, tag):
    worst = 0.0
    for p, q in zip(a.params, b.params):
        p, q = p.detach(), q.detach()
        bar = steps * (64 * U * lr + ulp32(q))
        worst = max(worst, float(((p - q).abs() / bar).max()))
    print(f"{tag}: worst parameter difference / bar = {worst:.3f}")
    assert worst <= 1.0


def test_harness_clips_like_the_torch_restatement(monkeypatch):
    calls = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    a = TrainHarness(clip_grad=True, clip_scale=H_CLIP_SCALE, **H_KW)
    b = TrainHarness(clip_grad=True, clip_scale=H_CLIP_SCALE, **H_KW)
    rec = record_grads(a)
    feed_grads(b, rec)
    b._clip = lambda: cn.clip_grad_torch(b.named_params(), TU.grad_group, FACTORS, H_CLIP_SCALE)
    for p, q in zip(a.params, b.params):
        assert torch.equal(p, q)
    a.eager_step()
    b.eager_step()
    assert calls.count("moda_clip_grad") == 1
    norms = np_(a.clipper.norms)
    assert np_(a.clipper.status).tolist() == [0, 0, 0, 0]
    clamped = [n for (n, f), v in zip(TU.GRAD_GROUPS, norms) if v > f * H_CLIP_SCALE]
    print("norms:", {n: float(v) for (n, _), v in zip(TU.GRAD_GROUPS, norms) if v > 0}, " clamped:", clamped)
    assert clamped                                            # the stage does something here
    compare_params(a, b, 1, H_KW["lr"], "eager step")
    a.capture(warm=0)
    assert a.graph_form == "one graph" and calls.count("moda_clip_grad") == 2       # recorded into the graph
    a.step()
    b.eager_step()
    torch.cuda.synchronize()
    assert calls.count("moda_clip_grad") == 2 and a.clipper.rebuilds == 1
    compare_params(a, b, 2, H_KW["lr"], "captured step")


def test_harness_without_clip_grad_is_the_step_as_it_was(monkeypatch):
    calls = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    a = TrainHarness(**H_KW)                                  # the default: off
    b = TrainHarness(clip_grad=True, **H_KW)
    b._clip = lambda: None                                    # nothing between the exchange and AdamW
    rec = record_grads(a)
    feed_grads(b, rec)
    a.eager_step()
    b.eager_step()
    a.capture(warm=0)
    a.step()
    b.eager_step()
    torch.cuda.synchronize()
    assert not a.clip_grad and a.clipper is None and "moda_clip_grad" not in calls
    for p, q in zip(a.params, b.params):
        assert torch.equal(p, q)
