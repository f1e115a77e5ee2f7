"""GPU: the loss stage with the reference's default flags (csrc/lossasm_kernels.hip) against the float64 restatements of
tests/lossasm_numpy.py -- the frame filter in both modes (flags demanded EXACTLY; the inputs are built in
tests/test_lossasm_oracle.py, which also asserts the conditions that make that a fair demand), root smoothness within a derived
fp32 bound, the full assembly at the tolerance of the existing total_loss test (2e-6), and the whole stage captured in a graph."""
import numpy as np
import pytest
import torch

import lossasm_numpy as ln
import lossasm_cases as cases

pytestmark = pytest.mark.gpu


def T(a, dtype=None):
    t = torch.as_tensor(np.asarray(a))
    return t.to("cuda", dtype) if dtype is not None else t.to("cuda")


def np_(t):
    return t.detach().cpu().numpy()


def run_line(flt, state, errid, frameid, vals, S):
    """One call on the device and on the restatement (which skips the ids outside the table, as the kernel does)."""
    inv = np_(flt(T(vals), T(errid), T(frameid)))
    ok = (errid >= 0) & (errid < state.size)
    st2 = state                                                       # updated in place
    ref_inv_ok, mean, med = ln.loss_filter_line(st2, errid[ok], frameid, vals[ok], S)
    return inv, ref_inv_ok, mean, med, int((~ok).sum())


def test_filter_line_three_calls_then_reset():
    """num_frames=7, img_size=8, N=24, repeated ids in shuffled order, a zero over a positive value, one id outside the table;
    the state persists between the calls; reset() zeroes it.  int64 ids."""
    from moda_amd import loss_utils as LU
    Tn, S, calls = cases.line_calls_small()
    flt = LU.LossFilter(Tn, S)
    state = np.zeros(Tn * S)
    seen_invalid = False
    for errid, frameid, vals in calls:
        inv, ref, mean, med, oob = run_line(flt, state, errid, frameid, vals, S)
        assert inv.dtype == np.bool_ and np.array_equal(inv, ref)
        assert np.array_equal(np_(flt.sil_err).astype(np.float64), state)
        assert np_(flt.status).tolist() == [oob, int(ref.sum()), int((mean > 0).sum()), 0]
        seen_invalid |= bool(ref.any())
    assert seen_invalid
    again = np_(flt(T(calls[2][2]), T(calls[2][0]), T(calls[2][1])))          # the same call on the same state: the same bits
    assert np.array_equal(again, inv)
    flt.reset()
    assert float(flt.sil_err.abs().max()) == 0
    errid, frameid, vals = calls[0]
    inv, ref, *_ = run_line(flt, np.zeros(Tn * S), errid, frameid, vals, S)
    assert np.array_equal(inv, ref)


@pytest.mark.parametrize("K", cases.POSITIVE_COUNTS)
def test_filter_line_positive_frame_counts(K):
    """K frames with a positive mean (two tied, one above ten medians when K >= 3): the median's ranking across the wave and
    block seams; K = 0 is a NaN median that flags nothing.  int32 ids."""
    from moda_amd import loss_utils as LU
    Tn, S, errid, frameid, vals = cases.line_case_counts(K)
    flt = LU.LossFilter(Tn, S)
    inv, ref, mean, med, _ = run_line(flt, np.zeros(Tn * S), errid, frameid, vals, S)
    assert np.array_equal(inv, ref)
    assert np_(flt.status).tolist() == [0, int(ref.sum()), K, 0]


@pytest.mark.parametrize("above", [False, True])
def test_filter_line_at_and_one_step_above_ten_medians(above):
    from moda_amd import loss_utils as LU
    Tn, S, errid, frameid, vals = cases.threshold_case(above)
    flt = LU.LossFilter(Tn, S)
    inv, ref, *_ = run_line(flt, np.zeros(Tn * S), errid, frameid, vals, S)
    assert inv.tolist() == ref.tolist() == [False, False, False, above]


def test_filter_line_img_size_512_random_values_and_drop_in():
    """img_size = 512 with random fp32 values: the restatement's margin to the threshold is asserted first (a condition on the
    inputs), then equality is demanded; the drop-in function with the reference's signature gives the same flags and state."""
    from moda_amd import loss_utils as LU
    Tn, S, errid, frameid, vals = cases.line_case_random()
    state = np.zeros(Tn * S)
    ref, mean, med = ln.loss_filter_line(state, errid, frameid, vals, S)
    assert np.abs(mean - 10 * med).min() > 1e-12 * 10 * med
    flt = LU.LossFilter(Tn, S)
    inv = np_(flt(T(vals).reshape(-1, 1), T(errid), T(frameid)))
    assert np.array_equal(inv, ref)
    assert np.array_equal(np_(flt.sil_err).astype(np.float64), state)
    sil_err = torch.zeros(Tn * S, device="cuda")
    inv2 = LU.loss_filter_line(sil_err, T(errid), T(frameid), T(vals), S)
    assert inv2.is_cuda and np.array_equal(np_(inv2), ref) and torch.equal(sil_err, flt.sil_err)
    with pytest.raises(RuntimeError):
        flt(T(vals).cpu(), T(errid), T(frameid))                     # values must be on the device: no CPU path


@pytest.mark.parametrize("bs", [1, 5])
@pytest.mark.parametrize("K", cases.POSITIVE_COUNTS)
def test_filter_frame_mode(bs, K):
    """lineload=False: flo_err, the flags from the history BEFORE the update, then the update (a repeated id keeps the last row);
    two consecutive calls; the drop-in loss_filter leaves the history alone."""
    from moda_amd import loss_utils as LU
    Tn, hist, x, mask, errid = cases.frame_case(bs, K)
    flt = LU.LossFilter(Tn, 8, lineload=False)
    flt.sil_err.copy_(T(hist))
    state = hist.astype(np.float64)
    fe, inv_d = LU.loss_filter(flt.sil_err.clone(), T(x)[..., None], T(mask)[..., None])
    for call in range(2):
        xs = x if call == 0 else x[::-1].copy()
        inv = np_(flt(T(xs)[..., None], T(errid), mask=T(mask)[..., None]))
        ref, flo_err, med = ln.loss_filter_frame(state, xs, mask, errid)
        assert np.array_equal(inv, ref), call
        assert np.array_equal(np_(flt.flo_err), flo_err)
        assert np.array_equal(np_(flt.sil_err).astype(np.float64), state)
        if call == 0:
            assert np.array_equal(np_(inv_d), ref) and np.array_equal(np_(fe), flo_err)
            assert np_(flt.status).tolist() == [0, int(ref.sum()), K, 0]
            assert ref[0] == (K > 0)                                 # row 0 lies far above ten medians of any history


def run_frame(flt, state, x, mask, errid):
    """One frame-mode call on the device and on the restatement (which skips the ids outside the table, as the kernel does)."""
    inv = np_(flt(T(x)[..., None], T(errid), mask=T(mask)[..., None]))
    ok = (errid >= 0) & (errid < state.size)
    probe = state.copy()
    ref, flo_err, med = ln.loss_filter_frame(probe, x, mask, np.where(ok, errid, 0))
    K = int((state > 0).sum())
    state[errid[ok]] = flo_err[ok]                                   # moda.py:533 without the skipped rows
    return inv, ref, flo_err, K, int((~ok).sum())


@pytest.mark.parametrize("bs", [1, 5])
@pytest.mark.parametrize("above", [False, True])
def test_filter_frame_at_and_one_step_above_ten_medians(bs, above):
    """flo_err exactly at 10 * median is not flagged (strict >), one input step above it is."""
    from moda_amd import loss_utils as LU
    Tn, hist, x, mask, errid = cases.frame_threshold_case(bs, above)
    flt = LU.LossFilter(Tn, 8, lineload=False)
    flt.sil_err.copy_(T(hist))
    inv, ref, *_ = run_frame(flt, hist.astype(np.float64), x, mask, errid)
    assert inv.tolist() == ref.tolist() == [above] + [False] * (bs - 1)


@pytest.mark.parametrize("bs", [1, 5])
def test_filter_frame_random_values(bs):
    """Random fp32 values: the kernel's flo_err (float64 sums, fp32 quotient) lies within fp32 rounding of the restatement's, and
    the restatement keeps every row 1e-5 clear of the threshold (asserted first, a condition on the inputs), so the flags are
    demanded exactly."""
    from moda_amd import loss_utils as LU
    Tn, hist, x, mask, errid = cases.frame_case_random(bs)
    state = hist.astype(np.float64)
    ref, flo_err, med = ln.loss_filter_frame(state.copy(), x, mask, errid)
    assert np.abs(flo_err.astype(np.float64) - 10 * med).min() > 1e-5 * 10 * med
    flt = LU.LossFilter(Tn, 8, lineload=False)
    flt.sil_err.copy_(T(hist))
    inv, ref2, flo_err2, K, _ = run_frame(flt, state, x, mask, errid)
    assert np.array_equal(inv, ref) and np.array_equal(np_(flt.flo_err), flo_err)
    assert np_(flt.status).tolist() == [0, int(ref.sum()), K, 0]


@pytest.mark.parametrize("bs", [1, 5])
def test_filter_frame_three_calls_then_reset(bs):
    """Three calls on one history, an errid outside the table in the second (skipped, counted in status[0]), then reset()."""
    from moda_amd import loss_utils as LU
    Tn, calls = cases.frame_calls(bs)
    flt = LU.LossFilter(Tn, 8, lineload=False)
    state = np.zeros(Tn)
    flagged = 0
    for x, mask, errid in calls:
        inv, ref, flo_err, K, oob = run_frame(flt, state, x, mask, errid)
        assert np.array_equal(inv, ref) and np.array_equal(np_(flt.flo_err), flo_err)
        assert np.array_equal(np_(flt.sil_err).astype(np.float64), state)
        assert np_(flt.status).tolist() == [oob, int(ref.sum()), K, 0]
        flagged += int(ref.sum())
    assert flagged > 0 and np_(flt.status)[0] == 0 and (state > 0).sum() > 0
    flt.reset()
    assert float(flt.sil_err.abs().max()) == 0
    x, mask, errid = calls[2]
    assert not np_(flt(T(x)[..., None], T(errid), mask=T(mask)[..., None])).any()      # no history: a NaN median flags nothing
    with pytest.raises(ValueError):
        LU.LossFilter(8001, 8)


@pytest.mark.parametrize("kind", ["videos", "same", "flip"])
def test_root_sm_against_float64(kind):
    """compute_root_sm_2nd_loss against the float64 restatement.  The loss within the fp32 bound derived per triple in
    lossasm_numpy.root_sm (gamma * eps * sum |products| of the trace through acos' slope at the clamped cosine, plus the
    norm's bound); the gradient per frame within the same relative budget.  Triples whose float64 cosine lies within the bound of
    a clamp edge may fall on either side in fp32: they are left out of the gradient comparison only, and are at most 2 % (asserted
    on the restatement in test_lossasm_oracle.py).
    Observed on an MI355X, |error| / bound: loss 0.017 (videos), 0.001 (flip), < 1e-5 (same); gradient, against the worst-case
    tolerance below, 0.001.  The rounding errors of some 200 triples largely cancel, the bounds add them up; the asserted limits
    are therefore, per kind, four times the observed ratio: 0.07, 0.0046 and 5.4e-6 x the loss bound, 0.004 x the gradient
    tolerance.  The gradient tolerance is not a per-triple bound: it is the cosine's per-triple bound pushed through the slope's
    own derivative c (1 - c^2)^-3/2, times a flat 16 roundings for the products that follow -- a bound on that chain would be
    several times longer than the kernel and, after the factor above, no tighter."""
    from moda_amd import loss_utils as LU
    rtk, off = cases.root_case(kind)
    ref = ln.root_sm(rtk, off)
    r = T(rtk).requires_grad_(True)
    loss = LU.compute_root_sm_2nd_loss(r, off)
    loss.backward()
    bound = ln.root_sm_loss_bound(ref)
    err = abs(float(loss.detach()) - ref["loss"])
    print(f"root_sm[{kind}]: loss error {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3e}")
    assert err <= {"videos": 0.07, "flip": 0.0046, "same": 5.4e-6}[kind] * bound
    g = np_(r.grad).astype(np.float64)
    assert np.all(g[:, 3] == 0)
    if kind == "same":
        assert np.all(g == 0)                                         # clamped cosine, zero norm: exactly no gradient
        return
    edge = (np.abs(ref["cos"] - ref["lo"]) <= ref["cos_bound"]) | (np.abs(ref["cos"] - ref["hi"]) <= ref["cos_bound"])
    if kind == "flip":
        assert np.all(g[:, :3, :3] == 0)                              # every cosine is +-1: clamped
        edge[:] = False
    touched = np.zeros(len(rtk), bool)
    for j in ref["first"][edge]:
        touched[j:j + 3] = True
    # per element: the gradient is a sum of <= 3 triples' terms, each a product chain of ~6 fp32 operations on top of the cosine's
    # error amplified by d/dc (1 - c^2)^-1/2 = c (1 - c^2)^-3/2
    c = np.clip(ref["cos"], ref["lo"], ref["hi"])
    amp = 1 + np.abs(c) / (1 - c * c) * ref["cos_bound"] / ln.U
    scale = np.zeros(len(rtk))
    for j, a in zip(ref["first"], amp):
        scale[j:j + 3] = np.maximum(scale[j:j + 3], a)
    tol = 0.004 * 4 * (16 * ln.U) * scale[:, None, None] * np.abs(ref["grad"]).max()
    gerr = np.abs(g - ref["grad"])
    ratio = (gerr / np.maximum(tol, 1e-300))[~touched].max()
    print(f"root_sm[{kind}]: gradient max error / asserted tolerance {ratio:.3e}")
    assert np.all(gerr[~touched] <= tol[~touched])
    r2 = T(rtk).requires_grad_(True)
    LU.compute_root_sm_2nd_loss(r2, off).backward()
    assert torch.equal(r2.grad, r.grad)                               # gather form: the same bits on every run
    r3 = T(rtk[:, :3]).requires_grad_(True)                           # (T, 3, 4)
    l3 = LU.compute_root_sm_2nd_loss(r3, off)
    l3.backward()
    assert float(l3) == float(loss) and torch.equal(r3.grad, r.grad[:, :3])


def test_root_sm_without_a_triple_is_nan_and_rot_angle():
    from moda_amd import loss_utils as LU, geom_utils as GU
    rtk, _ = cases.root_case("videos")
    assert np.isnan(float(LU.compute_root_sm_2nd_loss(T(rtk[:4]), (0, 2, 4))))
    mats = rtk[:, :3, :3]
    rel = mats[:-1] @ mats[1:].transpose(0, 2, 1)
    ang = np.arccos(np.clip((np.trace(rel.astype(np.float64), axis1=1, axis2=2) - 1) / 2, -1 + 1e-4, 1 - 1e-4))
    assert np.abs(np_(GU.rot_angle(T(rel))) - ang).max() < 1e-4


# ---- the assembly ------------------------------------------------------------------------------------------------------------
def rel_err(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def gpu_rendered(rendered, grad=True):
    out = {}
    for k, v in rendered.items():
        t = T(v)
        if grad and t.dtype == torch.float32 and k not in ("sil_coarse", "sil_at_samp", "vis_at_samp"):
            t.requires_grad_(True)
        out[k] = t
    return out


ASM_VARIANTS = {
    "all": dict(),
    "loss_select0": dict(loss_select=0),
    "proj_warmup": dict(progress=0.37),                 # inside (proj_start, proj_end) = (0, 0.4): warm-up weight 0.625
    "before_warmup_steps": dict(progress=0.05),         # progress <= warmup_steps: the silhouette term is not filtered
    "no_filter_no_novp": dict(opts=dict(loss_flt=False, rm_novp=False)),
    "use_unc": dict(opts=dict(use_unc=True, s3im_loss=False)),       # (sixteen terms at the most: S3IM makes room)
}


@pytest.mark.parametrize("variant", sorted(ASM_VARIANTS))
def test_forward_loss_against_float64(variant):
    """forward_loss over N = 37 rays with every term of the table (total_wt = 1.7), value, every aux term and every dx against the
    float64 restatement of moda.py:517-768 at the tolerance of the existing total_loss test (2e-6)."""
    from moda_amd import loss_utils as LU
    rendered, opts = cases.assembly_case()
    v = dict(ASM_VARIANTS[variant])
    opts = dict(opts, **v.pop("opts", {}))
    progress, loss_select = v.get("progress", 0.5), v.get("loss_select", 1)
    N = 37
    rtk, off = cases.root_case("videos")
    errid = np.arange(N)
    Tn, S = 7, 8
    frameid = errid // S
    rendered["sil_loss_samp"][8:16] *= 64                             # frame 1 lies above ten medians
    flt = LU.LossFilter(Tn, S) if opts.get("loss_flt", True) else None
    invalid = None
    if flt is not None:
        invalid, mean, med = ln.loss_filter_line(np.zeros(Tn * S), errid, frameid,
                                                 rendered["sil_loss_samp"].reshape(-1) * np.float32(opts.get("sil_wt", 0.1)), S)
        assert invalid.any() and not invalid.all()
        assert np.abs(mean - 10 * med).min() > 1e-9 * 10 * med
    rg = gpu_rendered(rendered)
    r = T(rtk).requires_grad_(True)
    before = rg["sil_loss_samp"].detach().clone()
    total, aux = LU.forward_loss(rg, opts, loss_filter=flt, errid=None if flt is None else T(errid), frameid=None if flt is None else T(frameid),
                                 progress=progress, loss_select=loss_select, rtk_all=r, data_offset=off)
    total.backward()
    root = ln.root_sm(rtk, off)
    t_ref, aux_ref, g_ref = ln.forward_default(rendered, opts, invalid=invalid, progress=progress, loss_select=loss_select,
                                               root_sm_loss=root["loss"])
    assert torch.equal(rg["sil_loss_samp"].detach(), before)          # the stated deviation: `rendered` is not zeroed in place
    if invalid is not None:
        assert np.array_equal(np_(aux["invalid"]), invalid)
    assert abs(float(total) - t_ref) < 2e-6 * abs(t_ref)
    assert float(aux["total_loss"]) == float(total) and aux["total_loss"].dim() == 0 and aux["total_loss"].is_cuda
    for k, val in aux_ref.items():
        assert abs(float(aux[k]) - val) <= 2e-6 * abs(val), k
    for k, gr in g_ref.items():
        if k == "root_sm_loss":
            got, want = np_(r.grad), root["grad"] * float(gr)
            assert np.abs(got - want).max() < 1e-4 * np.abs(want).max()          # (its own test bounds it per element)
            continue
        got = rg[k].grad
        if np.abs(gr).max() == 0:
            assert got is None or float(got.abs().max()) == 0, k
            continue
        assert rel_err(np_(got).astype(np.float64), gr) < 2e-6, k
    assert rg["sil_coarse"].grad is None


def test_forward_loss_with_a_frame_mode_filter():
    """lineload=False through forward_loss: render_rays' (N, 1) per-ray tensors, errid with one entry per frame -- the rays are
    that many equal runs.  N = 40 rays in 5 frames of 8; frame 1 has a history and an error far above ten medians."""
    from moda_amd import loss_utils as LU
    rendered, opts = cases.assembly_case(N=40)
    opts = dict(opts, root_sm=False, lineload=False)
    rendered["sil_loss_samp"][8:16] *= 64
    Tn, bs = 9, 5
    hist = np.zeros(Tn, np.float32)
    hist[[0, 1, 2, 3]] = np.float32(0.25)
    flt = LU.LossFilter(Tn, 8, lineload=False)
    flt.sil_err.copy_(T(hist))
    errid = np.array([4, 1, 5, 6, 7], np.int64)
    w = (rendered["sil_loss_samp"] * np.float32(0.1)).reshape(bs, 8)
    inv, flo_err, med = ln.loss_filter_frame(hist.astype(np.float64), w, np.ones((bs, 8), bool), errid)
    assert inv.tolist() == [False, True, False, False, False]
    invalid = np.repeat(inv, 8)
    total, aux = LU.forward_loss(gpu_rendered(rendered, False), opts, loss_filter=flt, errid=T(errid), progress=0.5)
    assert np.array_equal(np_(aux["invalid"]), invalid)
    t_ref, aux_ref, _ = ln.forward_default(rendered, opts, invalid=invalid, progress=0.5)
    assert abs(float(total) - t_ref) < 2e-6 * abs(t_ref)
    with pytest.raises(ValueError):
        LU.forward_loss(gpu_rendered(rendered, False), opts, loss_filter=flt, errid=T(errid[:3]), progress=0.5)


def test_train_harness_default_losses_captures_and_steps():
    """TrainHarness(default_losses=True): the real step -- render_rays, the filter, rm_novp through forward_loss, backward, clip,
    AdamW -- captured into one graph and replayed; the filter's state fills, the loss is finite and agrees with the same step
    issued eagerly by a second harness.  The default path builds no filter."""
    from moda_amd.bench_support import TrainHarness
    kw = dict(N=64, S=16, B=25, precision="fp32", lr=2e-5, clip_grad=True, default_losses=True)
    a, b = TrainHarness(**kw), TrainHarness(**kw)
    a.capture(warm=1)
    assert a.graph_form == "one graph"
    b.eager_step()
    a.step()
    b.eager_step()
    torch.cuda.synchronize()
    la, lb = a.loss(), b.loss()
    assert np.isfinite(la) and np.isfinite(float(a.terms.sum()))
    # the two harnesses run the same two steps; the backward kernels of the networks add in an order that varies from run to run,
    # so after one AdamW step at lr 2e-5 the parameters agree to ~lr and the second step's loss to far better than 1e-3
    assert abs(la - lb) <= 1e-3 * abs(lb)
    for h in (a, b):
        written = h.loss_filter.sil_err != 0
        assert int(written.sum()) > 0 and not bool(written.reshape(-1, 512)[:, 4:].any())    # line i % 4 of frame i // 4
        st = np_(h.loss_filter.status)
        assert st[0] == 0 and 0 < st[2] <= 16                                                # no id out of range, <= 16 frames
    assert TrainHarness(N=64, S=16, precision="fp32").loss_filter is None


def test_forward_loss_nan_rules():
    """A mask that selects nothing gives NaN (the mean of an empty selection); a NaN in a rejected row stays NaN (`*= 0`)."""
    from moda_amd import loss_utils as LU
    rendered, opts = cases.assembly_case()
    opts = dict(opts, loss_flt=False, root_sm=False)
    r1 = dict(rendered, sil_at_samp_flo=np.zeros((37, 1), bool))
    total, aux = LU.forward_loss(gpu_rendered(r1, False), opts)
    assert np.isnan(float(total)) and np.isnan(float(aux["flo_loss"])) and np.isfinite(float(aux["img_loss"]))
    total0, _ = LU.forward_loss(gpu_rendered(r1, False), opts, loss_select=0)
    assert np.isnan(float(total0))
    Tn, S = 7, 8
    flt = LU.LossFilter(Tn, S)
    errid = np.arange(37)
    sil = rendered["sil_loss_samp"].copy()
    sil[:] = 2.0 ** -6
    sil[8:16] = 4.0                                                   # frame 1 is rejected
    img = rendered["img_loss_samp"].copy()
    sil_at = np.ones((37, 1), np.float32)
    r2 = dict(rendered, sil_loss_samp=sil, img_loss_samp=img, sil_at_samp=sil_at)
    opts2 = dict(opts, loss_flt=True)
    kw = dict(loss_filter=flt, errid=T(errid), frameid=T(errid // S), progress=0.5)
    total, aux = LU.forward_loss(gpu_rendered(r2, False), opts2, **kw)
    assert np_(aux["invalid"]).tolist() == [8 <= i < 16 for i in range(37)] and np.isfinite(float(total))
    img[9, 1] = np.nan
    total, aux = LU.forward_loss(gpu_rendered(dict(r2, img_loss_samp=img), False), opts2, **kw)
    assert np.isnan(float(aux["img_loss"])) and np.isnan(float(total)) and np.isfinite(float(aux["feat_rnd_loss"]))


@pytest.mark.parametrize("without", ["vis_loss", "frame_cyc_dis", None])
def test_total_loss_is_forward_loss_with_the_three_flags_off(without):
    """total_loss(rendered, weights) as it is called today against forward_loss with loss_flt = rm_novp = root_sm = False: every
    term, every gradient and -- where both add the terms in the same order -- the total, bit for bit.  total_loss adds its
    visibility term BEFORE the cycle term, the reference (and forward_loss) after it (moda.py:645-704), so with both terms present
    the two totals are sums of the same addends in two orders: then they agree to 2 ulp, not bitwise."""
    from moda_amd import loss_utils as LU
    rendered, _ = cases.assembly_case(N=2049)
    keys = ["img_loss_samp", "sil_loss_samp", "frnd_loss_samp", "flo_loss_samp", "feat_err", "proj_err", "vis_loss", "frame_cyc_dis",
            "sil_at_samp", "vis_at_samp", "sil_at_samp_flo"]
    rd = {k: rendered[k] for k in keys if k != without}
    opts = dict(loss_flt=False, rm_novp=False, root_sm=False, bone_loc_reg=0.0)
    ra, rb = gpu_rendered(rd), gpu_rendered(rd)
    ta, terms = LU.total_loss(ra)
    tb, aux = LU.forward_loss(rb, opts)
    ta.backward()
    tb.backward()
    names = dict(img="img_loss", sil="sil_loss", frnd="feat_rnd_loss", flo="flo_loss", feat="feat_loss", proj="proj_loss", vis="visibility_loss")
    for k, a in names.items():
        if k in terms:
            assert float(terms[k]) == float(aux[a]), k
    for k in rd:
        if ra[k].grad is not None:
            assert torch.equal(ra[k].grad, rb[k].grad), k
    if without is None:
        assert abs(float(ta) - float(tb)) <= 2 * np.spacing(np.float32(abs(float(ta))))
    else:
        assert float(ta) == float(tb)


def _total_loss_bits():
    import importlib.util
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("gen_golden_total_loss_bits", os.path.join(here, "gen_golden_total_loss_bits.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen, np.load(os.path.join(here, "g31_total_loss_bits.npz"))


@pytest.mark.parametrize("case", cases.TOTAL_LOSS_BITS_CASES, ids=lambda c: f"n{c[0]}-wide{int(c[1])}-empty{int(c[2])}")
def test_total_loss_reproduces_the_recorded_bits(case):
    """total_loss through the one assembly against tests/golden/g31_total_loss_bits.npz, which the generator beside it recorded on
    an MI355X at the last commit where total_loss had a kernel pair of its own: the total, every weighted term and every input
    gradient, BIT FOR BIT (compared as uint32, so that the NaN term and total of the `empty` cases count too).  N = 37 / 64 / 577
    (under one wave; one wave; an eight-row block + one wave row + a tail of one), k = 1 and 3, masks none / float > 0 / bool, the
    0-dim vis_loss, the zero-weight feat term, and a term with nothing selected beside terms whose gradients must not move."""
    gen, want = _total_loss_bits()
    got = gen.run_case(*case)
    name = gen.case_name(*case)
    keys = [k.split("/", 1)[1] for k in want.files if k.startswith(name + "/")]
    assert sorted(keys) == sorted(got) and len(keys) == 1 + 8 + 8
    for k in keys:
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], want[f"{name}/{k}"]), k
    if case[2]:
        total, flo = got["total"].view(np.float32), got["term_flo"].view(np.float32)
        assert np.isnan(total) and np.isnan(flo) and not got["grad_flo_loss_samp"].any()
        assert np.isfinite(got["term_img"].view(np.float32)) and got["grad_img_loss_samp"].any()


def test_total_loss_refuses_values_that_do_not_match_the_mask_rows():
    """A value tensor whose leading dimension is not the mask's row count is refused, not regrouped into mask rows."""
    from moda_amd import loss_utils as LU
    rd = {k: T(v) for k, v in cases.total_loss_bits_case(37, False, False).items()}
    rd["img_loss_samp"] = rd["img_loss_samp"].reshape(3, 37)
    with pytest.raises(ValueError):
        LU.total_loss(rd)


def test_filter_assembly_backward_captured_and_replayed():
    """Filter + root term + assembly + backward captured once into a graph and replayed three times with new inputs copied into
    the static buffers: every replay equals the eager result on a second filter fed the same sequence -- total, gradients, flags
    and the filter's accumulated state."""
    from moda_amd import loss_utils as LU
    rendered, opts = cases.assembly_case()
    N, Tn, S = 37, 7, 8
    rtk, off = cases.root_case("videos")
    rng = np.random.default_rng(41)

    def batch(i):
        errid = rng.permutation(Tn * S)[:N]
        sil = cases.dyadic(rng, (N, 1), lo=1, hi=64)
        sil[errid // S == i % Tn] *= 256
        return dict(sil_loss_samp=sil, img_loss_samp=np.abs(rng.normal(size=(N, 3))).astype(np.float32)), errid

    static = gpu_rendered(rendered)
    s_errid, s_frameid = T(np.zeros(N, np.int64)), T(np.zeros(N, np.int64))
    r = T(rtk).requires_grad_(True)
    leaves = [t for t in static.values() if t.requires_grad] + [r]
    flt_g, flt_e = LU.LossFilter(Tn, S), LU.LossFilter(Tn, S)
    kw = dict(progress=0.5, rtk_all=r, data_offset=off)

    def step(flt, rd, errid, frameid):
        for t in leaves:
            t.grad = None
        total, aux = LU.forward_loss(rd, opts, loss_filter=flt, errid=errid, frameid=frameid, **kw)
        total.backward()
        return total, aux

    def load(b, errid):
        with torch.no_grad():
            for k, v in b.items():
                static[k].copy_(T(v))
            s_errid.copy_(T(errid))
            s_frameid.copy_(T(errid // S))

    b0, e0 = batch(0)
    load(b0, e0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(LU.LossFilter(Tn, S), static, s_errid, s_frameid)       # warm-up on a filter of its own (uploads the offset table)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    for t in leaves:
        t.grad = None
    with torch.cuda.graph(graph):
        g_total, g_aux = step(flt_g, static, s_errid, s_frameid)
    live = [t for t in leaves if t.grad is not None]                # (a value no term reads, unc_pred here, gets no gradient)
    g_grads = [t.grad for t in live]
    assert len(live) >= 14
    flt_g.reset()                                                    # (capture does not run the kernels; start both from zero)
    flagged = 0
    for i in range(1, 4):
        b, e = batch(i)
        load(b, e)
        graph.replay()
        got = (float(g_total), [x.clone() for x in g_grads], g_aux["invalid"].clone(), flt_g.sil_err.clone(), flt_g.status.clone())
        e_total, e_aux = step(flt_e, static, s_errid, s_frameid)
        assert got[0] == float(e_total), i
        for a, t in zip(got[1], live):
            assert torch.equal(a, t.grad), i
        assert torch.equal(got[2], e_aux["invalid"]) and torch.equal(got[3], flt_e.sil_err) and torch.equal(got[4], flt_e.status)
        flagged += int(got[2].sum())
    assert flagged > 0 and float(flt_g.sil_err.abs().max()) > 0
