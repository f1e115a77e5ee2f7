"""float64 numpy restatements of the reference's loss stage, cited line by line: loss_filter_line (nnutils/loss_utils.py:432-445),
loss_filter (:447-476) with the state update of nnutils/moda.py:533, compute_root_sm_2nd_loss (:486-517) with rot_angle
(nnutils/geom_utils.py:1196-1205) and its hand-derived gradient, and the assembly of banmo.forward_default (moda.py:517-768).
tests/test_lossasm_oracle.py checks them against what the reference's own functions gave (tests/golden/g30_loss_assembly.npz);
tests/test_gpu_lossasm.py checks the kernels against them."""
import numpy as np

EPS = 1e-4
U = 2.0 ** -24            # fp32 unit roundoff


def loss_filter_line(sil_err, errid, frameid, values, img_size, scale_factor=10):
    """loss_utils.py:432-445.  sil_err: float64 (T * img_size,), updated in place (:438; :444 zeroes a temporary only).
    -> (invalid (N,) bool, per-frame mean (T,), median)."""
    v = np.asarray(values, np.float64).reshape(-1)                                     # :437 (fp32 values, exactly)
    sil_err[np.asarray(errid)] = v                                                     # :438 the last of a repeated id stays
    rows = sil_err.reshape(-1, img_size)                                               # :439
    with np.errstate(invalid="ignore"):
        mean = rows.sum(-1) / (1e-9 + (rows > 0).astype(float).sum(-1))                # :440
        pos = mean[mean > 0]
        med = np.median(pos) if pos.size else np.nan                                   # :441 (numpy warns and gives NaN for none)
        invalid_frame = mean > med * scale_factor                                      # :442
    return invalid_frame[np.asarray(frameid)], mean, med                               # :443


def loss_filter_frame(state, x, mask, errid, scale_factor=10):
    """loss_utils.py:447-476 and moda.py:533.  state float64 (T,), updated in place AFTER the median is taken; x, mask (bs, n).
    The reference forms flo_err in fp32 (torch); here the sums are float64 (exact for the test's dyadic inputs, as they are in
    any order of fp32 additions), the quotient fp32 as there.  -> (invalid (bs,), flo_err (bs,) fp32, median)."""
    x = np.asarray(x, np.float32).reshape(len(x), -1)
    m = np.asarray(mask).reshape(x.shape).astype(np.float32)
    pos = state[state > 0]                                                             # :455
    num = (x * m).astype(np.float64).sum(1).astype(np.float32)                         # :470
    den = np.float32(1e-9) + m.astype(np.float64).sum(1).astype(np.float32)            # :471
    with np.errstate(invalid="ignore", divide="ignore"):
        flo_err = (num / den).astype(np.float32)
        med = np.median(pos) if pos.size else np.nan
        invalid = flo_err.astype(np.float64) > med * scale_factor                      # :475
    state[np.asarray(errid)] = flo_err                                                 # moda.py:533
    return invalid, flo_err, med


def triples(data_offset):
    """First frames of the consecutive triples of every video (loss_utils.py:492-498)."""
    out = []
    for a, b in zip(data_offset[:-1], data_offset[1:]):
        out += list(range(a, b - 2))
    return np.asarray(out, np.int64)


def root_sm(rtk, data_offset, clamp32=True):
    """loss_utils.py:486-517 and its gradient, in float64 whatever rtk's type.  -> dict(loss, grad (T, rows, 4), cos (M,) unclamped, angle, trn, first (M,),
    and per triple the fp32 error bounds `cos_bound`, `trn_bound` of a kernel that forms the same products in fp32)."""
    r = np.asarray(rtk, np.float64)
    j = triples(data_offset)
    M = len(j)
    if M == 0:
        return dict(loss=np.nan, grad=np.zeros_like(r), first=j)
    R0, R1, R2 = r[j, :3, :3], r[j + 1, :3, :3], r[j + 2, :3, :3]
    t0, t1, t2 = r[j, :3, 3], r[j + 1, :3, 3], r[j + 2, :3, 3]
    A = R0 @ R1.transpose(0, 2, 1)                                                     # :500
    B = R1 @ R2.transpose(0, 2, 1)                                                     # :501
    tr = (A * B).sum((1, 2))                                                           # trace of A B^T (:506, geom_utils.py:1202)
    cos = (tr - 1) / 2
    lo, hi = -1 + EPS, 1 - EPS                                                         # :1201-1203
    if clamp32:                               # on an fp32 tensor torch clamps at the bounds rounded to fp32
        lo, hi = float(np.float32(lo)), float(np.float32(hi))
    angle = np.arccos(np.clip(cos, lo, hi))                                            # :1203-1204
    d = (t0 - t1) - (t1 - t2)                                                          # :503-507
    trn = np.sqrt((d * d).sum(-1))                                                     # :514
    loss = (angle.mean() * 1e-1 + trn.mean()) * 0.1                                    # :512-516
    # gradient: acos' = -1 / sqrt(1 - c^2) where lo <= c <= hi (torch's clamp passes AT the bounds), d cos = <dA, B> / 2 + ...
    inside = (cos >= lo) & (cos <= hi)
    with np.errstate(divide="ignore", invalid="ignore"):
        gc = np.where(inside, -1.0 / np.sqrt(1 - np.clip(cos, lo, hi) ** 2), 0.0) * 0.5 * (0.1 * 1e-1 / M)
        gt = np.where(trn > 0, (0.1 / M) / np.where(trn > 0, trn, 1), 0.0)
    g = np.zeros_like(r)
    dA, dB = gc[:, None, None] * B, gc[:, None, None] * A
    np.add.at(g, (j, slice(0, 3), slice(0, 3)), dA @ R1)                               # A = R0 R1^T
    np.add.at(g, (j + 1, slice(0, 3), slice(0, 3)), dA.transpose(0, 2, 1) @ R0 + dB @ R2)
    np.add.at(g, (j + 2, slice(0, 3), slice(0, 3)), dB.transpose(0, 2, 1) @ R1)
    gd = gt[:, None] * d
    np.add.at(g, (j, slice(0, 3), 3), gd)
    np.add.at(g, (j + 1, slice(0, 3), 3), -2 * gd)
    np.add.at(g, (j + 2, slice(0, 3), 3), gd)
    # fp32 error bounds per triple.  An entry of A or B is a 3-term fp32 dot product: error <= gamma_3 * sum |products|.  The
    # trace is 9 products of such entries, added in fp32 (8 additions, first-order gamma_9 with the product's rounding), so
    #   |d tr| <= sum_ik (eA_ik |B_ik| + |A_ik| eB_ik) + gamma_9 * sum_ik |A_ik B_ik|,   gamma_n = n U / (1 - n U);
    # (tr - 1) / 2 adds one rounding of the difference (the halving is exact).
    g3, g9 = 3 * U / (1 - 3 * U), 9 * U / (1 - 9 * U)
    absA = np.abs(R0) @ np.abs(R1).transpose(0, 2, 1)
    absB = np.abs(R1) @ np.abs(R2).transpose(0, 2, 1)
    tr_bound = (g3 * absA * np.abs(B) + np.abs(A) * g3 * absB).sum((1, 2)) + g9 * np.abs(A * B).sum((1, 2))
    cos_bound = tr_bound / 2 + U * np.abs(tr - 1) / 2
    # the norm: d has two roundings per difference level (3 subtractions of fp32 inputs): |dd_c| <= 2U (|t0-t1| + |t1-t2|) + U |d_c|;
    # sqrt(sum of 3 squares) in fp32 adds gamma_4 relative plus the half-ulp of the square root
    dd = 2 * U * (np.abs(t0 - t1) + np.abs(t1 - t2)) + U * np.abs(d)
    trn_bound = np.sqrt((dd * dd).sum(-1)) + (4 * U / (1 - 4 * U)) * trn + U * trn
    return dict(loss=loss, grad=g, cos=cos, angle=angle, trn=trn, first=j, lo=lo, hi=hi, cos_bound=cos_bound, trn_bound=trn_bound)


def root_sm_loss_bound(ref):
    """fp32 error bound of the loss: every angle through acos' slope at the (clamped) cosine, plus acosf's own error (2 ulp of
    an angle <= pi), every norm by its bound, means in float64, three fp32 roundings of the final combination."""
    c = np.clip(ref["cos"], ref["lo"], ref["hi"])
    slope = 1.0 / np.sqrt(1 - c * c)
    e_ang = slope * ref["cos_bound"] + 2 * U * np.maximum(ref["angle"], 1e-30)
    return 0.1 * (0.1 * e_ang.mean() + ref["trn_bound"].mean()) + 4 * U * abs(ref["loss"])


# ---- the assembly (moda.py:517-768) ---------------------------------------------------------------------------------------------
DEFAULTS = dict(lineload=False, use_unc=False, img_size=512, warmup_steps=0.4, freeze_proj=False, proj_start=0.0, proj_end=0.2,
                use_embed=True, use_proj=True, use_corresp=True, total_wt=1.0, sil_wt=0.1, img_wt=0.1, feat_wt=0.0, use_corr=False,
                corr_wt=0.01, frnd_wt=1.0, proj_wt=0.02, flow_wt=1.0, cyc_wt=1.0, root_sm=True, eikonal_wt=0.0, loss_flt=True,
                rm_novp=True, s3im_loss=False, s3im_wt=0.01)


def forward_default(rendered, opts, invalid=None, progress=0.0, loss_select=1, root_sm_loss=None, with_grad=True):
    """moda.py:517-768 over float64 copies of `rendered` (numpy arrays, per-ray tensors (N, k) or (N,)); `invalid` (N,) bool as the
    filter returned it (None: loss_flt off).  -> (total, aux dict, grads dict: d total / d rendered[key] for every value key).
    The gradient is written out by hand: every term is w * sum(sel * keep * scale * x) / count(sel)."""
    o = dict(DEFAULTS)
    o.update(opts)
    R = {k: np.asarray(v, np.float64) if np.asarray(v).dtype.kind == "f" else np.asarray(v) for k, v in rendered.items()}
    N = R["sil_at_samp"].reshape(-1).shape[0]
    sil = R["sil_at_samp"].reshape(N) > 0
    vis = R["vis_at_samp"].reshape(N) > 0
    keep = np.ones(N) if invalid is None else np.where(np.asarray(invalid).reshape(N), 0.0, 1.0)
    scale = R["sil_coarse"].reshape(N) if o["rm_novp"] else np.ones(N)                # :548, :570, :582, :604, :614
    aux, grads = {}, {}
    state = dict(total=0.0, chain=[])                                                  # chain: (key, per-element coefficient array)

    def term(key, wt, sel, use_keep, use_scale):
        x = R[key].reshape(N, -1)
        with np.errstate(invalid="ignore"):
            rowc = (keep if use_keep else np.ones(N)) * (scale if use_scale else np.ones(N))
            vals = (x * (keep if use_keep else np.ones(N))[:, None]) * (scale if use_scale else np.ones(N))[:, None]   # `*= 0`: NaN stays
            cnt = sel.sum() * x.shape[1]
            mean = vals[sel].sum() / cnt if cnt else np.nan                            # x[mask].mean()
        coef = np.where(sel, rowc, 0.0)[:, None] * np.ones_like(x) * (wt / cnt if cnt else np.nan)
        return wt * mean, coef

    def add(key, value, coef, carry=1.0):
        state["total"] = state["total"] * carry + value
        state["chain"] = [(k, c * carry) for k, c in state["chain"]] + [(key, coef)]

    flt = invalid is not None
    v, c = term("img_loss_samp", o["img_wt"], sil, flt, o["rm_novp"])                  # :540-549
    aux["img_loss"] = v
    add("img_loss_samp", v, c)
    v, c = term("sil_loss_samp", o["sil_wt"], vis, flt and progress > o["warmup_steps"], False)   # :535-536, :550-551
    aux["sil_loss"] = v
    add("sil_loss_samp", v, c)
    if o["s3im_loss"]:                                                                 # :560-563
        aux["s3im_loss"] = o["s3im_wt"] * float(R["s3im_loss"])
        add("s3im_loss", aux["s3im_loss"], np.full(R["s3im_loss"].shape, o["s3im_wt"]))
    v, c = term("frnd_loss_samp", o["frnd_wt"], sil, flt, o["rm_novp"])                # :566-574
    aux["feat_rnd_loss"] = v
    add("frnd_loss_samp", v, c)
    if o["use_corresp"]:                                                               # :577-594
        v, c = term("flo_loss_samp", 2 * o["flow_wt"], R["sil_at_samp_flo"].reshape(N).astype(bool), flt, o["rm_novp"])
        aux["flo_loss"] = v
        add("flo_loss_samp", v, c, 0.0 if loss_select == 0 else 1.0)                   # :590-593 total*0. + flo
    if o["use_embed"]:                                                                 # :597-618
        v, c = term("feat_err", o["feat_wt"], sil, flt, o["rm_novp"])
        aux["feat_loss"] = v
        add("feat_err", v, c)
        if o["use_corr"]:
            v, c = term("corr_err", o["corr_wt"], sil, flt, o["rm_novp"])
            aux["corr_loss"] = v
            add("corr_err", v, c)
    if o["use_proj"]:                                                                  # :622-642
        v, c = term("proj_err", o["proj_wt"], sil, flt, False)
        aux["proj_loss"] = v
        add("proj_err", v, c)
        if o["freeze_proj"] and o["proj_start"] < progress < o["proj_end"]:            # :633-639
            w = (progress - o["proj_start"]) / (o["proj_end"] - o["proj_start"])
            w = float(np.clip((w - 0.8) * 5, 0, 1))
            add("proj_err", 10 * v * (1 - w), c * 10 * (1 - w), w)
    for key, wt, name in (("frame_cyc_dis", o["cyc_wt"], "cyc_loss"), ("elastic_loss", 1e-3, "elastic_loss"),
                          ("dis_reg", 1.0, None), ("dis_reg_forward", 1.0, None)):     # :645-664
        if key in R and (key != "elastic_loss" or "frame_cyc_dis" in R):
            m = R[key].mean()
            if name:
                aux[name] = m if name == "cyc_loss" else wt * m                        # :650 logs the unweighted cycle loss
            add(key, wt * m, np.full(R[key].shape, wt / R[key].size))
    if o["root_sm"]:                                                                   # :667-670
        aux["root_sm_loss"] = root_sm_loss
        add("root_sm_loss", root_sm_loss, np.ones(()))
    if o["eikonal_wt"] > 0:                                                            # :673-678
        aux["ekl_loss"] = o["eikonal_wt"] * float(R["eikonal_loss"])
        add("eikonal_loss", aux["ekl_loss"], np.full((), o["eikonal_wt"]))
    if "vis_loss" in R:                                                                # :701-704
        aux["visibility_loss"] = 0.01 * R["vis_loss"].mean()
        add("vis_loss", aux["visibility_loss"], np.full(R["vis_loss"].shape, 0.01 / R["vis_loss"].size))
    if o["use_unc"]:                                                                   # :707-720
        img = R["img_loss_samp"].reshape(N, -1) * o["img_wt"]                          # :540
        if flt:
            img = img * keep[:, None]                                                  # :544
        target = R["sil_at_samp"].reshape(N) * img.mean(-1)                            # :710, detached at :717
        diff = target - R["unc_pred"].reshape(N)
        aux["unc_loss"] = (diff ** 2).mean()
        add("unc_pred", aux["unc_loss"], (-2 * diff / N).reshape(R["unc_pred"].shape))
    total = state["total"] * o["total_wt"]                                             # :762
    aux["total_loss"] = total
    for key, coef in state["chain"]:
        g = coef * o["total_wt"]
        g = g.reshape(R[key].shape) if key in R else g
        grads[key] = grads[key] + g if key in grads else g
    return total, aux, grads
