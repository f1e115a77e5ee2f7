"""The per-ray loss heads `inference_deform` calls behind compositing, with the reference's names and argument
meaning (nnutils/loss_utils.py): visibility_loss :125-149, compute_pts_exp :165-175, feat_match_loss :176-210,
kp_reproj_loss :212-222, kp_reproj :224-270, feat_match :273-405, and the eikonal regulariser of the canonical density
(nerf_gradient :15-47, compute_gradients_sdf :48-71, eikonal_loss :73-104).  Every arithmetic node is a HIP kernel behind an
autograd Function (moda_amd/autograd.py), so the same code serves the no-grad and the training route.

Random tensors the reference draws inside these functions can be injected through `rng` (dict):
'feat_noise' (1, 20^3, 3) standard normals (loss_utils.py:306), 'vis_neg_rand' (1, N*S, 3) uniforms (:137),
'eik_inds' (1000,) ray indices (:81-84), 's3im_perms' (9, 1024) the permutations of S3IM (:683)."""
import numpy as np
import torch

from . import _lib as L
from . import autograd as A


def compute_pts_exp(pts_prob, pts):
    """loss_utils.py:165-175: pts (..., ndepth, 3), pts_prob (..., ndepth) -> (..., 3) expectation."""
    nd = pts_prob.shape[-1]
    return A.PtsExpFn.apply(pts_prob.reshape(-1, nd), pts.reshape(-1, nd, 3))


def _bound_key(bound):
    """(values, dtype) of the caller's `bound`, as the reference indexes it (bound[0..2])."""
    if torch.is_tensor(bound):
        bound = bound.detach().cpu().numpy()
    b = np.asarray(bound).reshape(-1)[:3]
    if b.dtype.kind != "f":
        b = b.astype(np.float64)
    return b, (tuple(float(v) for v in b), b.dtype.str)


def _query_grid(bound, grid_size):
    """loss_utils.py:290-294: query[i,j,k] = (x_i, y_j, z_k) on linspace(-bound, bound, grid_size), flattened.
    The reference's expression `np.linspace(-bound[c], bound[c], grid_size).astype(np.float32)` is evaluated AS IT STANDS, on
    scalars of the caller's dtype: with a float32 `bound` (MoDA's obj_bound) NumPy >= 2 computes the nodes in float32 arithmetic
    (NEP 50: result_type(float32, float32, python float) is float32), NumPy 1.x in float64 -- a few nodes then differ by one
    float32 ulp, which the 2^9 frequency of the positional encoding turns into 8e-4 of nerf_feat's first-layer weight gradient
    (found by the float64-truth fixtures of round 5; python floats were passed here before).  Mirroring the expression keeps
    this function equal to the reference in whatever environment both run."""
    b, _ = _bound_key(bound)
    ax = [np.linspace(-b[c], b[c], grid_size).astype(np.float32) for c in range(3)]
    g = np.empty((grid_size, grid_size, grid_size, 3), np.float32)
    g[..., 0] = ax[0][:, None, None]
    g[..., 1] = ax[1][None, :, None]
    g[..., 2] = ax[2][None, None, :]
    return g.reshape(-1, 3)


def feat_grid_query(bound, device, grid_size=20, is_training=True, rng=None):
    """The lattice feat_match evaluates nerf_feat on (loss_utils.py:290-306): linspace(-bound, bound, 20)^3, jittered by
    0.05 * bound * randn in training (rng['feat_noise'] injects the draw)."""
    b, key = _bound_key(bound)
    query = L.const_tensor(("feat_grid", key, grid_size), device, lambda: _query_grid(bound, grid_size))   # :290-301
    if is_training:                                                                   # :304-306
        nz = (rng or {}).get('feat_noise')
        nz = torch.randn((1,) + tuple(query.shape), device=device) if nz is None else L.dev(nz)
        scale = L.const_tensor(("bound", key), device, lambda: np.asarray(b, np.float32))
        out = torch.empty_like(query)
        L.call("moda_affine3", L.ptr(L.dev(nz).reshape(query.shape)), L.ptr(query), L.ptr(scale), 0.05, None, query.shape[0],
               L.ptr(out), L.stream())                                                # query + (randn * bound) * 0.05, one launch
        query = out
    return query


def feat_match(nerf_feat, embedding_xyz, feats, bound, grid_size=20, use_corr=True, use_ot=False, is_training=True,
               init_pts=None, rt_entropy=False, rng=None, grid=None):
    """loss_utils.py:273-405: feats (n, 16) pixel features -> (pts_pred (n,3), corr_err).
    grid = (query (G,3), vol (G,16)): the lattice and nerf_feat's output on it, when the caller has already evaluated them
    (render_rays' training route does, in the same network call as the rendered features)."""
    if init_pts is not None:
        return _feat_match_local(nerf_feat, embedding_xyz, feats, bound, grid_size, use_corr, use_ot, init_pts, rt_entropy)
    f = L.dev(feats).reshape(-1, feats.shape[-1])
    dev = f.device
    fn = A.NormalizeFn.apply(f)                                                       # :287
    if grid is not None:
        query, vol = grid
    else:
        query = feat_grid_query(bound, dev, grid_size, is_training, rng)
        train = torch.is_grad_enabled() and (f.requires_grad or any(p.requires_grad for p in nerf_feat.parameters()))
        if train:
            vol = nerf_feat.train_forward(query, embedding_xyz)                       # :311-313
        else:
            vol = nerf_feat.fused(query, n_freq=embedding_xyz.N_freqs, alpha=embedding_xyz.alpha)
    vn = A.NormalizeFn.apply(vol)                                                     # :315
    if use_ot:                                                                        # :338-374
        kappa = torch.full((1,), 1.0 / A.SINKHORN_TEMP, device=dev)
    else:                                                                             # :331-332, :376
        kappa = nerf_feat.beta.abs() + 1e-9
    pts_pred, prob = A.FeatMatchFn.apply(fn, vn, query, kappa, bool(use_ot), bool(use_corr or rt_entropy))   # :389
    corr_err = 0
    if use_corr:                                                                      # :386-391
        tt = A.LinearFn.apply(prob, prob, None, 0)                                    # prob prob^T, (n, n)
        corr_err = (tt - torch.eye(tt.shape[0], device=dev)).norm(2, -1)
    if rt_entropy:                                                                    # :397-402 normalised matching entropy
        match_unc = (-prob * prob.clamp(1e-9, 1 - 1e-9).log()).sum(1)[:, None] / float(np.log(grid_size ** 3))
        return pts_pred, match_unc, corr_err
    return pts_pred, corr_err


def _feat_match_local(nerf_feat, embedding_xyz, feats, bound, grid_size, use_corr, use_ot, init_pts, rt_entropy):
    """feat_match with `init_pts` (loss_utils.py:297-300, 322-331): every pixel n matches against a lattice of its own,
    query + init_pts[n] -- n * grid_size^3 network evaluations (one fused launch per chunk of pixels), the per-pixel matrix
    exp((<vol[n, g], feats[n]> - 1) kappa) (moda_match_matrix_rows) and the SAME library tail as the shared-lattice form
    (moda_match_sweep x 40, moda_match_expect, moda_match_prob; round 5 -- it was torch arithmetic before).  No caller in the
    reference uses this option (scripts/visualize/match.py:101, loss_utils.py:197): inference only, no lattice jitter (:304)."""
    L.no_grad_only(feats, init_pts, *nerf_feat.parameters())
    f = L.dev(feats).reshape(-1, feats.shape[-1])
    dev = f.device
    fn = A.NormalizeFn.apply(f)                                                       # :287
    base = L.const_tensor(("feat_grid", _bound_key(bound)[1], grid_size), dev, lambda: _query_grid(bound, grid_size))
    init = L.dev(init_pts).reshape(-1, 3)
    query = base[None] + init[:, None]                                                # :298 (n, G, 3)
    n, G = query.shape[0], query.shape[1]
    use_ot = bool(use_ot)
    kappa = torch.full((1,), 1.0 / A.SINKHORN_TEMP, device=dev) if use_ot else (nerf_feat.beta.abs() + 1e-9).reshape(1)   # :340 / :331-332
    Kmat = torch.empty((n, G), device=dev)
    step = max(1, (1 << 22) // G)                                                     # pixels per network launch (~4 M points)
    for j in range(0, n, step):
        vol = nerf_feat.fused(query[j:j + step].contiguous(), n_freq=embedding_xyz.N_freqs, alpha=embedding_xyz.alpha)   # :325-326
        vn = A.NormalizeFn.apply(vol.reshape(-1, vol.shape[-1]))                      # :328
        m = min(step, n - j)
        # K[n, g] = exp((<vol[n, g], feats[n]> - 1) kappa): the Sinkhorn kernel of :340 / the shifted softmax numerator of :337, 376
        L.call("moda_match_matrix_rows", L.ptr(fn[j:j + m]), L.ptr(vn), m, G, f.shape[1], L.ptr(kappa), L.ptr(Kmat[j:j + m]), L.stream())
    b = None
    if use_ot:                                                                        # :338-374: the sweeps of the shared-lattice form
        KmatT = Kmat.t().contiguous()
        a_t = torch.full((n,), 1.0 / n, device=dev)
        b = torch.empty((G,), device=dev)
        for _ in range(A.SINKHORN_ITERS):
            L.call("moda_match_sweep", L.ptr(KmatT), G, n, L.ptr(a_t), 1, 1.0 / G, None, L.ptr(b), 0, L.stream())
            a_n = torch.empty_like(a_t)
            L.call("moda_match_sweep", L.ptr(Kmat), n, G, L.ptr(b), 1, 1.0 / n, None, L.ptr(a_n), 0, L.stream())
            a_t = a_n
    # expectation over the shared base lattice, then the pixel's own offset: sum_g prob (base_g + init_n) = E[base] + init_n (:395)
    pred = torch.empty((n, 3), device=dev)
    rowsum = torch.empty((n,), device=dev)
    L.call("moda_match_expect", L.ptr(Kmat), L.ptr(b), L.ptr(base), n, G, L.ptr(pred), L.ptr(rowsum), 0, L.stream())
    pts_pred = pred + init
    corr_err = 0
    prob = None
    if use_corr or rt_entropy:
        prob = torch.empty((n, G), device=dev)
        L.call("moda_match_prob", L.ptr(Kmat), L.ptr(b), L.ptr(rowsum), n, G, L.ptr(prob), 0, L.stream())
    if use_corr:                                                                      # :386-391
        tt = A.LinearFn.apply(prob, prob, None, 0)                                    # prob prob^T (library GEMM)
        corr_err = (tt - torch.eye(n, device=dev)).norm(2, -1)
    if rt_entropy:
        match_unc = (-prob * prob.clamp(1e-9, 1 - 1e-9).log()).sum(1)[:, None] / float(np.log(grid_size ** 3))
        return pts_pred, match_unc, corr_err
    return pts_pred, corr_err


def feat_match_loss(nerf_feat, embedding_xyz, feats, pts, pts_prob, bound, use_corr=True, use_ot=False,
                    is_training=True, rng=None, grid=None):
    """loss_utils.py:176-210 -> (pts_pred (...,3), pts_exp (...,3), feat_err (...,1), corr_err)."""
    base = tuple(feats.shape[:-1])
    pts_exp = compute_pts_exp(pts_prob, pts)                                          # :193
    pts_pred, corr_err = feat_match(nerf_feat, embedding_xyz, feats, bound, grid_size=20, use_corr=use_corr,
                                    use_ot=use_ot, is_training=is_training, rng=rng, grid=grid)  # :196-197
    feat_err = A.RowDistFn.apply(pts_pred, pts_exp)                                   # :200 (pts_pred - pts_exp).norm(2, -1)
    if use_corr:
        corr_err = corr_err.view(base + (1,))                                         # :207-208
    return pts_pred.view(base + (3,)), pts_exp.view(base + (3,)), feat_err.view(base + (1,)), corr_err


def forward_warp(pts, models, embedding_xyz, bone_rts, dskin=None, dskin_bns=False, pts_tf=None):
    """Canonical -> observed warp of pts (N,n,3) with the rest-pose skinning field (gauss_mlp_skinning with
    rest_pose_code + neu_dbs backward=False; rendering.py:351-352, loss_utils.py:250-254).
    `dskin`: nerf_skin's output at exactly these points with the rest-pose code, when the caller already has it (the
    reference re-evaluates the same network on the same inputs for the cycle, target and dense-target warps,
    rendering.py:330, :351, :356); (N,n,B), or (N,B,n) with dskin_bns.  `pts_tf`: the points the transform is applied to
    when a residual field displaces them first (pts + nerf_dis(pts, rest), geom_utils.py:420-425)."""
    bones_rst = L.dev(models['bones_rst'])
    B = bones_rst.shape[-2]
    N, n_s = pts.shape[0], pts.shape[1]
    nerf_skin = models['nerf_skin'] if 'nerf_skin' in models.keys() else None
    rest = models['rest_pose_code'].weight.reshape(1, -1)
    leaves = [pts, bones_rst, bone_rts, models['skin_aux'], rest] + ([] if nerf_skin is None else list(nerf_skin.parameters()))
    if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in leaves + [dskin, pts_tf]):
        ds = dskin
        if ds is None and nerf_skin is not None:
            ds = nerf_skin.train_forward(pts, embedding_xyz, code=A.fanned(models['rest_pose_code'].weight).reshape(1, -1))
        rts = L.dev(bone_rts).reshape(-1, B, 8)
        if rts.shape[0] == 0 or N % rts.shape[0]:
            raise ValueError(f"bone_rts: {rts.shape[0]} transform sets do not divide {N} rays")
        if rts.shape[0] != N:                          # per-frame rows under autograd: expanded (gradients sum per frame)
            rts = A.ExpandRowsFn.apply(rts.reshape(rts.shape[0], B * 8), N // rts.shape[0]).reshape(N, B, 8)
        return A.WarpFn.apply(A.bone_prep(A.fanned(bones_rst).reshape(1, B, 10)), rts, pts, ds,
                              A.fanned(L.dev(models['skin_aux'])), None, pts_tf)[0]
    from .geom_utils import warp                      # no graph wanted: the fused inference kernels
    ds, bns = dskin, dskin_bns
    if ds is None and nerf_skin is not None:
        ds = nerf_skin.fused(pts, n_freq=embedding_xyz.N_freqs, alpha=embedding_xyz.alpha, code=L.dev(rest), out_tr_S=n_s)
        bns = True
    # frame-grouped layout (rays['rays_per_frame']): bone_rts may hold one row per frame of k consecutive rays
    n_sets = L.dev(bone_rts).reshape(-1, B * 8).shape[0]
    if n_sets == 0 or N % n_sets:
        raise ValueError(f"bone_rts: {n_sets} transform sets do not divide {N} rays")
    return warp(bones_rst, bone_rts, pts, ds, models['skin_aux'], backward=False, dskin_bns=bns, pts_tf=pts_tf,
                rays_per_set=N // n_sets)[0]


def kp_reproj(pts_pred, models, embedding_xyz, rays, to_target=False, neudbs=True):
    """loss_utils.py:224-270: canonical points (...,3) -> pixel coordinates (N,1,2) in the (target) frame."""
    if not neudbs:
        raise NotImplementedError("linear blend skinning: MoDA runs neudbs (moda.py:72-73)")
    pts = pts_pred.reshape(-1, 1, 3)
    N = pts.shape[0]
    rtk = L.dev(rays['rtk_vec_target'] if to_target else rays['rtk_vec']).reshape(N, 21)
    if 'bones' in models.keys():
        pts = forward_warp(pts, models, embedding_xyz, rays['bone_rts_target'] if to_target else rays['bone_rts'])
    return A.ProjectFn.apply(pts, rtk)[..., :2]


def kp_reproj_loss(pts_pred, xys, models, embedding_xyz, rays, neudbs=True):
    """loss_utils.py:212-222 -> reprojection distance (...,1)."""
    xy = kp_reproj(pts_pred, models, embedding_xyz, rays, neudbs=neudbs)
    err = A.RowDistFn.apply(xy, L.dev(xys).reshape(-1, 1, 2))            # (xys - xy).norm(2, -1)
    return err.view(tuple(pts_pred.shape[:-1]) + (1,))


def visibility_loss(mlp, embed, xyz_pos, w_pos, bound, chunk, rng=None):
    """loss_utils.py:125-149: xyz_pos (N,S,3) with visibilities w_pos (N,S); negatives uniform in the bound."""
    xyz_pos = L.dev(xyz_pos).detach()
    w_pos = L.dev(w_pos).detach()
    dev = xyz_pos.device
    nsample = w_pos.shape[0] * w_pos.shape[1]
    bt = tuple(float(b) for b in np.asarray(bound).reshape(-1)[:3])
    r = (rng or {}).get('vis_neg_rand')
    r = torch.rand(1, nsample, 3) if r is None else r                                 # :137 (the reference draws on the CPU)
    bnd2 = L.const_tensor(("bound*2", bt), dev, lambda: np.asarray(bt, np.float32) * np.float32(2))
    nbnd = L.const_tensor(("-bound", bt), dev, lambda: -np.asarray(bt, np.float32))
    xyz_neg = torch.empty((1, nsample, 3), device=dev)
    L.call("moda_affine3", L.ptr(L.dev(r.to(dev)).reshape(nsample, 3)), None, L.ptr(bnd2), 1.0, L.ptr(nbnd), nsample,
           L.ptr(xyz_neg), L.stream())                                                # (rand * 2) * bound - bound (:138), one launch
    train = torch.is_grad_enabled() and any(p.requires_grad for p in mlp.parameters())

    def logits(x):
        if train:
            return mlp.train_forward(x, embed)[..., 0]
        return mlp.fused(x, n_freq=embed.N_freqs, alpha=embed.alpha, with_sigma=False, sigmoid=False)[..., 0]

    # negatives and positives through ONE evaluation of the network (the reference makes two, :139 and :144; same arithmetic
    # per point): one forward / backward launch chain and one set of weight-gradient GEMMs instead of two
    both = logits(torch.cat([xyz_neg.reshape(-1, 3), xyz_pos.reshape(-1, 3)], 0))
    return A.VisPairLossFn.apply(both, w_pos, nsample)                                 # :140 + :145


def masked_mean(x, mask):
    """`x[mask].mean()` as the reference's loss assembly writes it (moda.py:540-640), without the boolean gather's host sync:
    x (N, k) | (N,), mask (N, 1) | (N,) bool or float (non-zero = selected).  NaN when nothing is selected, as the reference's
    mean of an empty selection.  One term of weight 1 of the loss assembly (moda_loss_assembly), one launch each way: the sum is
    formed in the assembly's order (per lane over the rows lane, lane + 64, ..., then one wave butterfly), and the rows are
    SELECTED, not multiplied by the mask -- a NaN or inf in an unselected row does not reach the mean, as in `x[mask]`."""
    kind = "bool" if mask.dtype == torch.bool else "!=0"
    return A.LossAssemblyFn.apply([(1.0, mask, kind, None, None, 1.0)], 1.0, x)[0]


# the weights of moda.py's loss assembly (flags moda.py:153-162; the visibility term's 0.01 is written out at :702)
LOSS_WEIGHTS = dict(img_wt=0.1, sil_wt=0.1, frnd_wt=1.0, flow_wt=1.0, feat_wt=0.0, proj_wt=0.02, cyc_wt=1.0, vis_wt=0.01)
LOSS_TERMS = ("img", "sil", "frnd", "flo", "feat", "proj", "vis", "cyc")


def total_loss(rendered, weights=None):
    """The loss assembly of banmo.forward_default over render_rays' result dict (moda.py:540-705) in a REDUCED configuration:
    loss_flt, rm_novp and root_sm off and no warm-up branch -- the reference itself trains with all three on (moda.py:164-168;
    `forward_loss` below is that assembly).  img_wt * img_loss_samp[sil > 0].mean() + sil_wt * sil_loss_samp[vis > 0].mean() +
    frnd_wt * frnd_loss_samp[sil > 0].mean() + 2 flow_wt * flo_loss_samp[sil_at_samp_flo].mean() + feat_wt * feat_err[sil > 0]
    .mean() + proj_wt * proj_err[sil > 0].mean() + vis_wt * vis_loss + cyc_wt * frame_cyc_dis.mean() -- the terms whose keys
    the dict holds, as ONE launch forward and one backward instead of ~55 eager ops with a boolean gather (and its host sync)
    per term: the assembly `forward_loss` runs (moda_loss_assembly) without scale, drop, carry and total_wt, in this function's
    own term order (vis before cyc).  -> (total, {term name: weighted term, detached}).  moda.py itself cannot be imported here
    (absl, mcubes ...): restated from the cited lines, checked against the plain-torch restatement (oracle/torch_ref.py)."""
    w = dict(LOSS_WEIGHTS)
    w.update(weights or {})
    sil = rendered.get("sil_at_samp")
    plan = [("img", "img_loss_samp", w["img_wt"], sil, ">0"), ("sil", "sil_loss_samp", w["sil_wt"], rendered.get("vis_at_samp"), ">0"),
            ("frnd", "frnd_loss_samp", w["frnd_wt"], sil, ">0"),
            ("flo", "flo_loss_samp", 2.0 * w["flow_wt"], rendered.get("sil_at_samp_flo"), "bool"),
            ("feat", "feat_err", w["feat_wt"], sil, ">0"), ("proj", "proj_err", w["proj_wt"], sil, ">0"),
            ("vis", "vis_loss", w["vis_wt"], None, None), ("cyc", "frame_cyc_dis", w["cyc_wt"], None, None)]
    names, spec, xs = [], [], []
    for name, key, wt, mask, kind in plan:
        if key in rendered:
            names.append(name)
            spec.append((wt, mask, kind, None, None, 1.0))
            xs.append(rendered[key])
    total, rest = A.LossAssemblyFn.apply(spec, 1.0, *xs)
    return total, {n: rest[i] for i, n in enumerate(names)}


# ---- the stage between render_rays and backward() with the reference's own flags (loss_flt, rm_novp, root_sm) ------------------
def _ids(t, device, what):
    """errid / frameid as the kernels read them: a contiguous int32 or int64 device tensor.  A host tensor is copied (once per
    call: not capturable -- keep the ids on the device, as pixel_lines.set_input leaves them)."""
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.asarray(t))
    if t.dtype not in (torch.int32, torch.int64):
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise TypeError(f"{what} must be an integer tensor, got {t.dtype}")
        t = t.to(torch.int64)
    if t.device != device:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{what} lies on {t.device}: copying it is not capturable, pass a device tensor")
        t = t.to(device)
    return t.reshape(-1).contiguous()


def _filter_ws(num_frames, img_size, device):
    nbytes = L.load().moda_loss_filter_ws_bytes(num_frames, img_size)
    return torch.full((nbytes,), 255, dtype=torch.uint8, device=device)        # every owner word -1: no slot claimed


def _filter_line(values, errid, frameid, sil_err, num_frames, img_size, scale_factor, ws, invalid, status):
    dev = sil_err.device
    v = L.dev(values.detach()).reshape(-1)
    e, f = _ids(errid, dev, "errid"), _ids(frameid, dev, "frameid")
    if e.numel() != v.numel() or f.numel() != v.numel():
        raise ValueError(f"loss_filter_line: {v.numel()} values, {e.numel()} errid, {f.numel()} frameid")
    if invalid is None:
        invalid = torch.empty((v.numel(),), dtype=torch.bool, device=dev)
    L.call("moda_loss_filter_line", L.ptr(v), L.ptr(e), int(e.dtype == torch.int64), L.ptr(f), int(f.dtype == torch.int64), v.numel(),
           L.ptr(sil_err), num_frames, img_size, float(scale_factor), L.ptr(ws), L.ptr(invalid), L.ptr(status), L.stream())
    return invalid


def _filter_frame(x, mask, state, errid, scale_factor, status):
    dev = state.device
    bs = mask.shape[0]
    xv = L.dev(x.detach()).reshape(bs, -1)
    m = mask.reshape(bs, -1)
    m = m.contiguous() if m.dtype in (torch.bool, torch.uint8) else L.dev(m)
    if m.device != dev or m.shape != xv.shape:
        raise ValueError(f"loss_filter: values {tuple(xv.shape)} and mask {tuple(m.shape)} on {m.device}")
    e = _ids(errid, dev, "errid")
    if e.numel() != bs:
        raise ValueError(f"loss_filter: {bs} batch rows, {e.numel()} errid")
    flo_err = torch.empty((bs,), device=dev)
    invalid = torch.empty((bs,), dtype=torch.bool, device=dev)
    L.call("moda_loss_filter_frame", L.ptr(xv), L.ptr(m), int(m.dtype != torch.float32), bs, xv.shape[1], L.ptr(state), state.numel(),
           L.ptr(e), int(e.dtype == torch.int64), float(scale_factor), L.ptr(flo_err), L.ptr(invalid), L.ptr(status), L.stream())
    return flo_err, invalid


def _check_state(t, numel, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == numel):
        raise ValueError(f"{what}: the state must be a contiguous fp32 device tensor of {numel} entries (the reference's numpy "
                         "array holds fp32 values: nothing is lost)")


MAX_FILTER_FRAMES = 8000        # include/moda_hip.h: moda_loss_filter_line / _frame


class LossFilter:
    """The frame rejection of moda.py:522-538 with its state -- the reference's `latest_vars['sil_err']` -- on the device.
    lineload=True  (loss_utils.py:432-445 loss_filter_line): state `sil_err` (num_frames * img_size,) fp32;
                   flt(sil_loss_weighted (N, ...), errid (N,), frameid (N,)) -> invalid (N,) bool.
    lineload=False (loss_utils.py:447-476 loss_filter + the update of moda.py:533): state (num_frames,);
                   flt(sil_loss_weighted (bs, n, ...), errid (bs,), mask=None (bs, n, ...)) -> invalid (bs,) bool; mask None is
                   the reference's `sil_at_samp > -1`, every ray.  `flt.flo_err` holds the batch's per-frame errors.
    The call enqueues three launches (one in frame mode) on the current stream, allocates only through torch's allocator and
    reads nothing back: it can be captured.  `status` (4,) int32 = [#ids out of range (skipped), #invalid rays, #frames with
    history, 0] stands for the reference's `print('%d removed from sil')`.  `reset()` is the per-epoch zeroing of
    train_utils.py:1120.  errid / frameid: int32 or int64 device tensors."""

    def __init__(self, num_frames, img_size, lineload=True, scale_factor=10, device="cuda"):
        self.num_frames, self.img_size, self.lineload, self.scale_factor = int(num_frames), int(img_size), bool(lineload), scale_factor
        dev = torch.device(device)
        if not 1 <= self.num_frames <= MAX_FILTER_FRAMES:
            raise ValueError(f"LossFilter: num_frames must lie in 1..{MAX_FILTER_FRAMES} (the medians are ranked in one workgroup's LDS)")
        if dev.type != "cuda":
            raise RuntimeError("LossFilter lives on a CUDA (ROCm) device; the HIP library is the only compute path")
        self.sil_err = torch.zeros((self.num_frames * self.img_size if self.lineload else self.num_frames,), device=dev)
        self.status = torch.zeros((4,), dtype=torch.int32, device=dev)
        self.flo_err = None
        self._ws = _filter_ws(self.num_frames, self.img_size, dev) if self.lineload else None

    def reset(self):
        self.sil_err.zero_()

    def __call__(self, sil_loss_weighted, errid, frameid=None, mask=None):
        if self.lineload:
            if frameid is None:
                raise ValueError("LossFilter(lineload=True) takes errid and frameid")
            return _filter_line(sil_loss_weighted, errid, frameid, self.sil_err, self.num_frames, self.img_size, self.scale_factor,
                                self._ws, None, self.status)
        if mask is None:
            mask = torch.ones(sil_loss_weighted.shape, dtype=torch.bool, device=self.sil_err.device)
        self.flo_err, invalid = _filter_frame(sil_loss_weighted, mask, self.sil_err, errid, self.scale_factor, self.status)
        return invalid


def loss_filter_line(sil_err, errid, frameid, sil_loss_samp, img_size, scale_factor=10):
    """loss_utils.py:432-445 with the reference's signature; `sil_err` a contiguous fp32 DEVICE tensor of num_frames * img_size
    entries, updated in place as the reference updates its array.  -> invalid (N,) bool, on the device."""
    if not torch.is_tensor(sil_err) or sil_err.numel() % int(img_size):
        raise ValueError("loss_filter_line: sil_err must be a device tensor of num_frames * img_size entries")
    _check_state(sil_err, sil_err.numel(), "loss_filter_line")
    T = sil_err.numel() // int(img_size)
    status = torch.empty((4,), dtype=torch.int32, device=sil_err.device)
    return _filter_line(sil_loss_samp, errid, frameid, sil_err, T, int(img_size), scale_factor,
                        _filter_ws(T, int(img_size), sil_err.device), None, status)


def loss_filter(g_floerr, flo_loss_samp, sil_at_samp_flo, scale_factor=10):
    """loss_utils.py:447-476 with the reference's signature; `g_floerr` the (T,) fp32 device history, NOT updated (the caller
    assigns `g_floerr[errid] = flo_err`, moda.py:533).  -> (flo_err (bs,), invalid (bs,) bool), device tensors."""
    _check_state(g_floerr, g_floerr.numel() if torch.is_tensor(g_floerr) else -1, "loss_filter")
    bs = sil_at_samp_flo.shape[0]
    status = torch.empty((4,), dtype=torch.int32, device=g_floerr.device)
    none = torch.full((bs,), -1, dtype=torch.int32, device=g_floerr.device)     # ids outside the table: no update
    return _filter_frame(flo_loss_samp, sil_at_samp_flo, g_floerr, none, scale_factor, status)


_OFFSETS = {}


def _offset_table(data_offset, T, device, what="compute_root_sm_2nd_loss"):
    """The videos' frame ranges as a device int32 table, uploaded once per distinct tuple."""
    off = tuple(int(v) for v in (data_offset.tolist() if hasattr(data_offset, "tolist") else data_offset))
    if len(off) < 2 or off[0] < 0 or off[-1] > T or any(b < a for a, b in zip(off, off[1:])):
        raise ValueError(f"data_offset {off}: expected non-decreasing frame indices within [0, {T}]")
    key = (off, str(device))
    t = _OFFSETS.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{what}: a new data_offset is uploaded from the host -- call once before capture")
        t = torch.tensor(off, dtype=torch.int32).to(device)
        _OFFSETS[key] = t
    return t


def root_sm_parts(rtk_all, data_offset):
    """-> (loss, parts (3,) detached = [0.1 * mean angle, mean trn, #triples]) of compute_root_sm_2nd_loss."""
    r = L.dev(rtk_all)
    if r.dim() != 3 or r.shape[1] not in (3, 4) or r.shape[2] != 4:
        raise ValueError(f"rtk_all: expected (T, 4, 4) or (T, 3, 4), got {tuple(r.shape)}")
    return A.RootSmFn.apply(r, _offset_table(data_offset, r.shape[0], r.device))


def compute_root_sm_2nd_loss(rtk_all, data_offset):
    """loss_utils.py:486-517: 0.1 * (0.1 * mean rot_angle((R0 R1^T)(R1 R2^T)^T) + mean |(t0 - t1) - (t1 - t2)|) over the
    consecutive frame triples of every video [data_offset[v], data_offset[v + 1]); NaN when no video has three frames.  One
    kernel forward, one backward (a gather per frame: no atomics, the same bits on every run)."""
    return root_sm_parts(rtk_all, data_offset)[0]


# ---- the warm-up stages that run before the first forward_default call (moda_amd/warmup.py) ----------------------------------------
def _warm_tensor(t, what, shape_txt, ok_shape):
    """A warm-up input as its kernel reads it: a contiguous fp32 device tensor.  Nothing is converted: CPU tensors raise
    RuntimeError, another dtype / shape / layout ValueError, each naming the argument."""
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: expected a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{what} must be a CUDA (ROCm) tensor; the HIP library is the only compute path")
    if t.dtype != torch.float32 or not ok_shape(t.shape) or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous fp32 tensor of shape {shape_txt}, got {t.dtype} {tuple(t.shape)}, "
                         f"contiguous={t.is_contiguous()}")
    return t


def _pose_rows(t, what):
    return _warm_tensor(t, what, "(T, 4, 4) or (T, 3, 4)", lambda s: len(s) == 3 and s[0] >= 1 and s[1] in (3, 4) and s[2] == 4)


def shape_targets(u, obj_bound, bound_factor, use_ellips=True):
    """The sample points and SDF targets of shape_init_loss (loss_utils.py:546-563) in one launch of moda_shape_target:
    u (n,3) uniforms in [0, 1), obj_bound (3,) -> (pts (1,n,3) = (u * 2) * bound - bound with bound = obj_bound * bound_factor,
    bit-equal to the reference on the same u; dis (n,), the signed distance to the ellipsoid with the semi-axes obj_bound scaled by
    their mean, or to the sphere of radius min(obj_bound))."""
    u = _warm_tensor(u, "u", "(n, 3)", lambda s: len(s) == 2 and s[0] >= 1 and s[1] == 3)
    if u.requires_grad:
        raise NotImplementedError("u: uniforms that require grad are not implemented (the samples have no backward kernel)")
    ob = _warm_tensor(obj_bound, "obj_bound", "(3,)", lambda s: tuple(s) == (3,)).detach()
    n = u.shape[0]
    pts = torch.empty((1, n, 3), device=u.device)
    dis = torch.empty((n,), device=u.device)
    L.call("moda_shape_target", L.ptr(u), n, L.ptr(ob), float(bound_factor), int(bool(use_ellips)), L.ptr(pts), L.ptr(dis), L.stream())
    return pts, dis


def shape_init_loss(pts, faces, mlp, embed, bound_factor, use_ellips=True, *, nsample=10000, u=None, obj_bound=None, dy_sum=None):
    """loss_utils.py:540-572: pull the coarse SDF towards the ellipsoid (use_ellips) or sphere of the template's bound.  pts (V,3)
    the template vertices (a device tensor); `faces` is accepted and unused -- the reference builds a trimesh from it and never
    reads it.  u (n,3): the uniforms of this step, a device tensor used as given (what pins a call to a reference run, and what a
    captured step refills); None draws torch.rand((nsample, 3)) on the device.  obj_bound (3,): the cached pts.abs().amax(0); None
    computes it on the device.  The network runs as mlp.train_forward(..., sigma_only=True) when gradients are wanted, else as
    mlp.fused(..., sigma_only=True); the loss is autograd.ShapeLossFn.  dy_sum (1,): a device buffer that the backward fills with
    the sum of the loss' gradient over the network's outputs, in a fixed order: the gradient of mlp.sigma.bias with the same bits on
    every run (the network's own backward adds that sum with float atomics; WarmupHarness writes this one over it).  Nothing is
    read back: with u given the call can be captured.  -> the loss, a 0-dim tensor."""
    pts = _warm_tensor(pts, "pts", "(V, 3)", lambda s: len(s) == 2 and s[0] >= 1 and s[1] == 3)
    if obj_bound is None:
        obj_bound = pts.detach().abs().amax(0)                                         # :548
    if u is None:
        if int(nsample) < 1:
            raise ValueError(f"nsample must be positive, got {nsample}")
        u = torch.rand((int(nsample), 3), device=pts.device)                           # :550 (the reference draws on the CPU)
    pts_samp, dis = shape_targets(u, obj_bound, bound_factor, use_ellips)
    if torch.is_grad_enabled() and any(p.requires_grad for p in mlp.parameters()):
        y = mlp.train_forward(pts_samp, embed, sigma_only=True)
    else:
        y = mlp.fused(pts_samp, n_freq=embed.N_freqs, alpha=embed.alpha, sigma_only=True)
    return A.ShapeLossFn.apply(y.reshape(-1), dis, dy_sum)


def rtk_loss(rtk, rtk_raw, aux_out):
    """loss_utils.py:151-163: 0.01 * mean rot_angle(Rp Rg^T) + mean |tp - tg|^2 over the predicted poses rtk (T, 3 | 4, 4) and
    the table rtk_raw (T, 3 | 4, 4); aux_out['rot_loss'] and aux_out['trn_loss'] are filled with 0-dim device tensors, each
    differentiable on its own.  One launch forward, one backward (a thread per frame); no gradient flows to rtk_raw."""
    r, gt = _pose_rows(rtk, "rtk"), _pose_rows(rtk_raw, "rtk_raw")
    if gt.shape[0] != r.shape[0]:
        raise ValueError(f"rtk_raw: {gt.shape[0]} frames, rtk has {r.shape[0]}")
    total, rot, trn = A.RtkLossFn.apply(r, gt.detach())
    aux_out['rot_loss'] = rot
    aux_out['trn_loss'] = trn
    return total


def root_sm1_parts(rtk_all, data_offset):
    """-> (loss, parts (3,) detached = [1e-3 * mean angle, 0.1 * mean trn, #pairs]) of compute_root_sm_loss."""
    r = _pose_rows(rtk_all, "rtk_all")
    return A.RootSm1Fn.apply(r, _offset_table(data_offset, r.shape[0], r.device, "compute_root_sm_loss"))


def compute_root_sm_loss(rtk_all, data_offset):
    """loss_utils.py:520-537: 1e-3 * mean rot_angle(R_i R_{i+1}^T) + 0.1 * mean |t_i - t_{i+1}| over the consecutive frame pairs
    of every video [data_offset[v], data_offset[v + 1]), the pairs of all videos pooled before the means.  The degenerate cases
    follow the rule of compute_root_sm_2nd_loss here: a video too short for a pair (length 0 or 1) contributes none, as the
    reference's empty slices do, and when no video has a pair the loss is NaN, the mean of an empty set (gradient zero).  The
    translation norm's gradient at a zero difference is 0, torch's sub-gradient.  One kernel forward, one backward (a gather per
    frame: no atomics, the same bits on every run)."""
    return root_sm1_parts(rtk_all, data_offset)[0]


# flags of moda.py the assembly reads, with the reference's defaults (moda.py:53-172)
LOSS_OPTS = dict(lineload=False, use_unc=False, img_size=512, warmup_steps=0.4, freeze_coarse=False, freeze_proj=False, proj_start=0.0,
                 proj_end=0.2, ft_cse=False, mt_cse=True, use_embed=True, use_proj=True, use_corresp=True, total_wt=1.0, sil_wt=0.1,
                 img_wt=0.1, feat_wt=0.0, use_corr=False, corr_wt=0.01, frnd_wt=1.0, proj_wt=0.02, flow_wt=1.0, cyc_wt=1.0,
                 root_sm=True, eikonal_wt=0.0, bone_loc_reg=0.1, loss_flt=True, rm_novp=True, s3im_loss=False, s3im_wt=0.01,
                 lbs=True, neudbs=True)


def _opt(opts, name):
    if isinstance(opts, dict):
        return opts.get(name, LOSS_OPTS[name])
    return getattr(opts, name, LOSS_OPTS[name])


def proj_warmup_weight(progress, proj_start, proj_end):
    """moda.py:633-635 in float64, as numpy evaluates it."""
    w = (float(progress) - proj_start) / (proj_end - proj_start)
    return float(np.clip((w - 0.8) * 5, 0, 1))


def bone_loc_loss(model, mesh_rest, opts=None, *, num_samples=1000, generator=None, u=None, samples_loss=None):
    """The bone-location term of moda.py:681-698, unweighted: the rest bones moved by the rest pose (correct_bones), `num_samples`
    points drawn on the rest mesh (sample_points_from_meshes; `generator` / `u` as there), and the debiased Sinkhorn divergence
    SamplesLoss("sinkhorn", p=2, blur=.05) between the bone centres and the samples, both times 10 (moda_amd.samples_loss).
    -> a 0-dim tensor to pass as forward_loss(..., bone_loc=); None when the mesh has 100 vertices or fewer, the reference's
    silent skip (moda.py:686: a shape test, nothing is read back) -- pass bone_loc=False then.
    Gradient reaches model.bones, rest_pose_code and the pose head through correct_bones' autograd; none flows to the samples.
    mesh_rest: a TriMesh or anything with .vertices / .faces.  samples_loss: a SamplesLoss("sinkhorn", p=2, blur=.05) to reuse --
    its .status tensor then tells why a term came out NaN (a non-finite bone or sample, a degenerate diameter); None builds one."""
    from .bones import sample_points_from_meshes
    from .feeders import correct_bones
    from .samples_loss import SamplesLoss
    verts = getattr(mesh_rest, "vertices_t", None)
    if verts is None:
        verts = mesh_rest.vertices
    if len(verts) <= 100:                                                              # moda.py:686
        return None
    bones_rst, _ = correct_bones(model, model.bones, neudbs=True if opts is None else _opt(opts, "neudbs"))   # moda.py:683-684
    if torch.is_tensor(verts) and hasattr(mesh_rest, "faces_t"):
        samp = sample_points_from_meshes(mesh_rest, num_samples=num_samples, generator=generator, u=u)
    else:
        dev = bones_rst.device
        v = torch.as_tensor(np.asarray(mesh_rest.vertices), dtype=torch.float32).to(dev)
        f = torch.as_tensor(np.asarray(mesh_rest.faces).astype(np.int32)).to(dev)
        samp = sample_points_from_meshes(v, f, num_samples=num_samples, generator=generator, u=u)
    if samples_loss is None:
        samples_loss = SamplesLoss("sinkhorn", p=2, blur=.05)
    return samples_loss(bones_rst[:, :3] * 10, samp.detach() * 10)                                  # moda.py:693-695


def forward_loss(rendered, opts, *, loss_filter=None, errid=None, frameid=None, progress=0., loss_select=1, rtk_all=None,
                 data_offset=None, extra_terms=(), bone_loc=None):
    """The loss assembly of banmo.forward_default (moda.py:517-768) with the branches the reference's default flags take:
    the frame filter (loss_flt: `loss_filter`, a LossFilter, with `errid` / `frameid`), rm_novp (five terms times the detached
    rendered['sil_coarse']), root_sm (`rtk_all`, `data_offset`), the loss_select == 0 and projection warm-ups, total_wt.
    Flags come from `opts` (an object or a dict), the reference's default (LOSS_OPTS) where one is absent.  The filter is three
    launches, the root term one, the assembly ONE each way (moda_loss_assembly); nothing is read back, so the step can be captured.
    -> (total_loss, aux_out): aux_out holds the reference's keys as 0-d device tensors, views of one output tensor.

    Terms in the reference's order: img, sil, s3im, frnd, flo, feat, corr, proj (twice inside the warm-up window), cyc, elastic,
    dis_reg, dis_reg_forward, root_sm, eikonal (rendered['eikonal_loss'], from `eikonal_loss`), bone_loc, vis, unc (`unc_loss`),
    then `extra_terms` ((name, weight, tensor) each, added as weight * tensor.mean()); sixteen at the most.

    bone_loc (moda.py:681-698, with lbs / neudbs and bone_loc_reg > 0, the reference's default 0.1): pass
    `bone_loc=bone_loc_loss(model, mesh_rest)`, a 0-dim tensor -- the term bone_loc_reg * bone_loc is added and logged as
    aux_out['bone_loc_loss'] (weighted, as the reference logs it).  bone_loc_loss returns None for a rest mesh of 100 vertices or
    fewer, where the reference skips the term silently: pass `bone_loc=False` for that skip.  bone_loc=None with the flag on
    raises -- a forgotten term must not pass for the reference's skip.

    Under graph capture: `progress`, `loss_select` and the projection warm-up weight are HOST values that decide which terms are
    filtered and the carry / weight arguments of the launch -- a captured graph replays those of capture time.  Re-capture when
    `progress` crosses warmup_steps, when loss_select changes, and do not capture inside (proj_start, proj_end) with freeze_proj,
    where the weight changes every step.

    Deviations, all stated: rendered['sil_loss_samp'] and rendered['flo_loss_samp'] are NOT zeroed in place at the rejected
    rows (moda.py:536, :580) -- the zeroing happens inside the kernel and `rendered` is left as it was; the bone-location term is computed by the caller
    (bone_loc_loss: it needs the model and the rest mesh, which `rendered` does not hold) and its Sinkhorn divergence restates
    geomloss 0.2.4, which the reference tree does not contain; ft_cse and freeze_coarse raise NotImplementedError."""
    o = lambda name: _opt(opts, name)
    with_bone_loc = (o("lbs") or o("neudbs")) and o("bone_loc_reg") > 0
    if with_bone_loc and bone_loc is None:
        raise NotImplementedError("bone_loc_reg > 0 (the reference's default 0.1) needs the bone-location term: pass bone_loc="
                                  "moda_amd.loss_utils.bone_loc_loss(model, mesh_rest) (a 0-dim tensor), bone_loc=False where that "
                                  "returns None (a rest mesh of 100 vertices or fewer: the reference's skip), or set "
                                  "opts.bone_loc_reg = 0")
    if o("ft_cse") and o("mt_cse"):
        raise NotImplementedError("ft_cse (the csenet fine-tuning term of moda.py:724-731) is not implemented")
    if o("freeze_coarse"):
        raise NotImplementedError("freeze_coarse (the xyz-weight terms of moda.py:733-755) is not implemented")
    sil = rendered["sil_at_samp"]
    invalid = None
    if o("loss_flt"):                                                                  # moda.py:522-533
        if loss_filter is None or errid is None:
            raise ValueError("opts.loss_flt (the reference's default) needs loss_filter= (a LossFilter) and errid=")
        weighted = rendered["sil_loss_samp"].detach() * o("sil_wt")
        if loss_filter.lineload:
            invalid = loss_filter(weighted, errid, frameid)
        else:                                     # whole frames: errid has one entry per frame, the rays are bs equal runs (bs, n)
            bs = errid.numel()
            if bs < 1 or weighted.numel() % bs:
                raise ValueError(f"forward_loss: {weighted.numel()} rays are not {bs} frames (errid) of equal length")
            inv = loss_filter(weighted.reshape(bs, -1), errid)                         # (bs,) -> one flag per ray
            invalid = inv[:, None].expand(bs, weighted.numel() // bs).reshape(-1)
    scale = rendered["sil_coarse"] if o("rm_novp") else None
    plan = []                                                                          # (aux key, x, weight, mask, kind, scale, drop, carry)

    def add(key, x, wt, mask=None, kind=None, sc=None, drop=None, carry=1.0):
        plan.append((key, x, wt, mask, kind, sc, drop, carry))

    add("img_loss", rendered["img_loss_samp"], o("img_wt"), sil, ">0", scale, invalid)                           # :540-549
    add("sil_loss", rendered["sil_loss_samp"], o("sil_wt"), rendered["vis_at_samp"], ">0", None,
        invalid if progress > o("warmup_steps") else None)                                                        # :535-536, :550-551
    if o("s3im_loss"):
        add("s3im_loss", rendered["s3im_loss"], o("s3im_wt"))                                                    # :560-563
    add("feat_rnd_loss", rendered["frnd_loss_samp"], o("frnd_wt"), sil, ">0", scale, invalid)                    # :566-574
    if o("use_corresp"):                                                                                          # :577-594
        add("flo_loss", rendered["flo_loss_samp"], 2.0 * o("flow_wt"), rendered["sil_at_samp_flo"], "bool", scale, invalid,
            0.0 if loss_select == 0 else 1.0)
    if o("use_embed"):                                                                                            # :597-618
        add("feat_loss", rendered["feat_err"], o("feat_wt"), sil, ">0", scale, invalid)
        if o("use_corr"):
            add("corr_loss", rendered["corr_err"], o("corr_wt"), sil, ">0", scale, invalid)
    if o("use_proj"):                                                                                             # :622-642
        add("proj_loss", rendered["proj_err"], o("proj_wt"), sil, ">0", None, invalid)
        if o("freeze_proj") and o("proj_start") < progress < o("proj_end"):
            w = proj_warmup_weight(progress, o("proj_start"), o("proj_end"))
            add(None, rendered["proj_err"], 10.0 * (1.0 - w) * o("proj_wt"), sil, ">0", None, invalid, w)      # total*w + 10*proj*(1-w)
    if "frame_cyc_dis" in rendered:                                                                               # :645-656
        add("cyc_loss", rendered["frame_cyc_dis"], o("cyc_wt"))
        if "elastic_loss" in rendered:
            add("elastic_loss", rendered["elastic_loss"], 1e-3)
    if "dis_reg" in rendered:                                                                                     # :659-664
        add(None, rendered["dis_reg"], 1.0)
    if "dis_reg_forward" in rendered:
        add(None, rendered["dis_reg_forward"], 1.0)
    root_parts = None
    if o("root_sm"):                                                                                              # :667-670
        if rtk_all is None or data_offset is None:
            raise ValueError("opts.root_sm (the reference's default) needs rtk_all= and data_offset=")
        root, root_parts = root_sm_parts(rtk_all, data_offset)
        add("root_sm_loss", root, 1.0)
    if o("eikonal_wt") > 0:                                                                                       # :673-678
        if "eikonal_loss" not in rendered:
            raise KeyError("opts.eikonal_wt > 0: put moda_amd.loss_utils.eikonal_loss(...) into rendered['eikonal_loss']")
        add("ekl_loss", rendered["eikonal_loss"], o("eikonal_wt"))
    if with_bone_loc and bone_loc is not False:                                                                   # :681-698
        if not (torch.is_tensor(bone_loc) and bone_loc.numel() == 1):
            raise ValueError("forward_loss: bone_loc must be the 0-dim tensor of bone_loc_loss(...), or False")
        add("bone_loc_loss", bone_loc, o("bone_loc_reg"))
    if "vis_loss" in rendered:                                                                                    # :701-704
        add("visibility_loss", rendered["vis_loss"], 0.01)
    if o("use_unc"):                                                                                              # :707-720
        img = rendered["img_loss_samp"].detach() * o("img_wt")                                                   # :540
        if invalid is not None:                                                                                   # :544 `*= 0`
            img = img.reshape(invalid.numel(), -1) * (~invalid).to(img.dtype)[:, None]
        add("unc_loss", unc_loss(rendered, img_loss_samp=img), 1.0)
    for name, wt, x in extra_terms:
        add(name, x, wt)
    if len(plan) > 16:
        raise ValueError(f"forward_loss: {len(plan)} terms, moda_loss_assembly takes 16")
    spec = [(wt, mask, kind, sc, drop, carry) for _, _, wt, mask, kind, sc, drop, carry in plan]
    total, rest = A.LossAssemblyFn.apply(spec, o("total_wt"), *[p[1] for p in plan])
    T = len(plan)
    aux_out = {}
    for t, p in enumerate(plan):
        if p[0] is not None:
            aux_out[p[0]] = rest[2 * T + t] if p[0] == "cyc_loss" else rest[t]         # cyc_loss is logged unweighted (:650)
    aux_out["total_loss"] = total.detach()
    if root_parts is not None:
        aux_out["root_rot_sm"], aux_out["root_trn_sm"] = root_parts[0], root_parts[1]
    if invalid is not None:
        aux_out["invalid"] = invalid
        aux_out["filter_status"] = loss_filter.status
    return total, aux_out


def unc_loss(rendered, img_loss_samp=None):
    """The uncertainty network's own loss (moda.py:707-720): mean over rays of (sil_at_samp * img_loss_samp.mean(-1)).detach() -
    unc_pred[..., 0], squared.  Only nerf_unc receives a gradient from it.  img_loss_samp: the tensor the reference has at that
    point -- img_wt * rendered['img_loss_samp'] with the filter's rejected rows zeroed (moda.py:540-544; forward_loss passes it);
    None: rendered['img_loss_samp'] as it is."""
    img = rendered["img_loss_samp"] if img_loss_samp is None else img_loss_samp
    sil0 = L.dev(rendered["sil_at_samp"])[..., 0]
    target = (sil0 * img.reshape(tuple(sil0.shape) + (-1,)).mean(-1)).detach()
    return A.RowDistFn.apply(rendered["unc_pred"].reshape(-1, 1), target.reshape(-1, 1), True).mean()


def s3im_loss(src_vec, tar_vec, mask, kernel_size=4, stride=4, repeat_time=10, patch_height=32, patch_width=32, rng=None):
    """S3IM(kernel_size, stride, repeat_time, patch_height, patch_width)(src_vec, tar_vec, mask) of loss_utils.py:648-702 with
    the constructor arguments rendering.py:529 passes as defaults: 1 - SSIM(window 4, stride 4) between the rendered and
    the observed colours (both times the mask) re-arranged into a (1, 3, 32, 32 * 10) virtual patch -- the first 1024 rays
    (rows repeated when there are fewer), once in order and nine times permuted (torch.randperm on the CPU, as there; or
    rng['s3im_perms'], (repeat_time - 1, 1024) integers).  One kernel forward, one backward (csrc/loss_kernels.hip).
    Unlike the reference this does NOT multiply its arguments by the mask in place; render_rays mirrors that side effect."""
    if kernel_size != 4 or stride != 4:
        raise NotImplementedError("the S3IM kernel implements the reference's call: kernel_size = stride = 4 (rendering.py:529)")
    src = L.dev(src_vec).reshape(-1, 3)
    tar = L.dev(tar_vec).reshape(-1, 3)
    P = patch_height * patch_width
    perms = (rng or {}).get('s3im_perms')
    if perms is None:
        perms = torch.stack([torch.randperm(P) for _ in range(repeat_time - 1)]) if repeat_time > 1 else torch.zeros((0, P))
    perms = torch.as_tensor(perms).to(device=src.device, dtype=torch.int32).reshape(-1)
    if perms.numel() != (repeat_time - 1) * P:
        raise ValueError(f"s3im_perms: expected {(repeat_time - 1, P)} indices, got {perms.numel()}")
    ident = L.const_tensor(("arange", P), src.device, lambda: torch.arange(P)).to(torch.int32)
    index = torch.cat([ident, perms])                                                  # :678-686
    return A.S3imFn.apply(src, tar, L.dev(mask).reshape(-1, 1).expand(src.shape[0], 1), index, patch_height)


def nerf_gradient(mlp, embed, pts, use_xyz=False, code=None, sigma_only=False):
    """loss_utils.py:15-47 for the density head: (d y / d pts (..., 3, 1), sigmas (..., 1)), the gradient differentiable
    with respect to the parameters.

    The reference differentiates autograd's own backward pass (create_graph=True).  Here the reverse sweep is written
    out as forward nodes -- g <- (g * relu_mask_i) W_i from the density row back to the encoding, then the encoding's
    Jacobian -- so one ordinary backward gives the same parameter gradient (ReLU'' = 0: the masks are constants, which
    is also what the double backward sees)."""
    if not sigma_only or code is not None or use_xyz:
        raise NotImplementedError("nerf_gradient serves eikonal_loss: sigma_only=True, no code (loss_utils.py:97)")
    if mlp.skips != [4]:
        raise NotImplementedError("skips=[4] (the only value MoDA uses)")
    lead = pts.shape[:-1]
    x = L.dev(pts).detach().reshape(-1, 3)
    P = x.shape[0]
    with torch.no_grad():                                   # primal pass: activation signs and y
        emb = embed(x)
        h, masks = emb, []
        for i in range(mlp.D):
            if i in mlp.skips:
                h = torch.cat([emb, h], -1)
            h = mlp._linear(h, getattr(mlp, f"xyz_encoding_{i+1}")[0], 1)
            masks.append(h > 0)
        y = mlp._linear(h, mlp.sigma, 0)
        sdf = -y
        sigmas = 0.5 + 0.5 * sdf.sign() * torch.expm1(-sdf.abs() / (mlp.beta.abs() + 1e-9))
    ne = emb.shape[1]
    g = mlp.sigma.weight.expand(P, mlp.W)
    g_emb = None
    for i in reversed(range(mlp.D)):
        lin = getattr(mlp, f"xyz_encoding_{i+1}")[0]
        g = A.LinearFn.apply(g * masks[i], lin.weight.t(), None, 0)          # (P, fan_in) = (g . mask) W
        if i in mlp.skips:
            g_emb, g = g[:, :ne], g[:, ne:]
    g_emb = g if g_emb is None else g_emb + g
    # encoding Jacobian (nerf.py:58-72 order: x, then sin(2^k x), cos(2^k x) per band, each times the window w_k): one kernel,
    # differentiable w.r.t. g_emb through the encoding's tangent kernel (A.EmbedJacTFn; torch.sin / cos loops before round 5)
    out = A.EmbedJacTFn.apply(x, g_emb.contiguous(), embed.N_freqs, [float(w) for w in embed.window()])
    return out.view(lead + (3, 1)), sigmas.view(lead + (1,))


def compute_gradients_sdf(mlp, embed, pts, sigma_only=False, eps=1e-3):
    """loss_utils.py:48-71: tetrahedral finite differences, four density evaluations (whole-network nodes)."""
    pts = L.dev(pts).detach()
    ks = ((1, -1, -1), (-1, -1, 1), (-1, 1, -1), (1, 1, 1))
    total = None
    for kk in ks:
        k = L.const_tensor(("tetra", kk), pts.device, lambda: np.asarray(kk, np.float32))
        sdf = mlp.train_forward(pts + k * eps, embed, sigma_only=sigma_only)
        total = k * sdf if total is None else total + k * sdf
    return total / (4.0 * eps)


def eikonal_loss(mlp, embed, pts, bound, ppr_eikonal, rng=None):
    """loss_utils.py:73-104: mean (|d sigma / d x| - 1)^2 over (at most 1000 rays of) the in-bound canonical points.
    Out-of-bound points are weighted 0 instead of being gathered out, so no size is read back from the device."""
    bs = pts.shape[0]
    if bs > 1000:                                                                                     # :79-84
        ri = (rng or {}).get('eik_inds')
        ri = torch.multinomial(torch.ones(bs), 1000, replacement=False) if ri is None else ri
        pts = pts[ri.to(pts.device)]
    pts = L.dev(pts).detach().reshape(-1, 3)
    bt = tuple(float(b) for b in np.asarray(bound).reshape(-1)[:3])
    bnd = L.const_tensor(("bound", bt), pts.device, lambda: np.asarray(bt, np.float32))[None]
    inb = (((bnd - pts.abs()) > 0).sum(-1) == 3).float()                                              # :91
    if ppr_eikonal:
        g = compute_gradients_sdf(mlp, embed, pts, sigma_only=True)
    else:
        g = nerf_gradient(mlp, embed, pts, sigma_only=True)[0][..., 0]
    err = (g.norm(2, dim=-1) - 1) ** 2
    return (err * inb).sum() / inb.sum()
