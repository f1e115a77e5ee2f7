"""GPU (-m gpu): the device-resident root poses (moda_amd/csrc/rootpose_kernels.hip behind feeders.RTHead / RTExplicit / RTExpMLP,
root_pose.compute_rts / convert_root_pose, geom_utils.prepare_ray_cams) against the float64 restatement tests/rootpose_numpy.py.

Tolerance: every output is compared with the float64 restatement and may differ by 4 x d_ref, d_ref = max |fp32 - float64| of the
reference's own CPU run of that output (tests/golden/g32_root_pose.npz), with a floor of 4 ulp of the output's largest magnitude
(rootpose_cases.allowance): a different summation order, the device's sin / cos / sqrt 1-2 ulp off libm, and 1 - cos(theta) near the
clamp.  Recorded d_ref: RTHead out 2.0e-7 / 6.0e-8 (quaternion / rotation vector), RTExplicit out 1.0e-7 / 2.3e-7 and d_se3 2.5e-4 /
1.3e-6 (the quaternion rows include |q| = 1e-3, whose gradient is 1e3 times an ordinary one), RTExpMLP out 5.8e-7 / 7.4e-7, d_se3
1.6e-3 / 3.3e-6, d_rgb 5.4e-8 / 1.0e-7, refine_rt 5.9e-8, Kinv 1.7e-7.  Agreement with the fp32 golden itself: <= 1e-4 relative.
The composed tail has a d_ref per case (60 cases: rtk 2.1e-7 .. 7.7e-7, d_se3 3.5e-7 .. 6.7e-5, d_delta 4.0e-7 .. 5.2e-6), the chain into
raycast its own (rays_d 4.7e-7, d_se3 2.5e-5, d_rgb 2.9e-7, d_ks 6.7e-9).  
Largest observed error on an MI355X as a fraction of its allowance:
0.68 (RTExpMLP last-layer gradient, 1.5e-7 of 2.2e-7), 0.63 (the tail's d_se3, 5.2e-5 of 8.3e-5), 0.53 (RTExpMLP d_se3 with rotation vectors), 
0.51 (RTHead last-layer gradient), 0.36 (d_se3 through raycast), 0.32 (the tail's rtk), 0.31 (the tail's d_delta); every other output below 0.3."""
import numpy as np
import pytest
import torch

import rootpose_cases as C
import rootpose_numpy as rn
from helpers import golden, rel_err

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import moda_amd
    from moda_amd import feeders as FD, root_pose as RP, geom_utils as GU
    from gpu_helpers import T, DEV


def np_(t):
    return t.detach().cpu().numpy()


def ids_t(a, dtype=torch.int64):
    return torch.as_tensor(np.asarray(a), dtype=dtype, device=DEV)


@pytest.fixture(autouse=True)
def exact_fp32():
    prev = moda_amd.get_train_precision()
    moda_amd.set_train_precision("fp32")
    yield
    moda_amd.set_train_precision(prev)


def check(name, got, ref64, d_ref, report):
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    err, tol = float(np.abs(got - ref64).max()), C.allowance(ref64, d_ref)
    report.append((name, err, tol))
    print(f"{name:40s} err {err:.3e} allowance {tol:.3e}")
    assert err <= tol, (name, err, tol)


def tail(se3=None, ids=None, delta=None, rt_raw=None, mode=None, obj_scale=1.0, ks=None, dataid=None, rows=4, g=None, ids_dtype=torch.int64):
    """One call of the fused tail on the device -> (rtk, status, grads dict)."""
    mode = (FD.RAW_BASE if rt_raw is None else FD.RAW_ROWS) if mode is None else mode
    se3_t = None if se3 is None else T(se3).requires_grad_(True)
    delta_t = None if delta is None else T(delta).requires_grad_(True)
    ks_t = None if ks is None else T(ks).requires_grad_(True)
    rtk, status = FD.RootPoseFn.apply(se3_t, None if ids is None else ids_t(ids, ids_dtype), delta_t, None if rt_raw is None else T(rt_raw),
                                      mode, obj_scale, ks_t, None if dataid is None else ids_t(dataid, torch.int32), rows)
    grads = {}
    if g is not None:
        (T(g) * rtk).sum().backward()
        grads = {k: np_(t.grad) for k, t in (("d_se3", se3_t), ("d_delta", delta_t), ("d_ks", ks_t)) if t is not None}
    return np_(rtk), np_(status), grads


# ---- the tail on its edge cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [False, True])
def test_explicit_tail_on_the_edge_rows(delta):
    g32, rep = golden("g32_root_pose"), []
    tag = "exp_w" if delta else "exp_q"
    se3 = C.se3_table(delta, 8)
    g4 = rn.rts12_bwd(g32[tag + "_w"].astype(np.float64))
    ref = rn.root_pose(se3=se3, ids=C.EDGE_IDS, raw="none", g=g4)
    for dt in (torch.int64, torch.int32):
        rtk, status, grads = tail(se3=se3, ids=C.EDGE_IDS, mode=FD.RAW_NONE, g=g4.astype(np.float32), ids_dtype=dt)
        assert status.tolist() == [0, 0, 0, 0]
        check(tag + " out", rn.rts12(rtk.astype(np.float64)), rn.rts12(ref["rtk"]), g32[tag + "_dref_out"], rep)
        check(tag + " d_se3", grads["d_se3"], ref["d_se3"], g32[tag + "_dref_d_se3"], rep)
    assert rel_err(rn.rts12(rtk), g32[tag + "_out_32"]) <= 1e-4 and rel_err(grads["d_se3"], g32[tag + "_d_se3_32"]) <= 1e-4
    # the module gives the same numbers as (bs, 1, 12)
    m = FD.RTExplicit(8, delta=delta, rand=False).to(DEV)
    m.se3.data = T(se3)
    out = m(ids_t(C.EDGE_IDS))
    assert out.shape == (len(C.EDGE_IDS), 1, 12) and np.array_equal(np_(out), rn.rts12(rtk))
    if delta:
        # below the clamp theta is a constant: the gradient is what the formula gives with f1, f2 frozen, and row 0 (w = 0) is finite
        w = se3[1:2, 3:6].astype(np.float64)
        assert float((w * w).sum()) < rn.CLAMP32 < float((se3[2, 3:6].astype(np.float64) ** 2).sum())
        assert np.all(np.isfinite(grads["d_se3"]))
        assert np.array_equal(rtk[0, :3, :3], np.eye(3, dtype=np.float32))


@pytest.mark.parametrize("n", C.TAIL_N)
@pytest.mark.parametrize("cols,dcols", C.TAIL_COLS)
def test_tail_shapes_bases_and_raw_forms(n, cols, dcols):
    """Every case has its own d_ref in the fixture: the reference's composed tail (RTExpMLP.forward over these rows, then
    refine_rt) run in fp32 and in float64 on exactly these inputs."""
    g32, rep = golden("g32_root_pose"), []
    c = C.tail_case(n, cols, dcols)
    Tn, se3, delta, ids, ks, dataid, g, raw = (c[k] for k in ("T", "se3", "delta", "ids", "ks", "dataid", "g", "raw"))
    for (name, obj_scale), kw_np, kw_dev in zip(C.TAIL_RAW, (
            dict(raw="base"), dict(rt_raw=raw[:n], raw="rows"), dict(rt_raw=raw[:Tn], raw="by_id")), (
            dict(), dict(rt_raw=raw[:n]), dict(rt_raw=raw[:Tn], mode=FD.RAW_BY_ID))):
        ref = rn.root_pose(se3=se3, ids=ids, delta=delta, ks=ks, dataid=dataid, g=g, obj_scale=obj_scale, **kw_np)
        rtk, status, grads = tail(se3=se3, ids=ids, delta=delta, ks=ks, dataid=dataid, g=g, obj_scale=obj_scale, **kw_dev)
        d = lambda out: float(g32[C.tail_key(n, cols, dcols, name, out)])
        assert status.tolist() == [0, 0, 0, 0]
        assert np.array_equal(rtk[:, 3], ks[dataid])
        check(f"{name} rtk", rtk[:, :3], ref["rtk"][:, :3], d("rtk"), rep)
        check(f"{name} d_se3", grads["d_se3"], ref["d_se3"], d("d_se3"), rep)
        check(f"{name} d_delta", grads["d_delta"], ref["d_delta"], d("d_delta"), rep)
        assert np.array_equal(grads["d_ks"], rn.id_rows_sum(g[:, 3], dataid, 2, dtype=np.float32))       # a plain sum in index order
        absent = np.setdiff1d(np.arange(Tn), ids)
        assert np.all(grads["d_se3"][absent] == 0)
    # three rows of output: compute_rts' layout
    rtk3, _, _ = tail(se3=se3, ids=ids, delta=delta, rows=3)
    rtk4, _, _ = tail(se3=se3, ids=ids, delta=delta, rows=4)
    assert rtk3.shape == (n, 3, 4) and np.array_equal(rtk3, rtk4[:, :3]) and np.all(rtk4[:, 3] == [0, 0, 0, 1])


def test_magnified_gradient_is_ten_times_the_exp_basis():
    rng = np.random.default_rng(3)
    se3 = rng.normal(size=(5, 7)).astype(np.float32)
    ids, g = np.asarray([0, 4, 4, 2, 1, 4]), rng.normal(size=(6, 4, 4)).astype(np.float32)
    _, _, a = tail(se3=se3, ids=ids, delta=np.zeros((6, 6), np.float32), g=g)
    _, _, b = tail(se3=se3, ids=ids, g=g)
    ref = rn.root_pose(se3=se3, ids=ids, raw="base", g=g)["d_se3"]
    assert np.abs(a["d_se3"] - 10 * b["d_se3"]).max() <= C.allowance(10 * ref, 0.0)
    assert np.all(a["d_se3"][3] == 0)


def test_repeated_ids_sum_in_index_order_with_the_same_bits():
    rng = np.random.default_rng(4)
    n, Tn = 257, 65
    rows = rng.normal(size=(n, 7)).astype(np.float32)
    for ids in (np.full(n, 7), rng.integers(0, Tn, size=n), np.arange(n) % 3):
        want = rn.id_rows_sum(rows, ids, Tn, dtype=np.float32)                 # the index-order fp32 sum
        a = np_(FD.id_rows_sum(T(rows), ids_t(ids), Tn))
        b = np_(FD.id_rows_sum(T(rows), ids_t(ids, torch.int32), Tn, lanes=64))   # twice the workgroups
        c = np_(FD.id_rows_sum(T(rows), ids_t(ids), Tn, lanes=128))
        assert np.array_equal(a, want) and np.array_equal(b, want) and np.array_equal(c, want)
        assert np.all(a[np.setdiff1d(np.arange(Tn), ids)] == 0)
    big = rng.integers(0, 3, size=2500)                                        # more than two id tiles
    rows = rng.normal(size=(2500, 4)).astype(np.float32)
    assert np.array_equal(np_(FD.id_rows_sum(T(rows), ids_t(big), 3)), rn.id_rows_sum(rows, big, 3, dtype=np.float32))
    # through autograd: every id equal, two runs, the same bits
    se3 = rng.normal(size=(Tn, 6)).astype(np.float32)
    g = rng.normal(size=(n, 4, 4)).astype(np.float32)
    delta = rng.normal(size=(n, 6)).astype(np.float32) * 0.1
    r1 = tail(se3=se3, ids=np.full(n, 7), delta=delta, g=g)[2]["d_se3"]
    r2 = tail(se3=se3, ids=np.full(n, 7), delta=delta, g=g)[2]["d_se3"]
    assert np.array_equal(r1, r2) and np.all(r1[np.arange(Tn) != 7] == 0) and np.all(r1[7] != 0)


def test_ids_out_of_range_are_counted_and_refused():
    rng = np.random.default_rng(5)
    Tn, n = 9, 12
    se3 = rng.normal(size=(Tn, 7)).astype(np.float32)
    delta = rng.normal(size=(n, 6)).astype(np.float32) * 0.1
    ks = (np.abs(rng.normal(size=(2, 4))) + 3).astype(np.float32)
    ids = rng.integers(0, Tn, size=n)
    good = tail(se3=se3, ids=ids, delta=delta, ks=ks, dataid=np.zeros(n, np.int64), g=np.ones((n, 4, 4), np.float32))
    bad_ids = ids.copy()
    bad_ids[2], bad_ids[9] = -1, Tn
    dataid = np.zeros(n, np.int64)
    dataid[5] = 2
    rtk, status, grads = tail(se3=se3, ids=bad_ids, delta=delta, ks=ks, dataid=dataid, g=np.ones((n, 4, 4), np.float32))
    assert status.tolist() == [2, 1, 0, 0]
    assert np.all(np.isnan(rtk[[2, 9]])) and np.all(np.isnan(rtk[5, 3])) and np.all(np.isfinite(rtk[5, :3]))
    keep = np.setdiff1d(np.arange(n), [2, 9])
    assert np.array_equal(rtk[keep][:, :3], good[0][keep][:, :3])
    assert np.all(grads["d_delta"][[2, 9]] == 0) and np.array_equal(grads["d_delta"][keep], good[2]["d_delta"][keep])
    assert np.all(np.isfinite(grads["d_se3"])) and np.all(np.isfinite(grads["d_ks"]))
    # the modules refuse the same way
    m = FD.RTExplicit(Tn).to(DEV)
    out = m(ids_t(bad_ids))
    assert np_(m.id_status).tolist() == [2, 0, 0, 0] and np.all(np.isnan(np_(out)[[2, 9]])) and np.all(np.isfinite(np_(out)[keep]))


# ---- the modules -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,use_quat", [("rthead_q", True), ("rthead_w", False)])
def test_rthead_matches_the_restatement_and_the_reference(tag, use_quat):
    g32, rep = golden("g32_root_pose"), []
    n_out = 7 if use_quat else 6
    p = C.head_params(tag, n_out)
    head = FD.RTHead(use_quat=use_quat, out_channels=n_out, raw_feat=True, **C.HEAD_KW)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    head = head.to(DEV).train()
    x = T(g32["x"]).requires_grad_(True)
    out = head(x)
    (T(g32[tag + "_w"]) * out).sum().backward()
    rows = rn.mlp(p, g32["x"])
    ref = rn.root_pose(delta=rows, raw="none", g=rn.rts12_bwd(g32[tag + "_w"].astype(np.float64)))
    _, grads = rn.mlp(p, g32["x"], g=ref["d_delta"])
    check(tag + " out", np_(out), rn.rts12(ref["rtk"]), g32[tag + "_dref_out"], rep)
    check(tag + " d_x", np_(x.grad), grads["d_x"], g32[tag + "_dref_d_x"], rep)
    check(tag + " d_rgb", np_(head.rgb[0].weight.grad), grads["rgb.0.weight"], g32[tag + "_dref_d_rgb"], rep)
    assert rel_err(np_(out), g32[tag + "_out_32"]) <= 1e-4 and rel_err(np_(x.grad), g32[tag + "_d_x_32"]) <= 1e-4
    # the `mlp` basis by composition: nn.Sequential(nn.Embedding, RTHead) through compute_rts
    emb = torch.nn.Embedding(8, C.CODE).to(DEV)
    emb.weight.data = T(g32["x"])
    rt = RP.compute_rts(torch.nn.Sequential(emb, head), 8)
    want = rn.root_pose(delta=rows, raw="base")["rtk"][:, :3]
    check(tag + " mlp basis", np_(rt), want, g32[tag + "_dref_out"], rep)


def _expmlp(delta):
    m = FD.RTExpMLP(C.T, C.NUM_FREQS, C.CODE, np.asarray(C.DATA_OFFSET), delta=delta)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in C.expmlp_state(delta).items()}, strict=True)
    return m.to(DEV).train()


def _expmlp_ref(m, delta, ids, **kw):
    """The float64 restatement from the module's own fp32 frame code (as the fixture's float64 record starts)."""
    sd = C.expmlp_state(delta)
    mlp_p = {k[len("mlp_rt."):]: v for k, v in sd.items() if k.startswith("mlp_rt.")}
    with torch.no_grad():
        code = np_(m.root_code(ids_t(ids))).astype(np.float64)
    return mlp_p, code, rn.mlp(mlp_p, code), sd["base_rt.se3"]


@pytest.mark.parametrize("tag,delta", [("expmlp_q", False), ("expmlp_w", True)])
def test_rtexpmlp_and_checkpoint_match_the_restatement_and_the_reference(tag, delta):
    g32, rep = golden("g32_root_pose"), []
    from moda_amd import checkpoint
    states = {"nerf_root_rts." + k: torch.from_numpy(v) for k, v in C.expmlp_state(delta).items()}
    assert set(k[len("nerf_root_rts."):] for k in states) == set(str(k) for k in g32["expmlp_keys"])
    states["ks_param"] = torch.tensor([[300., 500., 200., 250.], [310., 510., 210., 260.]])
    built = checkpoint.build_root_pose(states, C.DATA_OFFSET, device=DEV)
    m = built["nerf_root_rts"].train()
    assert isinstance(m, FD.RTExpMLP) and m.base_rt.delta == delta and built["ks_param"].shape == (2, 4)
    out = m(ids_t(C.IDS))
    (T(g32[tag + "_w"]) * out).sum().backward()
    assert rel_err(np_(m.root_code(ids_t(C.IDS))), g32[tag + "_code_32"]) <= 1e-5
    for ids in (C.IDS, np.arange(C.T), np.asarray([64, 0, 40, 39])):      # the tabulated code has FrameCode.forward's own bits
        assert torch.equal(m.root_code(ids_t(ids)), FD.FrameCode.forward(m.root_code, ids_t(ids)))
    mlp_p, code, rows, se3 = _expmlp_ref(m, delta, C.IDS)
    ref = rn.root_pose(se3=se3, ids=C.IDS, delta=rows, raw="none", g=rn.rts12_bwd(g32[tag + "_w"].astype(np.float64)))
    _, grads = rn.mlp(mlp_p, code, g=ref["d_delta"])
    check(tag + " out", np_(out), rn.rts12(ref["rtk"]), g32[tag + "_dref_out"], rep)
    check(tag + " d_se3", np_(m.base_rt.se3.grad), ref["d_se3"], g32[tag + "_dref_d_se3"], rep)
    check(tag + " d_rgb", np_(m.mlp_rt.rgb[0].weight.grad), grads["rgb.0.weight"], g32[tag + "_dref_d_rgb"], rep)
    assert rel_err(np_(out), g32[tag + "_out_32"]) <= 1e-4
    assert rel_err(np_(m.base_rt.se3.grad), g32[tag + "_d_se3_32"]) <= 1e-4
    assert rel_err(np_(m.mlp_rt.rgb[0].weight.grad), g32[tag + "_d_rgb_32"]) <= 1e-4
    # the `exp` basis from a checkpoint
    e = checkpoint.build_root_pose({"nerf_root_rts.se3": torch.from_numpy(C.se3_table(delta, 8))}, C.DATA_OFFSET, device=DEV)
    assert isinstance(e["nerf_root_rts"], FD.RTExplicit) and e["nerf_root_rts"].delta == delta and e["ks_param"] is None


def test_refine_rt_helpers_and_ray_cams():
    g32, rep = golden("g32_root_pose"), []
    raw, root, kaug = g32["refine_rt_raw"], g32["refine_root"], g32["kaug"]
    assert rel_err(np_(GU.refine_rt(T(raw), T(root))), g32["refine_out_32"]) <= 1e-6
    assert np.array_equal(np_(GU.create_base_se3(3, DEV)), g32["base_se3"])
    assert rel_err(np_(GU.K2inv(T(kaug))), g32["cams_K2inv_32"]) <= 1e-6
    assert rel_err(np_(GU.Kmatinv(GU.K2mat(T(raw[:, 3])))), g32["cams_Kmatinv_32"]) <= 1e-6
    assert np.array_equal(np_(GU.mat2K(GU.K2mat(T(raw[:, 3])))), raw[:, 3])
    r = T(raw).requires_grad_(True)
    Rm, Tm, Ki = GU.prepare_ray_cams(r, T(kaug))
    ((T(g32["cams_wR"]) * Rm).sum() + (T(g32["cams_wT"]) * Tm).sum() + (T(g32["cams_wK"]) * Ki).sum()).backward()
    ref = rn.ray_cams(raw, kaug, g32["cams_wR"].astype(np.float64), g32["cams_wT"].astype(np.float64), g32["cams_wK"].astype(np.float64))
    assert np.array_equal(np_(Rm), raw[:, :3, :3]) and np.array_equal(np_(Tm), raw[:, :3, 3])
    check("Kinv", np_(Ki), ref["Kinv"], g32["cams_dref_Kinv"], rep)
    d = np_(r.grad)
    assert np.array_equal(d[:, :3, :3], g32["cams_wR"]) and np.array_equal(d[:, :3, 3], g32["cams_wT"])
    d_ref_k = np.abs(g32["cams_d_rtk_32"][:, 3].astype(np.float64) - g32["cams_d_rtk_64"][:, 3]).max()   # the K row on its own scale
    check("d_rtk K row", d[:, 3], ref["d_rtk"][:, 3], d_ref_k, rep)
    assert raw[0, 3, 0] != raw[0, 3, 1] and np.all(kaug[:, 0] != kaug[:, 1])                          # fx != fy, a non-trivial kaug
    assert rel_err(np_(Ki), g32["cams_Kinv_32"]) <= 1e-4 and rel_err(d[:, 3], g32["cams_d_rtk_32"][:, 3]) <= 1e-4


def test_chain_into_raycast():
    """convert_root_pose -> prepare_ray_cams -> raycast -> sum(w_o rays_o + w_d rays_d), 4 frames x 8 pixels; d_ref of every output
    from the reference's own run of this chain (fixture keys chain_*)."""
    g32, rep = golden("g32_root_pose"), []
    m = _expmlp(False)
    c = C.chain_case()
    fid, did, ks0, xys, wd, wo = (c[k] for k in ("fid", "did", "ks", "xys", "wd", "wo"))
    ks = torch.nn.Parameter(T(ks0))
    kaug = g32["kaug"][:4]
    rtk = RP.convert_root_pose(m, ids_t(fid), ids_t(did), ks)
    assert rtk.shape == (4, 4, 4) and np_(m.id_status).tolist() == [0, 0, 0, 0]
    rays = FD.raycast(T(xys), *GU.prepare_ray_cams(rtk, T(kaug)), None)
    ((T(wd) * rays["rays_d"]).sum() + (T(wo) * rays["rays_o"]).sum()).backward()
    mlp_p, code, rows, se3 = _expmlp_ref(m, False, fid)
    fwd = rn.convert_root_pose(se3, rows, fid, did, ks0)
    cams = rn.ray_cams(fwd["rtk"], kaug)
    rc = rn.raycast(xys, cams["Rmat"], cams["Tmat"], cams["Kinv"], wd.astype(np.float64), wo.astype(np.float64))
    d_rtk = rn.ray_cams(fwd["rtk"], kaug, rc["d_Rmat"], rc["d_Tmat"], rc["d_Kinv"])["d_rtk"]
    ref = rn.convert_root_pose(se3, rows, fid, did, ks0, g=d_rtk)
    _, grads = rn.mlp(mlp_p, code, g=ref["d_delta"])
    check("chain rays_d", np_(rays["rays_d"]), rc["rays_d"], g32["chain_dref_out"], rep)
    check("chain rays_o", np_(rays["rays_o"]), rc["rays_o"], g32["chain_dref_rays_o"], rep)
    check("chain d_se3", np_(m.base_rt.se3.grad), ref["d_se3"], g32["chain_dref_d_se3"], rep)
    check("chain d_rgb", np_(m.mlp_rt.rgb[0].weight.grad), grads["rgb.0.weight"], g32["chain_dref_d_rgb"], rep)
    check("chain d_ks", np_(ks.grad), ref["d_ks"], g32["chain_dref_d_ks"], rep)
    assert rel_err(np_(rays["rays_d"]), g32["chain_out_32"]) <= 1e-4 and rel_err(np_(ks.grad), g32["chain_d_ks_32"]) <= 1e-4
    # use_cam: the dataset's poses, scaled; the input is not modified
    raw = g32["refine_rt_raw"][:4].copy()
    raw_t = T(raw)
    rtk2 = RP.convert_root_pose(m, ids_t(fid), ids_t(did), ks, rtk=raw_t, obj_scale=2.0)
    want = rn.convert_root_pose(se3, rows, fid, did, ks0, rtk=raw, obj_scale=2.0)["rtk"]
    check("use_cam rtk", np_(rtk2)[:, :3], want[:, :3], g32["expmlp_q_dref_out"], rep)
    assert np.array_equal(np_(rtk2)[:, 3], ks0[did])
    assert np.array_equal(np_(raw_t), raw)


def test_compute_rts_captured_with_root_smoothness_replays_the_eager_bits():
    """Bit for bit: what the root-pose kernels write -- the pose table, the loss on it, d_delta and d_se3.  The MLP's own gradients
    are compared too, but only to rounding: its bias gradients come from LinearFn's column sum, whose workgroups add with float
    atomics in whatever order they run, so they are not the same bits from run to run, eager or replayed.
    Nothing that holds an autograd graph outlives a step: a kept graph keeps the parameters' gradient-accumulation nodes alive, and
    those run on the stream of the call that created them -- inside a later capture that is a stream which is not capturing (the
    choreography of bench_support.TrainHarness.capture)."""
    from moda_amd.loss_utils import compute_root_sm_2nd_loss
    m = _expmlp(False)
    params = [p for p in m.parameters()]
    raw_rows, kept = m.mlp_rt.raw, {}

    def raw(x):
        y = raw_rows(x)
        y.retain_grad()
        kept["delta"] = y
        return y
    m.mlp_rt.raw = raw

    def step():
        for p in params:
            p.grad = None
        rt = RP.compute_rts(m, C.T)
        loss = compute_root_sm_2nd_loss(rt, C.DATA_OFFSET)
        loss.backward()
        return rt.detach(), loss.detach(), kept.pop("delta").grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                                                # builds the code table and the offset table
            rt, loss, _ = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert rt.shape == (C.T, 3, 4) and np.isfinite(float(loss))
    used = [p for p in params if p.grad is not None]
    static = [torch.zeros_like(p) for p in used]
    for p in params:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                         # on a side stream of its own
        rt_g, loss_g, dd_g = step()
        for s, p in zip(static, used):
            s.copy_(p.grad)
    torch.cuda.synchronize()
    with torch.no_grad():                                                 # a parameter update between capture and replay
        m.base_rt.se3.add_(T(C.synth.normal(C.SEED, "g32/upd", tuple(m.base_rt.se3.shape))) * 0.05)
        m.mlp_rt.rgb[0].weight.mul_(1.5)
    rt_e, loss_e, dd_e = step()
    eager = [p.grad.clone() for p in used]
    assert float(m.base_rt.se3.grad.abs().max()) > 0 and float(dd_e.abs().max()) > 0
    i_se3 = [i for i, p in enumerate(used) if p is m.base_rt.se3][0]
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(rt_g, rt_e) and torch.equal(loss_g, loss_e) and torch.equal(dd_g, dd_e)
        assert torch.equal(static[i_se3], eager[i_se3])
        for s, e in zip(static, eager):
            assert rel_err(np_(s), np_(e)) <= 1e-5


def test_harness_trains_the_root_poses():
    from moda_amd import bench_support as BS
    kw = dict(N=64, S=16, B=5, precision="bf16", rays_per_frame=4, default_losses=True)
    h = BS.TrainHarness(root_pose=True, **kw)
    before = h.root_rts.base_rt.se3.detach().clone()
    h.eager_step()
    first, first_root = h.loss(), float(h.aux_out["root_sm_loss"])
    h.eager_step()
    torch.cuda.synchronize()
    assert np.isfinite(h.loss()) and np.isfinite(float(h.aux_out["root_rot_sm"])) and np.isfinite(first_root) and first_root > 0
    assert not torch.equal(before, h.root_rts.base_rt.se3.detach())
    assert any(n.startswith("nerf_root_rts.base_rt.se3") for n, _ in h.named_params())
    h.capture(warm=1)                                                     # the captured step runs compute_rts too
    mid = h.root_rts.base_rt.se3.detach().clone()
    h.step()
    torch.cuda.synchronize()
    assert np.isfinite(h.loss()) and np.isfinite(float(h.aux_out["root_rot_sm"])) and not torch.equal(mid, h.root_rts.base_rt.se3.detach())
    # off (the default) nothing of it exists, and the flag touches nothing else: both harnesses see the same rays and the same
    # parameters in their first step, so the two first losses differ by the root-smoothness term and by the roundings of two fp32
    # sums of about a dozen terms taken in different order (half an ulp a term, each way: 16 ulp)
    h0 = BS.TrainHarness(**kw)
    assert h0.root_rts is None and not h0.loss_opts["root_sm"] and not any("root" in n for n, _ in h0.named_params())
    assert len(h0.params) == len(h.params) - len(list(h.root_rts.parameters()))
    h0.eager_step()
    assert abs((first - first_root) - h0.loss()) <= 16 * float(np.spacing(np.float32(first)))
