"""GPU checks of the warm-up stages (moda_amd/warmup.py, csrc/warmup_kernels.hip) against the float64 oracle tests/warmup_numpy.py
within the bounds it derives, and against the reference's records in tests/golden/g36_warmup.npz.  Sizes: N around the wave (64)
and workgroup (256) seams and the reference's 10 000 once; T around 64 and past 256; videos of 1, 2, 3 and 70 frames."""
import numpy as np
import pytest
import torch

import moda_amd
import warmup_numpy as O
from helpers import rel_err
from moda_amd import geom_utils, loss_utils, warmup
from moda_amd import autograd as A
from test_warmup_oracle import G, MODES, obj_bound, quat_cases

pytestmark = pytest.mark.gpu
SEAMS = (1, 63, 64, 65, 255, 256, 257)
ANISO = np.asarray([0.11, 0.045, 0.3], np.float32)
BF = 2.4


@pytest.fixture(autouse=True)
def exact_fp32_training():
    prev = moda_amd.get_train_precision()
    moda_amd.set_train_precision("fp32")
    yield
    moda_amd.set_train_precision(prev)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def within(got, want, bound):
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    assert (err <= bound).all(), (int((err > bound).sum()), float(err.max()), float(np.max(bound)))


def uniforms(n, kind):
    if kind == "zeros":
        return np.zeros((n, 3), np.float32)
    if kind == "ones":                                                       # one ulp below 1: the far corner of the box
        return np.full((n, 3), np.nextafter(np.float32(1), np.float32(0)), np.float32)
    return np.random.default_rng(n).random((n, 3), dtype=np.float32)


# ---- moda_shape_target and the loss pair ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ellips", [True, False])
@pytest.mark.parametrize("n,kind", [(n, "rand") for n in SEAMS + (10000,)] + [(65, "zeros"), (65, "ones")])
def test_shape_target_and_loss(n, kind, ellips):
    u = uniforms(n, kind)
    val, b = O.shape_target(u, ANISO, BF, ellips)
    pts, dis = loss_utils.shape_targets(dev(u), dev(ANISO), BF, ellips)
    assert pts.shape == (1, n, 3) and np.array_equal(host(pts)[0], val["pts"])                      # bit for bit
    within(host(dis), val["dis"], b["dis"])
    y = (np.random.default_rng(n + 1).standard_normal(n) * 0.1).astype(np.float32)
    lv, lb = O.shape_loss(y, host(dis), g=0.7)
    yt = dev(y).requires_grad_(True)
    dy_sum = torch.full((1,), 7.0, device="cuda")
    loss = A.ShapeLossFn.apply(yt, dis, dy_sum)
    (loss * 0.7).backward()
    within(float(loss.detach()), lv["loss"], lb["loss"])
    within(host(yt.grad), lv["dy"], lb["dy"])
    exact = host(yt.grad).astype(np.float64).sum()                           # the fp32 dy summed in float64, rounded once
    assert abs(float(dy_sum) - exact) <= O.U32 * abs(exact) + 1e-45
    pts2, dis2 = loss_utils.shape_targets(dev(u), dev(ANISO), BF, ellips)                          # the same bits on every run
    yt2 = dev(y).requires_grad_(True)
    dy_sum2 = torch.zeros((1,), device="cuda")
    loss2 = A.ShapeLossFn.apply(yt2, dis2, dy_sum2)
    (loss2 * 0.7).backward()
    assert torch.equal(pts, pts2) and torch.equal(dis, dis2) and torch.equal(loss, loss2) and torch.equal(yt.grad, yt2.grad)
    assert torch.equal(dy_sum, dy_sum2)


def test_shape_loss_past_the_partial_buffer():
    """More 256-element tiles than MODA_SHAPE_LOSS_MAX_BLOCKS: workgroups stride over the input."""
    n = 256 * A.SHAPE_LOSS_MAX_BLOCKS + 300
    rng = np.random.default_rng(9)
    y, dis = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    lv, lb = O.shape_loss(y, dis)
    within(float(A.ShapeLossFn.apply(dev(y), dev(dis))), lv["loss"], lb["loss"])


# ---- rtk_loss -------------------------------------------------------------------------------------------------------------------
def pose_table(rng, T, rows=4):
    out = np.zeros((T, rows, 4), np.float32)
    out[:, :3, :3] = O.random_rotations(rng, T)
    out[:, :3, 3] = rng.standard_normal((T, 3)) * 0.3
    if rows == 4:
        out[:, 3] = (500, 500, 256, 256)
    return out


def check_rtk(pred, raw):
    aux = {}
    p = dev(pred).requires_grad_(True)
    total = loss_utils.rtk_loss(p, dev(raw), aux)
    val, b = O.rtk_loss(pred, raw, (1.0, 0.5, 0.0))
    (total + 0.5 * aux["rot_loss"]).backward()
    for k, got in (("total", total), ("rot_loss", aux["rot_loss"]), ("trn_loss", aux["trn_loss"])):
        within(float(got), val[k], b[k])
    within(host(p.grad), val["drtk"], b["drtk"])
    return host(p.grad), val


@pytest.mark.parametrize("T", [1, 2, 64, 65, 300])
@pytest.mark.parametrize("rows", [4, 3])
def test_rtk_loss(T, rows):
    rng = np.random.default_rng(T)
    pred, raw = pose_table(rng, T, rows), pose_table(rng, T, 4)
    if T >= 2:
        pred[0, :3, :3] = raw[0, :3, :3]                                      # clamp active at the top: zero rotation gradient
        pred[1, :3, :3] = (raw[1, :3, :3].astype(np.float64) @ np.diag([-1., 1., -1.])).astype(np.float32)      # 180 degrees: the bottom
    grad, val = check_rtk(pred, raw)
    if T >= 2:
        assert (grad[:2, :3, :3] == 0).all() and (val["drtk"][:2, :3, :3] == 0).all()
    if rows == 4:
        assert (grad[:, 3] == 0).all()


def test_rtk_loss_golden_case():
    check_rtk(G["rtk/pred"], G["rtk/raw"])
    aux = {}
    p = dev(G["rtk/pred"]).requires_grad_(True)
    total = loss_utils.rtk_loss(p, dev(G["rtk/raw"]), aux)
    aux["rot_loss"].backward()
    _, b = O.rtk_loss(G["rtk/pred"], G["rtk/raw"], (0.0, 1.0, 0.0))
    within(host(p.grad), G["rtk/f64/d_rot"], b["drtk"])
    within(float(total), G["rtk/f64/total"], b["total"])


# ---- compute_root_sm_loss -------------------------------------------------------------------------------------------------------
def check_sm(rtk, offsets):
    p = dev(rtk).requires_grad_(True)
    loss, parts = loss_utils.root_sm1_parts(p, offsets)
    (loss * 1.3).backward()
    val, b = O.root_sm_loss(rtk, offsets, g=1.3)
    assert int(parts[2]) == val["pairs"]
    if val["pairs"] == 0:
        assert np.isnan(float(loss)) and (host(p.grad) == 0).all()
        return host(p.grad)
    within(float(loss), val["loss"], b["loss"])
    within(float(parts[0]), val["rot"], b["rot"])
    within(float(parts[1]), val["trn"], b["trn"])
    within(host(p.grad), val["drtk"], b["drtk"])
    assert float(loss_utils.compute_root_sm_loss(dev(rtk), offsets)) == float(loss)
    return host(p.grad)


@pytest.mark.parametrize("rows", [4, 3])
def test_root_sm_loss_short_and_long_videos(rows):
    rng = np.random.default_rng(70)
    rtk = pose_table(rng, 76, rows)                                           # videos of 1, 2, 3 and 70 frames
    rtk[20] = rtk[19]                                                         # a repeated frame: zero difference
    grad = check_sm(rtk, (0, 1, 3, 6, 76))
    assert np.isfinite(grad).all() and (grad[0] == 0).all()
    check_sm(rtk[:6], (0, 1, 3, 6))
    check_sm(np.stack([rtk[0], rtk[0], rtk[1]]), (0, 3))
    check_sm(rtk[:72], (0, 1, 2, 3))                                    # frames past the last video belong to none
    check_sm(rtk[:3], (0, 1, 2, 3))                                           # no pair at all: NaN, zero gradient


def test_root_sm_loss_golden_case():
    check_sm(G["sm/rtk"], tuple(int(v) for v in G["sm/data_offset"]))
    p = dev(G["sm/rtk"]).requires_grad_(True)
    loss = loss_utils.compute_root_sm_loss(p, G["sm/data_offset"])
    loss.backward()
    _, b = O.root_sm_loss(G["sm/rtk"], G["sm/data_offset"])
    within(float(loss), G["sm/f64/loss"], b["loss"])
    within(host(p.grad), G["sm/f64/d"], b["drtk"])


# ---- matrix_to_quaternion and the preset ----------------------------------------------------------------------------------------
def test_matrix_to_quaternion_round_trip():
    R = quat_cases()
    q = host(geom_utils.matrix_to_quaternion(dev(R)))
    assert (q[:, 0] >= 0).all()
    assert np.abs(O.quaternion_to_matrix(q) - R).max() <= O.ROUNDTRIP_F32
    want = O.matrix_to_quaternion(R)
    flip = np.where((q * want).sum(-1, keepdims=True) < 0, -1.0, 1.0)        # a half turn's sign is free (real part 0 on both sides)
    assert (np.abs(want[:, 0]) < 1e-6)[flip[:, 0] < 0].all()
    assert np.abs(q * flip - want).max() <= (14.6 + 2.3) * O.U32
    rtk = np.zeros((len(R), 4, 4), np.float32)
    rtk[:, :3, :3] = R
    assert torch.equal(geom_utils.matrix_to_quaternion(dev(rtk)[:, :3, :3]), dev(q))       # the strided view, no copy


def test_preset_root_rotations():
    T = 65
    rng = np.random.default_rng(3)
    rtk = pose_table(rng, T)
    root = moda_amd.RTExpMLP(T, 6, 128, [0, 30, T]).cuda()
    with torch.no_grad():
        root.mlp_rt.rgb[0].weight.zero_()                                     # a zero-initialised tail: the delta is the identity
        root.mlp_rt.rgb[0].bias.zero_()
    warmup.preset_root_rotations(root, dev(rtk))
    with torch.no_grad():
        got = host(moda_amd.compute_rts(root, T))
    assert np.abs(got[:, :3, :3] - rtk[:, :3, :3]).max() <= O.ROUNDTRIP_F32 + 16 * O.U32      # + quat_to_mat and one product in fp32
    assert (host(root.base_rt.se3)[:, :3] == 0).all()
    state = moda_amd.FrameState(T)
    state.rtk.copy_(dev(rtk))
    before = host(root.base_rt.se3).copy()
    warmup.preset_root_rotations(root, state)
    assert np.array_equal(host(root.base_rt.se3), before)
    for other in (moda_amd.RTExplicit(T).cuda(), torch.nn.Linear(2, 2).cuda()):
        with pytest.raises(NotImplementedError, match="expmlp"):
            warmup.preset_root_rotations(other, dev(rtk))
    with pytest.raises(ValueError, match="rtk"):
        warmup.preset_root_rotations(root, dev(rtk[:5]))
    with pytest.raises(ValueError, match="rtk"):
        warmup.preset_root_rotations(root, dev(rtk).double())


# ---- shape_init_loss end to end -------------------------------------------------------------------------------------------------
def golden_net():
    net = moda_amd.NeRF(D=5, W=64, in_channels_xyz=63)
    sd = {k[len("shape/w/"):]: torch.from_numpy(G[k]) for k in G.files if k.startswith("shape/w/")}
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and all("xyz_encoding" not in k and "sigma" not in k for k in missing)
    return net.cuda().train(), moda_amd.Embedding(3, 10)


@pytest.mark.parametrize("mode,ellips", MODES)
def test_shape_init_loss_against_the_reference_run(mode, ellips):
    """The reference's fp32 run with its u and weights; y at 5e-6 and parameter gradients at 1e-4 (rel-L2), the bars
    tests/test_gpu_grad.py holds NeRF.train_forward to in the exact fp32 training precision."""
    net, emb = golden_net()
    pre = f"shape/{mode}/f32/"
    u = dev(G[f"shape/{mode}/u"])
    loss = moda_amd.shape_init_loss(dev(G["shape/pts"]), None, net, emb, float(G["shape/bound_factor"]), ellips, u=u)
    loss.backward()
    assert rel_err(np.asarray(float(loss)), G[pre + "loss"]) < 5e-6
    with torch.no_grad():
        pts, _ = loss_utils.shape_targets(u, dev(obj_bound()), float(G["shape/bound_factor"]), ellips)
        assert np.array_equal(host(pts)[0], G[pre + "pts_samp"])
        assert rel_err(host(net.fused(pts, sigma_only=True)).reshape(-1), G[pre + "y"]) < 1e-4      # the inference route: its own bar
        loss_ng = moda_amd.shape_init_loss(dev(G["shape/pts"]), None, net, emb, float(G["shape/bound_factor"]), ellips, u=u,
                                           obj_bound=dev(obj_bound()))
    assert rel_err(np.asarray(float(loss_ng)), G[pre + "loss"]) < 1e-4
    for name, p in net.named_parameters():
        used = name.startswith("sigma.") or (name.startswith("xyz_encoding_") and "final" not in name)
        if not used:
            assert p.grad is None, name                                       # dir / rgb layers and beta: not evaluated
            continue
        assert p.grad is not None and float(p.grad.abs().max()) > 0, name
        if ellips:
            e = rel_err(host(p.grad), G[pre + "d/" + name])
            assert e < 1e-4, (name, e)


def test_shape_init_loss_draws_and_refuses():
    net, emb = golden_net()
    pts = dev(G["shape/pts"])
    a = moda_amd.shape_init_loss(pts, None, net, emb, 2.4, nsample=64)
    b = moda_amd.shape_init_loss(pts, None, net, emb, 2.4, nsample=64)
    assert np.isfinite(float(a)) and float(a) != float(b)                     # fresh points each call
    with pytest.raises(NotImplementedError, match="u"):
        moda_amd.shape_init_loss(pts, None, net, emb, 2.4, u=torch.rand(8, 3, device="cuda", requires_grad=True))
    with pytest.raises(ValueError, match="u"):
        moda_amd.shape_init_loss(pts, None, net, emb, 2.4, u=torch.rand(8, 3, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError, match="u"):
        moda_amd.shape_init_loss(pts, None, net, emb, 2.4, u=torch.rand(3, 8, device="cuda").t())
    with pytest.raises(ValueError, match="obj_bound"):
        moda_amd.shape_init_loss(pts, None, net, emb, 2.4, obj_bound=torch.ones(1, 3, device="cuda"))
    with pytest.raises(ValueError, match="rtk_raw"):
        loss_utils.rtk_loss(torch.zeros(3, 4, 4, device="cuda"), torch.zeros(2, 4, 4, device="cuda"), {})
    with pytest.raises(ValueError, match="rtk_all"):
        loss_utils.compute_root_sm_loss(torch.zeros(3, 4, 3, device="cuda"), (0, 3))


def test_forward_warmup_shape():
    net, emb = golden_net()

    class Model:
        dp_verts_unit, dp_faces, nerf_coarse, embedding_xyz = dev(G["shape/pts"]) * 10, None, net, emb
    u = dev(G["shape/ellips/u"])
    loss, aux = warmup.forward_warmup_shape(Model, dict(bound_factor=2, init_ellips=True), u=u)
    assert set(aux) == {"shape_init_loss"} and aux["shape_init_loss"] is loss
    assert rel_err(np.asarray(float(loss)), G["shape/ellips/f32/loss"]) < 1e-4        # (pts * 10 * 0.1 rounds once more)


# ---- WarmupHarness --------------------------------------------------------------------------------------------------------------
def harness(seed=11):
    torch.manual_seed(5)
    net = moda_amd.NeRF(D=5, W=64, in_channels_xyz=63).cuda().train()
    verts = dev(G["shape/pts"]) * 10
    return warmup.WarmupHarness(net, moda_amd.Embedding(3, 10), verts, dict(warmup_shape_ep=5, bound_factor=2, init_ellips=True),
                                steps_per_epoch=8, seed=seed, nsample=256)


def test_warmup_harness_replays_learn_on_new_points():
    a = harness()
    a.step()
    first = a.loss()
    a.capture(warm=2)
    sums = []
    for _ in range(17):
        a.step()
        sums.append(float(a.u.double().sum()))
    assert a.steps_done == 20 and a.graph is not None and int(a.opt.step_count) == 20
    assert len(set(sums)) == len(sums)                                        # the replayed graph saw new points each step
    assert a.loss() < first
    assert int(a.clipper.status[0]) == 0 and int(a.opt.status[0]) == 0
    a.run()
    assert a.steps_done == 40


def test_warmup_stage_kernels_replay_bit_for_bit():
    """Everything this stage adds around the network -- targets, the loss pair, rtk_loss, compute_root_sm_loss, forward and
    backward -- captured as one graph and replayed on refilled inputs, against the same calls made eagerly."""
    rng = np.random.default_rng(4)
    u, y = torch.zeros(300, 3, device="cuda"), torch.zeros(300, device="cuda", requires_grad=True)
    pred = dev(pose_table(rng, 70)).requires_grad_(True)
    raw, ob = dev(pose_table(rng, 70)), dev(ANISO)
    loss_utils._offset_table((0, 1, 3, 70), 70, pred.device)                  # uploaded once, before the capture

    def body():
        _, dis = loss_utils.shape_targets(u, ob, BF, True)
        aux = {}
        total = A.ShapeLossFn.apply(y, dis) + loss_utils.rtk_loss(pred, raw, aux) + 0.1 * aux["rot_loss"] \
            + loss_utils.compute_root_sm_loss(pred, (0, 1, 3, 70))
        gy, gp = torch.autograd.grad(total, [y, pred])
        return torch.cat([total.reshape(1), dis, gy, gp.reshape(-1)])

    def fill(k):
        g = torch.Generator(device="cuda").manual_seed(k)
        u.uniform_(generator=g)
        with torch.no_grad():
            y.normal_(generator=g)
    fill(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = body()
    for k in (1, 2, 3):
        fill(k)
        graph.replay()
        got = out.clone()
        assert torch.equal(got, body()) and bool(torch.isfinite(got).all())


def test_warmup_harness_eager_and_replayed():
    """20 eager steps and 20 replayed steps from the same seed leave bit-identical parameters (the warm-up steps that precede the
    capture are undone by restore=True, so all 20 compared steps are replays).  Exact fp32 training precision, 256 points: below
    the 512 at which the network's weight-gradient GEMMs split their reduction over atomically adding workgroups; sigma.bias's
    gradient, which the network's backward adds with float atomics at every size, is the fixed-order sum the harness writes."""
    a, b = harness(), harness()
    for _ in range(20):
        a.step()
    b.capture(warm=3, restore=True)
    assert b.steps_done == 0 and int(b.opt.step_count) == 0
    for _ in range(20):
        b.step()
    assert a.steps_done == b.steps_done == 20 and b.graph is not None
    assert torch.equal(a.u, b.u)
    for (name, pa), (_, pb) in zip(a.named, b.named):
        assert torch.equal(pa.detach(), pb.detach()), name
    assert a.loss() == b.loss()
    assert torch.equal(a.opt.exp_avg, b.opt.exp_avg) and torch.equal(a.opt.exp_avg_sq, b.opt.exp_avg_sq)


def test_warmup_harness_sigma_bias_gradient_is_the_ordered_sum():
    h = harness()
    h.step()
    assert torch.equal(h.sigma_bias.grad.reshape(1), h.dy_sum) and float(h.dy_sum) != 0.0


# ---- forward_warmup_rootmlp -----------------------------------------------------------------------------------------------------
def test_forward_warmup_rootmlp():
    T = 40
    rng = np.random.default_rng(8)
    state = moda_amd.FrameState(T)
    state.rtk.copy_(dev(pose_table(rng, T)))

    class Model:
        nerf_root_rts = moda_amd.RTExpMLP(T, 6, 128, [0, 15, T]).cuda()
        num_fr, data_offset, latest_vars, use_cam, obj_scale = T, [0, 15, T], state, False, 1.0
    total, aux = warmup.forward_warmup_rootmlp(Model, dict(root_opt=True))
    assert set(aux) == {"rot_loss", "warmup_root_sm_loss"}
    total.backward()
    grads = {n: p.grad for n, p in Model.nerf_root_rts.named_parameters()}
    assert float(grads["base_rt.se3"].abs().max()) > 0
    assert any(float(g.abs().max()) > 0 for n, g in grads.items() if n.startswith("mlp_rt.") and g is not None)
    with torch.no_grad():
        rtk = moda_amd.compute_rts(Model.nerf_root_rts, T)
    val, b = O.rtk_loss(host(rtk), host(state.rtk))
    sm = float(moda_amd.compute_root_sm_2nd_loss(rtk, [0, 15, T]))
    within(float(aux["rot_loss"]), val["rot_loss"], b["rot_loss"])
    assert abs(float(total) - (0.1 * val["rot_loss"] + 0.01 * sm)) <= 0.1 * b["rot_loss"] + 4 * O.U32 * abs(float(total))
    Model.use_cam = True                                                      # the reference starts from a ZERO table then (moda.py:780)
    total_c, aux_c = warmup.forward_warmup_rootmlp(Model, dict(root_opt=True))
    with torch.no_grad():
        rtk_c = moda_amd.compute_rts(Model.nerf_root_rts, T, rt_raw=torch.zeros(T, 3, 4, device="cuda"))
    assert float(rtk_c.abs().max()) == 0.0                                    # zero rotations: every pose is zero
    val_c, b_c = O.rtk_loss(host(rtk_c), host(state.rtk))
    within(float(aux_c["rot_loss"]), val_c["rot_loss"], b_c["rot_loss"])
    assert set(aux_c) == {"rot_loss", "warmup_root_sm_loss"} and np.isfinite(float(total_c))
    Model.use_cam = False
    Model.latest_vars = {"rtk": host(state.rtk)}                              # the reference's dict of arrays: uploaded
    total2, _ = warmup.forward_warmup_rootmlp(Model, dict(root_opt=True))
    assert float(total2) == float(total)
