"""GPU (-m gpu): the pose CNN kernels (csrc/posecnn_kernels.hip) and the stage built on them -- moda_amd.Encoder, the `cnn` basis
of convert_root_pose, warmup.extract_cams -- against float64 (tests/posecnn_torch.py, tests/golden/g38_posecnn.npz).

Bounds.  A convolution output is one fp32 fma chain of K = kh kw Cin steps plus the bias, residual and activation roundings;
against float64 on the SAME fp32 operands its error is at most (K + 4) 2^-24 (sum |w x| + |b|) per element (the standard bound of
a length-K recursive sum, with slack for the epilogue's operations).  The whole network is held to the project's fp32 parity bar
of 1e-4 of the reference's largest value; torch's own fp32 error on the CPU is reported beside ours.  Measured on an MI355X for
the golden weights, as a share of max |ref|, inputs a / b: features 1.9e-6 / 1.2e-6 (torch fp32 on the CPU 2.7e-7 / 2.2e-7),
head output 1.4e-6 / 1.2e-6 (6.0e-7 / 5.5e-7), rtk 2.7e-9 / 2.3e-9 (1.2e-9 / 1.1e-9; its largest value is a focal length).  The
kernel's sums are single chains of up to 4608 steps where torch's are blocked, hence the larger figure; it is 50 times inside
the bar."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import moda_amd
import posecnn_torch as PT
import warmup_numpy as O
from moda_amd import pose_cnn as PC
from moda_amd import warmup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device="cuda", dtype=dtype).contiguous()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def g38():
    return np.load(os.path.join(ROOT, "tests", "golden", "g38_posecnn.npz"))


@pytest.fixture(scope="module")
def state():
    return PT.state_tensors(PT.make_state(PT.SEED))


@pytest.fixture(scope="module")
def posenet(state):
    return moda_amd.build_pose_cnn({"module.nerf_root_rts." + k: v for k, v in state.items()}, device="cuda")


@pytest.fixture(scope="module")
def frames5(g38):
    """The five golden frames at ONE size, so that they can share a batch: the three 112 x 112 frames, and the two 100 x 123 frames
    cut to 112 columns and padded with zero rows to 112."""
    b = np.zeros((2, 16, 112, 112), np.float32)
    b[:, :, 6:106] = g38["x_b"][:, :, :, 5:117]
    return dev(np.concatenate([g38["x_a"], b]))


# ---- 1. the convolution, per layer form, against float64 ------------------------------------------------------------------------------
CONV_CASES = [   # kh, stride, pad, Cin, Cout, H, W
    (7, 2, 3, 16, 64, 13, 11),
    (3, 1, 1, 64, 64, 5, 7),
    (3, 2, 1, 64, 128, 7, 7),
    (1, 2, 0, 128, 256, 7, 7),
    (3, 1, 1, 512, 512, 4, 4),
    (3, 1, 1, 512, 128, 4, 4),
]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "k{}s{}p{}_{}to{}_{}x{}".format(*c))
def test_conv_against_float64(case, B):
    k, stride, pad, Cin, Cout, H, W = case
    rs = np.random.RandomState(Cin + Cout + B)
    x = rs.standard_normal((B, H, W, Cin)).astype(np.float32)
    w = (rs.standard_normal((Cout, k, k, Cin)) / np.sqrt(k * k * Cin)).astype(np.float32)
    bias = rs.standard_normal((Cout,)).astype(np.float32)
    Ho, Wo = PC.conv_out(H, k, stride, pad), PC.conv_out(W, k, stride, pad)
    res = rs.standard_normal((B, Ho, Wo, Cout)).astype(np.float32)
    K = k * k * Cin
    xd, wd, bd, rd = dev(x), dev(w), dev(bias), dev(res)
    for use_res in (False, True):
        for act in (PC.ACT_NONE, PC.ACT_RELU, PC.ACT_LEAKY):
            ref, mag = PT.conv_nhwc_ref(x, w, bias, stride, pad, res if use_res else None, act)
            got = PC.conv2d_nhwc(xd, wd, bd, stride=stride, pad=pad, res=rd if use_res else None, act=act)
            assert got.shape == (B, Ho, Wo, Cout)
            err = np.abs(host(got).astype(np.float64) - ref)
            bound = (K + 4) * U32 * mag
            print(f"conv {case} B={B} res={use_res} act={act}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3e}")
            assert (err <= bound).all(), (case, B, use_res, act, float(err.max()), float((err / bound).max()))
            for tile in (PC.TILE_32, PC.TILE_64):              # both tile forms give the automatic one's bits
                forced = PC.conv2d_nhwc(xd, wd, bd, stride=stride, pad=pad, res=rd if use_res else None, act=act, tile=tile)
                assert torch.equal(forced, got), (case, B, use_res, act, tile)


# ---- 2. the max pool ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 8, 8, 64), (3, 7, 9, 8)])
def test_maxpool_equals_torch_on_negative_inputs(shape):
    rs = np.random.RandomState(7)
    x = (-np.abs(rs.standard_normal(shape)) - 0.5).astype(np.float32)          # all negative: a zero padding would win every border
    x[0, 2, 3, :4] = 1.5
    ref = F.max_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    got = PC.maxpool3x3s2_nhwc(dev(x))
    assert got.shape == ref.shape and torch.equal(got.cpu(), ref)
    assert float(got.max()) == 1.5 and float(got[1].max()) < 0


# ---- 3. the whole PoseNet against the reference's float64 run -------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b"])
def test_posenet_against_the_reference(g38, state, posenet, tag):
    img, ks, dataid = g38["x_" + tag], g38["ks"], g38["dataid_" + tag]
    B = img.shape[0]
    with torch.no_grad():
        feat = posenet[0](dev(img))
        rts = posenet[1](feat)
        rtk = moda_amd.convert_root_pose(posenet, torch.arange(B, device="cuda"), dev(dataid, torch.int64), dev(ks), dp_feats=dev(img))
    cpu32 = dict(zip(("feat", "rts", "rtk"), PT.posenet(state, img, ks, dataid, torch.float32)))
    report = []
    for name, got in (("feat", feat), ("rts", rts), ("rtk", rtk)):
        ref = g38[f"{name}_{tag}_64"]
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        scale = np.abs(ref).max()
        e_hip = np.abs(host(got).astype(np.float64) - ref).max() / scale
        e_cpu = np.abs(cpu32[name].numpy().astype(np.float64) - ref).max() / scale
        report.append((name, e_hip, e_cpu))
    text = "; ".join(f"{n}: HIP {a:.3e}, torch fp32 on the CPU {b:.3e} (of max |ref|)" for n, a, b in report)
    print(f"posenet {tag}: {text}")
    assert all(a <= 1e-4 for _, a, _ in report), text
    assert torch.isfinite(rtk).all() and torch.equal(rtk[:, 3], dev(ks)[dev(dataid, torch.int64)])


# ---- 4. a frame has the same bits alone and in any batch ------------------------------------------------------------------------------
def test_batch_independence(posenet, frames5, g38):
    enc = posenet[0]
    with torch.no_grad():
        whole = enc(frames5)
        singly = torch.cat([enc(frames5[i:i + 1]) for i in range(5)])
        split = torch.cat([enc(frames5[:2]), enc(frames5[2:])])
        xb = dev(g38["x_b"])
        pair, alone = enc(xb), torch.cat([enc(xb[i:i + 1]) for i in range(2)])
    assert whole.shape == (5, 128) and torch.isfinite(whole).all() and float(whole.std()) > 0
    assert torch.equal(whole, singly) and torch.equal(whole, split) and torch.equal(pair, alone)


def _extract(posenet, frames5, chunk, order, **kw):
    state = moda_amd.FrameState(7)
    fid = torch.as_tensor(order, device="cuda")
    dataid = torch.as_tensor([0, 1, 0, 1, 0], device="cuda")
    kaug = dev(np.asarray([[1.0, 1.5, 10.0, 20.0]] * 5) + np.arange(5)[:, None] * 0.1)
    out = warmup.extract_cams(posenet, frames5, fid, dataid, dev(PT.KS), kaug, state, chunk=chunk, **kw)
    return out, state


def test_extract_cams_does_not_depend_on_the_chunk(posenet, frames5):
    order = [4, 0, 6, 1, 3]
    (rtk2, ok2, err2), s2 = _extract(posenet, frames5, 2, order)
    (rtk50, ok50, err50), s50 = _extract(posenet, frames5, 50, order)
    assert rtk2.shape == (5, 4, 4) and torch.isfinite(rtk2).all()
    assert torch.equal(rtk2, rtk50) and torch.equal(ok2, ok50) and torch.equal(err2, err50) and bool(ok2.all())
    for name in ("rtk", "rt_raw", "idk", "status"):
        assert torch.equal(getattr(s2, name), getattr(s50, name)), name
    assert host(s2.idk).tolist() == [1, 1, 0, 1, 1, 0, 1] and host(s2.status).tolist() == [0, 0, 0, 0]
    assert torch.equal(s2.rt_raw[order], rtk2[:, :3]) and torch.equal(s2.rtk[order][:, :3], rtk2[:, :3])
    # the features reach the CNN normalised: a power-of-two scale is exact in every step of the normalisation, so it changes no
    # bit; and normalize=False is the plain route
    (rtk_s, _, _), _ = _extract(posenet, frames5 * 4.0, 50, order)
    assert torch.equal(rtk_s, rtk2)
    (rtk_n, _, _), _ = _extract(posenet, PC.normalize_feats(frames5), 3, order, normalize=False)
    assert torch.equal(rtk_n, rtk2)
    with torch.no_grad():
        direct = moda_amd.convert_root_pose(posenet, torch.as_tensor(order, device="cuda"), torch.as_tensor([0, 1, 0, 1, 0], device="cuda"),
                                            dev(PT.KS), dp_feats=PC.normalize_feats(frames5))
    assert torch.equal(direct, rtk2)


def test_extract_cams_with_the_uncertainty_filter(posenet, frames5):
    rs = np.random.RandomState(11)
    emb = rs.standard_normal((40, 16)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    dps = dev(rs.randint(0, 40, (5, 112, 112)) * (host(frames5).any(1)), torch.int64)
    (rtk_a, ok_a, err_a), _ = _extract(posenet, frames5, 2, [0, 1, 2, 3, 4], dp_embed=dev(emb), dps=dps, unc_filter=True)
    (rtk_b, ok_b, err_b), _ = _extract(posenet, frames5, 50, [0, 1, 2, 3, 4], dp_embed=dev(emb), dps=dps, unc_filter=True)
    assert torch.equal(rtk_a, rtk_b) and torch.equal(ok_a, ok_b) and torch.equal(err_a, err_b)
    ok_ref, err_ref = moda_amd.ood_check_cse(PC.normalize_feats(frames5), dev(emb), dps)
    assert torch.equal(ok_a, ok_ref) and torch.equal(err_a, err_ref) and float(err_a.min()) > 0
    with pytest.raises(ValueError, match="unc_filter"):
        _extract(posenet, frames5, 2, [0, 1, 2, 3, 4], unc_filter=True)


# ---- 5. determinism and capture ---------------------------------------------------------------------------------------------------------
def test_eager_runs_and_a_graph_replay_agree_bit_for_bit(posenet, frames5):
    fid = torch.arange(3, device="cuda")
    dataid = torch.zeros(3, dtype=torch.int64, device="cuda")
    ks = dev(PT.KS)
    buf = frames5[:3].clone()

    def run():
        feat = posenet[0](buf)
        return feat, moda_amd.convert_root_pose(posenet, fid, dataid, ks, dp_feats=buf)

    with torch.no_grad():
        f1, r1 = run()
        f2, r2 = run()
        assert torch.equal(f1, f2) and torch.equal(r1, r2)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fg, rg = run()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(fg, f1) and torch.equal(rg, r1)
        buf.copy_(frames5[2:5])                                                # the replay follows the buffer
        graph.replay()
        torch.cuda.synchronize()
        f3, r3 = posenet[0](frames5[2:5].contiguous()), moda_amd.convert_root_pose(posenet, fid, dataid, ks, dp_feats=frames5[2:5].contiguous())
        assert torch.equal(fg, f3) and torch.equal(rg, r3) and not torch.equal(f3, f1)
        assert torch.equal(f3[0], f1[2])


def test_packed_weights_follow_a_changed_parameter(state):
    enc = moda_amd.Encoder((112, 112), in_channels=16)
    enc.load_state_dict({k[2:]: v for k, v in state.items() if k.startswith("0.")})
    enc = enc.cuda().eval()
    x = dev(PT.golden_inputs()[0][:1])
    with torch.no_grad():
        a = enc(x)
        assert enc.packed() is enc.packed()
        saved = enc.conv1[1].running_mean.clone()
        enc.conv1[1].running_mean.add_(0.25)
        b = enc(x)
        enc.conv1[1].running_mean.copy_(saved)                                 # (subtracting 0.25 again would not restore the bits)
        c = enc(x)
    assert not torch.equal(a, b) and torch.equal(a, c)


# ---- 6. the input kernel ------------------------------------------------------------------------------------------------------------------
def test_input_kernel_normalises_like_float64(g38):
    rs = np.random.RandomState(3)
    x = g38["x_b"] * rs.uniform(0.01, 30.0, (2, 1, 100, 123)).astype(np.float32)    # zero outside the blob, any length inside
    x[0, :, 50, 60] = 1e-20                                                           # a norm below eps: divided by eps
    ref = F.normalize(torch.from_numpy(x).double(), 2, 1).permute(0, 2, 3, 1).numpy()
    got = host(PC.to_nhwc(dev(x), normalize=True)).astype(np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert (np.abs(got - ref) <= 2 * ulp).all(), float((np.abs(got - ref) / ulp).max())
    zero = ~x.any(1)
    assert zero.mean() > 0.5 and (got[zero] == 0).all()
    plain = PC.to_nhwc(dev(x), cpad=32)
    assert torch.equal(plain[..., :16], dev(x).permute(0, 2, 3, 1)) and float(plain[..., 16:].abs().max()) == 0
    assert torch.equal(PC.normalize_feats(dev(x)), PC.to_nhwc(dev(x), normalize=True).permute(0, 3, 1, 2))


# ---- 7. refusals on the device ------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(posenet, frames5):
    fid = torch.arange(5, device="cuda")
    with pytest.raises(NotImplementedError, match="Encoder"):
        moda_amd.convert_root_pose(posenet, fid, torch.zeros_like(fid), dev(PT.KS))
    with pytest.raises(NotImplementedError, match="Encoder"):
        moda_amd.compute_rts(posenet, 5)
    with pytest.raises(ValueError):
        posenet[0](frames5[:, :, :64, :64].contiguous())
    with pytest.raises(NotImplementedError, match="grad"):
        posenet[0](frames5.clone().requires_grad_(True))
    posenet.train()
    try:
        with pytest.raises(NotImplementedError, match="training"):
            posenet[0](frames5)
    finally:
        posenet.eval()
    with pytest.raises(ValueError, match="dp_feats"):
        head = moda_amd.RTHead(use_quat=True, D=1, W=16, in_channels_xyz=8, in_channels_dir=0, out_channels=7, raw_feat=True).cuda()
        moda_amd.convert_root_pose(torch.nn.Sequential(torch.nn.Embedding(5, 8).cuda(), head), fid, torch.zeros_like(fid), dev(PT.KS),
                                   dp_feats=frames5)


# ---- 8. cameras from the CNN into the root preset -----------------------------------------------------------------------------------------
def test_extract_cams_then_preset_root_rotations(posenet, frames5):
    T = 5
    (rtk, _, _), state = _extract_all(posenet, frames5, T)
    root = moda_amd.RTExpMLP(T, 6, 128, [0, T]).cuda()
    with torch.no_grad():
        root.mlp_rt.rgb[0].weight.zero_()                                     # a zero-initialised tail: the delta is the identity
        root.mlp_rt.rgb[0].bias.zero_()
    warmup.preset_root_rotations(root, state)
    with torch.no_grad():
        got = host(moda_amd.compute_rts(root, T))
    want = host(rtk)[:, :3, :3]
    assert np.abs(np.linalg.det(want.astype(np.float64)) - 1).max() < 1e-5
    assert np.abs(got[:, :3, :3] - want).max() <= O.ROUNDTRIP_F32 + 16 * O.U32


def _extract_all(posenet, frames5, T):
    state = moda_amd.FrameState(T)
    fid = torch.arange(T, device="cuda")
    kaug = dev(np.asarray([[1.0, 1.0, 0.0, 0.0]] * T))
    return warmup.extract_cams(posenet, frames5, fid, torch.zeros_like(fid), dev(PT.KS), kaug, state), state
