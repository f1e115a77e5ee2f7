"""The PoseNet of the reference -- nn.Sequential(Encoder, RTHead(use_quat=True, D=1)) (nnutils/nerf.py:513-573, 307-344,
nnutils/moda.py:361-366) -- restated with torch.nn.functional in a chosen dtype (float64: the oracle; float32: torch's own fp32
error on the same weights), without torchvision: ResNet-18's published topology (7x7 s2 conv, BatchNorm, ReLU, 3x3 s2 max pool,
four stages of two BasicBlocks, 64 / 128 / 256 / 512 channels, a 1x1 s2 downsample in the first block of stages 2-4), then the
3x3 conv block 512 -> 128 with BatchNorm and LeakyReLU(0.2), max_pool2d(4, 4), the head, refine_rt on create_base_se3 and the K row.

make_state(seed) draws a full state dict from numpy.random.RandomState(seed): conv weights scaled by 1 / sqrt(fan_in),
running_var in [0.5, 2], running_mean, BatchNorm bias and weight non-trivial -- a wrong fold, a swapped mean / var, or a dropped
conv bias cannot pass.  The trunk is 11 M parameters: the tests regenerate it from the seed, nothing of it is stored.

tests/golden/g38_posecnn.npz holds what the reference's own modules gave for make_state(SEED) on the two inputs of
golden_inputs() (tests/golden/gen_golden_posecnn.py)."""
import numpy as np
import torch
import torch.nn.functional as F

SEED = 38
KS = np.asarray([[300.0, 500.0, 200.0, 250.0], [320.0, 480.0, 210.0, 240.0]], np.float32)
STAGES = ((1, 64, 64, 1), (2, 64, 128, 2), (3, 128, 256, 2), (4, 256, 512, 2))
BN_EPS = 1e-5
HEAD_W = 256


def _bn_keys(prefix):
    return [prefix + s for s in (".weight", ".bias", ".running_mean", ".running_var", ".num_batches_tracked")]


def layer_shapes(in_channels=16):
    """[(key, shape)] of the Encoder's convolutions and BatchNorms in torchvision's order, then the tail block's."""
    out = [("resnet_conv.resnet.conv1.weight", (64, in_channels, 7, 7)), ("resnet_conv.resnet.bn1", 64)]
    for li, cin, cout, stride in STAGES:
        for bi in range(2):
            p = f"resnet_conv.resnet.layer{li}.{bi}"
            c0 = cin if bi == 0 else cout
            out += [(p + ".conv1.weight", (cout, c0, 3, 3)), (p + ".bn1", cout), (p + ".conv2.weight", (cout, cout, 3, 3)), (p + ".bn2", cout)]
            if bi == 0 and (stride != 1 or cin != cout):
                out += [(p + ".downsample.0.weight", (cout, cin, 1, 1)), (p + ".downsample.1", cout)]
    out += [("conv1.0.weight", (128, 512, 3, 3)), ("conv1.0.bias", (128,)), ("conv1.1", 128)]
    return out


def head_shapes():
    W = HEAD_W
    return [("xyz_encoding_1.0.weight", (W, 128)), ("xyz_encoding_1.0.bias", (W,)), ("xyz_encoding_final.weight", (W, W)),
            ("xyz_encoding_final.bias", (W,)), ("dir_encoding.0.weight", (W // 2, W)), ("dir_encoding.0.bias", (W // 2,)),
            ("sigma.weight", (1, W)), ("sigma.bias", (1,)), ("rgb.0.weight", (7, W // 2)), ("rgb.0.bias", (7,)), ("beta", (1,))]


def make_state(seed=SEED, in_channels=16):
    """-> {key: numpy array} of nn.Sequential(Encoder, RTHead): keys '0.*' and '1.*', float32 (num_batches_tracked int64)."""
    rs = np.random.RandomState(seed)
    sd = {}
    for key, shape in layer_shapes(in_channels):
        if isinstance(shape, tuple):
            fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
            scale = 1.0 / np.sqrt(fan_in) if len(shape) > 1 else 0.1
            sd["0." + key] = (rs.standard_normal(shape) * scale).astype(np.float32)
        else:
            sd["0." + key + ".weight"] = rs.uniform(0.5, 1.5, shape).astype(np.float32)
            sd["0." + key + ".bias"] = (rs.standard_normal(shape) * 0.2).astype(np.float32)
            sd["0." + key + ".running_mean"] = (rs.standard_normal(shape) * 0.3).astype(np.float32)
            sd["0." + key + ".running_var"] = rs.uniform(0.5, 2.0, shape).astype(np.float32)
            sd["0." + key + ".num_batches_tracked"] = np.asarray(rs.randint(1, 1000), np.int64)
    for key, shape in head_shapes():
        if key == "beta":
            sd["1." + key] = np.asarray([0.01], np.float32)
        elif len(shape) == 2:
            sd["1." + key] = (rs.standard_normal(shape) / np.sqrt(shape[1])).astype(np.float32)
        else:
            sd["1." + key] = (rs.standard_normal(shape) * 0.1).astype(np.float32)
    return sd


def state_tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def blob_input(rs, B, H, W, C=16):
    """(B,C,H,W) float32 like a DensePose-CSE feature image: zero outside an elliptic blob, unit norm over C inside."""
    x = rs.standard_normal((B, C, H, W))
    x /= np.sqrt((x * x).sum(1, keepdims=True))
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros_like(x)
    for b in range(B):
        cy, cx = H * (0.4 + 0.1 * b), W * (0.55 - 0.05 * b)
        m = ((yy - cy) / (0.22 * H)) ** 2 + ((xx - cx) / (0.18 * W)) ** 2 <= 1.0
        out[b] = x[b] * m[None]
    return out.astype(np.float32)


def golden_inputs(seed=SEED):
    rs = np.random.RandomState(seed + 1000)
    return blob_input(rs, 3, 112, 112), blob_input(rs, 2, 100, 123)


# ---- the forward pass in `dtype` -----------------------------------------------------------------------------------------------------
def _bn(x, sd, p, dt):
    return F.batch_norm(x, sd[p + ".running_mean"].to(dt), sd[p + ".running_var"].to(dt), sd[p + ".weight"].to(dt), sd[p + ".bias"].to(dt),
                        False, 0.0, BN_EPS)


def encoder(sd, img, dtype=torch.float64, prefix="0."):
    """sd: {key: tensor}; img (B,C,H,W) -> (B,128) in `dtype`."""
    dt = dtype
    r = prefix + "resnet_conv.resnet."
    x = torch.as_tensor(img).to(dt)
    x = F.conv2d(x, sd[r + "conv1.weight"].to(dt), None, 2, 3)
    x = F.relu(_bn(x, sd, r + "bn1", dt))
    x = F.max_pool2d(x, 3, 2, 1)
    for li, cin, cout, stride in STAGES:
        for bi in range(2):
            p = f"{r}layer{li}.{bi}"
            s = stride if bi == 0 else 1
            y = F.relu(_bn(F.conv2d(x, sd[p + ".conv1.weight"].to(dt), None, s, 1), sd, p + ".bn1", dt))
            y = _bn(F.conv2d(y, sd[p + ".conv2.weight"].to(dt), None, 1, 1), sd, p + ".bn2", dt)
            if p + ".downsample.0.weight" in sd:
                x = _bn(F.conv2d(x, sd[p + ".downsample.0.weight"].to(dt), None, s, 0), sd, p + ".downsample.1", dt)
            x = F.relu(y + x)
    t = prefix + "conv1."
    x = F.conv2d(x, sd[t + "0.weight"].to(dt), sd[t + "0.bias"].to(dt), 1, 1)
    x = F.leaky_relu(_bn(x, sd, t + "1", dt), 0.2)
    x = F.max_pool2d(x, 4, 4)
    return x.view(x.shape[0], -1)


def quaternion_to_matrix(q):
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r), two_s * (i * j + k * r),
                     1 - two_s * (i * i + k * k), two_s * (j * k - i * r), two_s * (i * k - j * r), two_s * (j * k + i * r),
                     1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def head(sd, feat, dtype=torch.float64, prefix="1."):
    """RTHead(use_quat=True, D=1): feat (B,128) -> (B,1,12) = [R | t]."""
    dt = dtype
    lin = lambda x, k: F.linear(x, sd[prefix + k + ".weight"].to(dt), sd[prefix + k + ".bias"].to(dt))
    h = F.relu(lin(feat.to(dt), "xyz_encoding_1.0"))
    d = F.relu(lin(lin(h, "xyz_encoding_final"), "dir_encoding.0"))
    rts = lin(d, "rgb.0").view(-1, 7)
    rmat = quaternion_to_matrix(F.normalize(rts[:, 3:7], 2, -1)).view(-1, 9)
    return torch.cat([rmat, rts[:, :3] * 0.1], -1).view(feat.shape[0], 1, -1)


def rtk_of(rts, ks, dataid, dtype=torch.float64):
    """refine_rt(create_base_se3, rts) with the K row (moda.py:1433-1447): (B,1,12) -> (B,4,4)."""
    bs = rts.shape[0]
    rtk = torch.zeros(bs, 4, 4, dtype=dtype)
    base_t = torch.tensor([0.0, 0.0, float(np.float32(0.3))], dtype=dtype)          # create_base_se3 is fp32: R = I, t = (0, 0, 0.3f)
    rtk[:, :3, :3] = rts[:, 0, :9].view(-1, 3, 3)
    rtk[:, :3, 3] = base_t[None] + rts[:, 0, 9:12]
    rtk[:, 3] = torch.as_tensor(ks).to(dtype)[torch.as_tensor(dataid).long()]
    return rtk


def posenet(sd, img, ks, dataid, dtype=torch.float64):
    """-> (feat (B,128), rts (B,1,12), rtk (B,4,4)) in `dtype`."""
    feat = encoder(sd, img, dtype)
    rts = head(sd, feat, dtype)
    return feat, rts, rtk_of(rts, ks, dataid, dtype)


# ---- per-layer references of the GPU tests -------------------------------------------------------------------------------------------
def conv_nhwc_ref(x, w, bias, stride, pad, res=None, act=0):
    """x (B,H,W,Cin), w (Cout,kh,kw,Cin) packed, both float32 arrays -> (out float64 (B,Ho,Wo,Cout), mag = sum |w x| + |bias| per
    element, float64): what moda_conv2d_nhwc computes, in float64 on the same fp32 operands."""
    xt = torch.from_numpy(np.asarray(x)).double().permute(0, 3, 1, 2)
    wt = torch.from_numpy(np.asarray(w)).double().permute(0, 3, 1, 2)
    bt = torch.from_numpy(np.asarray(bias)).double()
    y = F.conv2d(xt, wt, bt, stride, pad)
    mag = F.conv2d(xt.abs(), wt.abs(), bt.abs(), stride, pad)
    if res is not None:
        r = torch.from_numpy(np.asarray(res)).double().permute(0, 3, 1, 2)
        y = y + r
    if act == 1:
        y = F.relu(y)
    elif act == 2:
        y = F.leaky_relu(y, 0.2)
    return y.permute(0, 2, 3, 1).contiguous().numpy(), mag.permute(0, 2, 3, 1).contiguous().numpy()
