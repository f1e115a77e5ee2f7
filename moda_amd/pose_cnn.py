"""The pose CNN of the reference's camera initialisation, in inference mode on the device: `ResNetConv` (nnutils/nerf.py:513-534,
the ResNet-18 trunk without its classifier) and `Encoder` (nerf.py:536-556: trunk, one 3x3 conv block 512 -> 128 with BatchNorm
and LeakyReLU(0.2), max_pool2d(4, 4)) -> (B, 128).  With an RTHead behind it this is `dp_root_rts`, the PoseNet that
warmup_pose(pose_cnn_path=...) loads and extract_cams runs over every frame's DensePose-CSE feature image
(nnutils/train_utils.py:871-906, 794-807).

The modules hold the reference's / torchvision's parameter and buffer names, so a PoseNet state dict loads with strict=True
(checkpoint.build_pose_cnn); torchvision is not needed and no pretrained weights are ever looked for -- the initial values are a
plain seeded draw.  forward() is 24 launches of csrc/posecnn_kernels.hip: the input reshuffle NCHW -> NHWC, 20 implicit-GEMM
convolutions on the fp32 MFMA with eval-mode BatchNorm folded into weights and bias and the residual add and activation in the
epilogue, the 3x3 max pool, and the final maximum over the 4 x 4 map.  Nothing is read back, so a call can be captured; a frame
has the same bits alone and inside any batch.

The folded, packed weights ([Cout][kh][kw][Cin] fp32) are built on the first call and again whenever a parameter or buffer has
been written since (its version counter or storage changed): that call must happen outside a graph capture.

Not implemented, refused by name: training (module.training, inputs that require grad, BatchNorm batch statistics, any gradient
through the convolutions -- the recipe never trains the CNN), batch_norm=False, and input sizes whose layer-4 map is not 4 x 4
(the reference's view(B, -1) gives 128 columns for those alone)."""
import math

import torch
from torch import nn

from . import _lib as L
from . import abi

K_CHUNK = abi.CONSTANTS["MODA_CONV_K_CHUNK"]
ACT_NONE, ACT_RELU, ACT_LEAKY = (abi.CONSTANTS["MODA_CONV_ACT_" + k] for k in ("NONE", "RELU", "LEAKY"))
TILE_AUTO, TILE_32, TILE_64 = (abi.CONSTANTS["MODA_CONV_TILE_" + k] for k in ("AUTO", "32", "64"))
INIT_SEED = 0


def conv_out(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def fold_bn(weight, conv_bias, bn_weight, bn_bias, running_mean, running_var, eps, *, cin_pad=None, dtype=torch.float64):
    """A convolution followed by eval-mode BatchNorm as one convolution: weight (Cout,Cin,kh,kw) ->
    (w' (Cout,kh,kw,Cp) = w * gamma / sqrt(var + eps) with channels Cin .. Cp-1 zero, b' (Cout) = beta + (conv_bias - mean) *
    gamma / sqrt(var + eps)), formed in float64 and returned as `dtype`."""
    w = weight.detach().double()
    scale = bn_weight.detach().double() / torch.sqrt(running_var.detach().double() + eps)
    shift = bn_bias.detach().double() - running_mean.detach().double() * scale
    if conv_bias is not None:
        shift = shift + conv_bias.detach().double() * scale
    w = (w * scale[:, None, None, None]).permute(0, 2, 3, 1)
    cin = w.shape[-1]
    if cin_pad is not None and cin_pad > cin:
        w = torch.cat([w, w.new_zeros(w.shape[:-1] + (cin_pad - cin,))], -1)
    return w.contiguous().to(dtype), shift.contiguous().to(dtype)


def conv2d_nhwc(x, w, bias, *, stride=1, pad=0, res=None, act=ACT_NONE, tile=TILE_AUTO):
    """moda_conv2d_nhwc: x (B,H,W,Cin), w (Cout,kh,kw,Cin) packed, bias (Cout), res (B,Ho,Wo,Cout) | None -> (B,Ho,Wo,Cout) =
    act(conv(x, w) + bias + res); Cin a multiple of 16.  Contiguous fp32 device tensors."""
    for t in (x, w, bias, res):
        if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError("conv2d_nhwc: contiguous fp32 tensors only")
    if x.dim() != 4 or w.dim() != 4 or w.shape[3] != x.shape[3] or bias.shape != (w.shape[0],):
        raise ValueError(f"conv2d_nhwc: x {tuple(x.shape)}, w {tuple(w.shape)}, bias {tuple(bias.shape)}")
    for t in (x, w, bias, res):
        if t is not None and not t.is_cuda:
            raise RuntimeError("conv2d_nhwc takes CUDA (ROCm) tensors; the HIP library is the only compute path")
    B, H, W, Cin = x.shape
    Cout, kh, kw, _ = w.shape
    Ho, Wo = conv_out(H, kh, stride, pad), conv_out(W, kw, stride, pad)
    if res is not None and tuple(res.shape) != (B, Ho, Wo, Cout):
        raise ValueError(f"conv2d_nhwc: res {tuple(res.shape)} for an output of {(B, Ho, Wo, Cout)}")
    out = torch.empty((B, max(Ho, 0), max(Wo, 0), Cout), device=x.device, dtype=torch.float32)
    L.call("moda_conv2d_nhwc", L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(res), L.ptr(out), B, H, W, Cin, Cout, kh, kw, int(stride),
           int(pad), int(act), int(tile), L.stream())
    return out


def maxpool3x3s2_nhwc(x):
    """F.max_pool2d(., 3, 2, 1) over x (B,H,W,C), C a multiple of 4: -inf padding, a NaN wins."""
    x = L.dev(x)
    B, H, W, C = x.shape
    out = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), device=x.device, dtype=torch.float32)
    L.call("moda_maxpool3x3s2_nhwc", L.ptr(x), B, H, W, C, L.ptr(out), L.stream())
    return out


def to_nhwc(img, *, cpad=None, normalize=False):
    """moda_posecnn_input: img (B,C,H,W) -> (B,H,W,Cp) with channels C .. Cp-1 zero; normalize: F.normalize(img, 2, 1) on the way."""
    img = L.dev(img)
    B, C, H, W = img.shape
    Cp = C if cpad is None else int(cpad)
    out = torch.empty((B, H, W, Cp), device=img.device, dtype=torch.float32)
    L.call("moda_posecnn_input", L.ptr(img), B, C, H, W, Cp, 1 if normalize else 0, L.ptr(out), L.stream())
    return out


def normalize_feats(dp_feats):
    """F.normalize(dp_feats, 2, 1) (moda.py:1399) for (B,C,H,W) features: the input kernel's normalisation, moved back to NCHW."""
    return to_nhwc(dp_feats, normalize=True).permute(0, 3, 1, 2).contiguous()


def max_over_positions(x):
    """moda_posecnn_tail: x (B,h,w,C) -> (B,C), the maximum over the map."""
    x = L.dev(x)
    B, C = x.shape[0], x.shape[-1]
    out = torch.empty((B, C), device=x.device, dtype=torch.float32)
    L.call("moda_posecnn_tail", L.ptr(x), B, x.numel() // (B * C), C, L.ptr(out), L.stream())
    return out


def _conv(cin, cout, k, stride, bias=False):
    return nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=(k - 1) // 2, bias=bias)


class BasicBlock(nn.Module):
    """torchvision's BasicBlock, as a parameter tree: conv1, bn1, conv2, bn2, downsample = Sequential(conv 1x1, bn) | None."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = _conv(cin, cout, 3, stride)
        self.bn1 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = _conv(cout, cout, 3, 1)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(_conv(cin, cout, 1, stride), nn.BatchNorm2d(cout))
        self.stride = stride


class ResNet18Trunk(nn.Module):
    """The attributes of torchvision.models.resnet18 that ResNetConv uses (fc is None, as the reference sets it)."""

    def __init__(self, in_channels):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = nn.Sequential(BasicBlock(64, 64, 1), BasicBlock(64, 64, 1))
        self.layer2 = nn.Sequential(BasicBlock(64, 128, 2), BasicBlock(128, 128, 1))
        self.layer3 = nn.Sequential(BasicBlock(128, 256, 2), BasicBlock(256, 256, 1))
        self.layer4 = nn.Sequential(BasicBlock(256, 512, 2), BasicBlock(512, 512, 1))
        self.fc = None


class ResNetConv(nn.Module):
    """nerf.py:513-534: the ResNet-18 trunk over `in_channels` input channels -> (B,512,h/32,w/32).  Run through Encoder."""

    def __init__(self, in_channels):
        super().__init__()
        self.resnet = ResNet18Trunk(in_channels)

    def forward(self, x):
        raise NotImplementedError("ResNetConv: the trunk runs inside moda_amd.Encoder.forward (NHWC, folded BatchNorm); it is not "
                                  "implemented as a stand-alone forward")


def _seeded_init(module, seed):
    """Convolutions ~ N(0, 2 / fan_out) from a generator of their own (no global RNG state is consumed for the values),
    BatchNorm weight 1, bias 0, running statistics 0 / 1."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.Conv2d):
                fan_out = m.out_channels * m.kernel_size[0] * m.kernel_size[1]
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * math.sqrt(2.0 / fan_out))
                if m.bias is not None:
                    m.bias.zero_()
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.fill_(1.0)
                m.bias.zero_()
                m.running_mean.zero_()
                m.running_var.fill_(1.0)


class Encoder(nn.Module):
    """nerf.py:536-556: img (B,Cin,H,W) -> (B,128).  input_shape is kept for the reference's signature (it does not use it either)."""

    def __init__(self, input_shape, in_channels=3, out_channels=128, batch_norm=True):
        super().__init__()
        if not batch_norm:
            raise NotImplementedError("Encoder: batch_norm=False (the tail conv block without BatchNorm) is not implemented; the "
                                      "reference never builds it")
        self.input_shape = tuple(input_shape)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.resnet_conv = ResNetConv(in_channels=in_channels)
        self.conv1 = nn.Sequential(_conv(512, out_channels, 3, 1, bias=True), nn.BatchNorm2d(out_channels), nn.LeakyReLU(0.2, inplace=True))
        _seeded_init(self, INIT_SEED)
        self._packed = {}

    # ---- folded, packed weights ------------------------------------------------------------------------------------------
    def _stamp(self):
        return tuple((t._version, t.data_ptr()) for t in list(self.parameters()) + list(self.buffers()))

    def packed(self, device=None):
        """{layer name: (w' (Cout,kh,kw,Cp) fp32, b' (Cout) fp32)} on the parameters' device, rebuilt when anything was written."""
        device = next(self.parameters()).device if device is None else torch.device(device)
        stamp = self._stamp()
        hit = self._packed.get(str(device))
        if hit is not None and hit[0] == stamp:
            return hit[1]
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("Encoder: the folded weights are packed on the first call and after a parameter changed -- call once "
                               "before capture")
        r = self.resnet_conv.resnet
        cp = -(-self.in_channels // K_CHUNK) * K_CHUNK
        out = {}

        def put(name, conv, bn, cin_pad=None):
            w, b = fold_bn(conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, cin_pad=cin_pad,
                           dtype=torch.float32)
            out[name] = (w.to(device), b.to(device))
        put("conv1", r.conv1, r.bn1, cp)
        for li in range(1, 5):
            for bi, blk in enumerate(getattr(r, f"layer{li}")):
                put(f"layer{li}.{bi}.conv1", blk.conv1, blk.bn1)
                put(f"layer{li}.{bi}.conv2", blk.conv2, blk.bn2)
                if blk.downsample is not None:
                    put(f"layer{li}.{bi}.downsample", blk.downsample[0], blk.downsample[1])
        put("tail", self.conv1[0], self.conv1[1])
        self._packed[str(device)] = (stamp, out)
        return out

    # ---- forward ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def map_size(H, W):
        """The layer-4 map of an H x W input: conv 7x7 s2 p3, max pool 3x3 s2 p1, then three 3x3 s2 p1 convolutions."""
        for k, p in ((7, 3), (3, 1), (3, 1), (3, 1), (3, 1)):
            H, W = conv_out(H, k, 2, p), conv_out(W, k, 2, p)
        return H, W

    def _check(self, img):
        if self.training:
            raise NotImplementedError("Encoder: the module is in training mode -- training the pose CNN (BatchNorm batch statistics, "
                                      "gradients through the convolutions) is not implemented; call .eval()")
        if not torch.is_tensor(img):
            raise TypeError(f"Encoder: expected a tensor, got {type(img)}")
        if img.requires_grad:
            raise NotImplementedError("Encoder: inputs that require grad are not implemented (the convolution kernels have no "
                                      "backward; the reference runs the PoseNet under no_grad); pass them detached")
        if img.dim() != 4 or img.shape[1] != self.in_channels or img.dtype != torch.float32 or img.shape[0] < 1:
            raise ValueError(f"Encoder: expected fp32 (B, {self.in_channels}, H, W), got {img.dtype} {tuple(img.shape)}")
        if min(img.shape[2:]) < 1 or self.map_size(*img.shape[2:]) != (4, 4):
            raise ValueError(f"Encoder: an input of {img.shape[2]} x {img.shape[3]} gives a layer-4 map of "
                             f"{self.map_size(*img.shape[2:])}, not 4 x 4 (ceil(H / 32) == ceil(W / 32) == 4, e.g. 112 x 112)")
        if not img.is_cuda:
            raise RuntimeError("Encoder takes CUDA (ROCm) tensors; the HIP library is the only compute path")

    def forward(self, img, normalize=False):
        """img (B,Cin,H,W) fp32 on the device -> (B,128).  normalize: F.normalize(img, 2, 1) first, inside the input kernel."""
        self._check(img)
        pk = self.packed(img.device)
        r = self.resnet_conv.resnet
        x = to_nhwc(img, cpad=pk["conv1"][0].shape[3], normalize=normalize)
        x = conv2d_nhwc(x, *pk["conv1"], stride=2, pad=3, act=ACT_RELU)
        x = maxpool3x3s2_nhwc(x)
        for li in range(1, 5):
            for bi, blk in enumerate(getattr(r, f"layer{li}")):
                name = f"layer{li}.{bi}"
                y = conv2d_nhwc(x, *pk[name + ".conv1"], stride=blk.stride, pad=1, act=ACT_RELU)
                idt = x if blk.downsample is None else conv2d_nhwc(x, *pk[name + ".downsample"], stride=blk.stride, pad=0)
                x = conv2d_nhwc(y, *pk[name + ".conv2"], stride=1, pad=1, res=idt, act=ACT_RELU)
        x = conv2d_nhwc(x, *pk["tail"], stride=1, pad=1, act=ACT_LEAKY)
        return max_over_positions(x)
