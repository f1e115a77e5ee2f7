"""Generate tests/golden/g38_posecnn.npz by running the reference's own PoseNet on the CPU (development container only, like
gen_golden_root_pose.py): nnutils/nerf.py's Encoder (over its ResNetConv and conv2d block) and RTHead(use_quat=True, D=1) in
eval mode, then refine_rt on create_base_se3 (nnutils/moda.py, compiled from its syntax tree as gen_golden_root_pose.py does) and
the K row of convert_root_pose -- in float64 and in float32, on the weights of tests/posecnn_torch.make_state(SEED) and the two
inputs of golden_inputs().

torchvision is absent here.  ResNetConv only needs `torchvision.models.resnet18(pretrained=True)` to return a module with the
attributes conv1, bn1, relu, maxpool, layer1..4 and fc; this generator installs a stand-in built from plain torch.nn layers with
ResNet-18's published topology.  The `pretrained` argument is ignored -- every weight is overwritten by make_state -- so nothing
is fetched.

Stored: the state dict's key names, the two inputs (float32, zero outside a blob, so they compress), per input the features
(B,128), the head's output (B,1,12) and rtk (B,4,4) in both precisions, the intrinsics and data ids used.  The weights are not
stored: the tests draw them again from the seed.

    python tests/golden/gen_golden_posecnn.py
"""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_import  # noqa: E402
import posecnn_torch as PT  # noqa: E402
from gen_golden_root_pose import moda_static_methods  # noqa: E402


class BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


class ResNet18(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = nn.Sequential(BasicBlock(64, 64, 1), BasicBlock(64, 64, 1))
        self.layer2 = nn.Sequential(BasicBlock(64, 128, 2), BasicBlock(128, 128, 1))
        self.layer3 = nn.Sequential(BasicBlock(128, 256, 2), BasicBlock(256, 256, 1))
        self.layer4 = nn.Sequential(BasicBlock(256, 512, 2), BasicBlock(512, 512, 1))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512, 1000)


def install_torchvision_stub():
    tv = sys.modules.get("torchvision") or types.ModuleType("torchvision")
    models = types.ModuleType("torchvision.models")
    models.resnet18 = lambda pretrained=False, **kw: ResNet18()
    tv.models = models
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, models


def main():
    _ref_import.install_stubs()
    install_torchvision_stub()
    _, nerf, geom, _ = _ref_import.import_reference()
    refine_rt, create_base_se3, _ = moda_static_methods(geom)
    sd = PT.state_tensors(PT.make_state(PT.SEED))
    out = {"ks": PT.KS}

    def posenet(dt):
        m = nn.Sequential(nerf.Encoder((112, 112), in_channels=16, out_channels=128),
                          nerf.RTHead(use_quat=True, D=1, in_channels_xyz=128, in_channels_dir=0, out_channels=7, raw_feat=True))
        m.load_state_dict(sd, strict=True)
        return m.to(dt).eval()

    out["keys"] = np.asarray(list(posenet(torch.float32).state_dict().keys()))
    for tag, img in zip(("a", "b"), PT.golden_inputs()):
        B = img.shape[0]
        dataid = np.arange(B) % len(PT.KS)
        out[f"x_{tag}"], out[f"dataid_{tag}"] = img, dataid
        for dt, suffix in ((torch.float64, "64"), (torch.float32, "32")):
            m = posenet(dt)
            with torch.no_grad():
                feat = m[0](torch.from_numpy(img).to(dt))
                rts = m[1](feat)
                rtk = torch.zeros(B, 4, 4, dtype=dt)
                rtk[:, :3] = create_base_se3(B, "cpu").to(dt)
                rtk = refine_rt(rtk, rts)
                rtk[:, 3] = torch.from_numpy(PT.KS).to(dt)[torch.from_numpy(dataid)]
            out[f"feat_{tag}_{suffix}"], out[f"rts_{tag}_{suffix}"], out[f"rtk_{tag}_{suffix}"] = feat.numpy(), rts.numpy(), rtk.numpy()
        for k in ("feat", "rts", "rtk"):
            ref = out[f"{k}_{tag}_64"]
            print(f"  {k}_{tag}: max |fp32 - fp64| / max |fp64| = "
                  f"{np.abs(out[f'{k}_{tag}_32'].astype(np.float64) - ref).max() / np.abs(ref).max():.3e}")
    path = os.path.join(HERE, "g38_posecnn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
