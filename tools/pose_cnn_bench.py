"""Time the PoseNet stage of extract_cams -- Encoder + RTHead + refine_rt on create_base_se3 + the K row, 112 x 112 inputs -- at
B = 50 (the reference's chunk) and B = 1, on the HIP kernels (moda_amd.Encoder, convert_root_pose(dp_feats=)) and on the
reference's route restated in torch on the same device: F.conv2d / F.batch_norm / F.max_pool2d / F.linear in fp32, eval mode, TF32
off.  Both run the same weights.  Reports eager time, graph-replay time and the launch count of each (kernels seen by
torch.profiler), and the largest difference of the two results.  One JSON line per process; --runs N starts N fresh processes and
writes their medians and ranges to profiles/posecnn/pose_cnn_bench.json.

    python tools/pose_cnn_bench.py --runs 3
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GFLOP_PER_FRAME = 1.25          # the convolutions of the trunk and the tail at 112 x 112 (2 flops per multiply-add)


def torch_posenet(sd, ks):
    """The reference's route (nerf.py:513-573, 307-344; moda.py:1025-1033, 1450-1466) as plain torch calls on the state dict sd."""
    import torch
    import torch.nn.functional as F

    def bn(x, p):
        return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)

    def run(img, dataid):
        r = "0.resnet_conv.resnet."
        x = F.max_pool2d(F.relu(bn(F.conv2d(img, sd[r + "conv1.weight"], None, 2, 3), r + "bn1")), 3, 2, 1)
        for li in range(1, 5):
            for bi in range(2):
                p = f"{r}layer{li}.{bi}"
                s = 2 if (li > 1 and bi == 0) else 1
                y = F.relu(bn(F.conv2d(x, sd[p + ".conv1.weight"], None, s, 1), p + ".bn1"))
                y = bn(F.conv2d(y, sd[p + ".conv2.weight"], None, 1, 1), p + ".bn2")
                if p + ".downsample.0.weight" in sd:
                    x = bn(F.conv2d(x, sd[p + ".downsample.0.weight"], None, s, 0), p + ".downsample.1")
                x = F.relu(y + x)
        x = F.leaky_relu(bn(F.conv2d(x, sd["0.conv1.0.weight"], sd["0.conv1.0.bias"], 1, 1), "0.conv1.1"), 0.2)
        feat = F.max_pool2d(x, 4, 4).view(img.shape[0], -1)
        h = F.relu(F.linear(feat, sd["1.xyz_encoding_1.0.weight"], sd["1.xyz_encoding_1.0.bias"]))
        h = F.linear(h, sd["1.xyz_encoding_final.weight"], sd["1.xyz_encoding_final.bias"])
        h = F.relu(F.linear(h, sd["1.dir_encoding.0.weight"], sd["1.dir_encoding.0.bias"]))
        rts = F.linear(h, sd["1.rgb.0.weight"], sd["1.rgb.0.bias"])
        q = F.normalize(rts[:, 3:7], 2, -1)
        a, i, j, k = q.unbind(-1)
        ts = 2.0 / (q * q).sum(-1)
        R = torch.stack((1 - ts * (j * j + k * k), ts * (i * j - k * a), ts * (i * k + j * a), ts * (i * j + k * a),
                         1 - ts * (i * i + k * k), ts * (j * k - i * a), ts * (i * k - j * a), ts * (j * k + i * a),
                         1 - ts * (i * i + j * j)), -1).view(-1, 3, 3)
        rtk = torch.zeros(img.shape[0], 4, 4, device=img.device)
        rtk[:, :3, :3] = R                                  # refine_rt on create_base_se3: R0 = I, t0 = (0, 0, 0.3)
        rtk[:, :3, 3] = rts[:, :3] * 0.1
        rtk[:, 2, 3] += 0.3
        rtk[:, 3] = ks[dataid]
        return rtk
    return run


def one_process(steps):
    import torch
    import moda_amd
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = "cuda"
    net = torch.nn.Sequential(moda_amd.Encoder((112, 112), in_channels=16),
                              moda_amd.RTHead(use_quat=True, D=1, in_channels_xyz=128, in_channels_dir=0, out_channels=7, raw_feat=True))
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():                                   # BatchNorm statistics and head biases that are not the identity
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=gen) * 0.3)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=gen) * 1.5 + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.2)
    net = net.to(dev).eval()
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    ks = torch.tensor([[300., 500., 200., 250.]], device=dev)
    plain_net = torch_posenet(sd, ks)

    def timed(fn, n):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    res = {}
    for B in (50, 1):
        img = torch.randn((B, 16, 112, 112), generator=gen).to(dev)
        img = moda_amd.pose_cnn.normalize_feats(img * (torch.rand((B, 1, 112, 112), generator=gen) > 0.7).to(dev))
        fid = torch.arange(B, device=dev)
        dataid = torch.zeros(B, dtype=torch.int64, device=dev)
        outs = {}

        def hip():
            outs["hip"] = moda_amd.convert_root_pose(net, fid, dataid, ks, dp_feats=img)

        def plain():
            outs["torch"] = plain_net(img, dataid)

        with torch.no_grad():
            for name, fn in (("hip", hip), ("torch", plain)):
                for _ in range(3):
                    fn()
                res[f"{name}_eager_ms_B{B}"] = timed(fn, steps)
                with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                    fn()
                    torch.cuda.synchronize()
                res[f"{name}_launches_B{B}"] = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.stream(side):
                    fn()
                    with torch.cuda.graph(graph, stream=side):
                        fn()
                torch.cuda.current_stream().wait_stream(side)
                res[f"{name}_replay_ms_B{B}"] = timed(graph.replay, steps)
            res[f"hip_replay_tflops_B{B}"] = GFLOP_PER_FRAME * B / res[f"hip_replay_ms_B{B}"]
            res[f"max_abs_diff_rt_B{B}"] = float((outs["hip"][:, :3] - outs["torch"][:, :3]).abs().max())
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=0, help="start this many fresh processes and write their medians and ranges")
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    if a.runs <= 0:
        return one_process(a.steps)
    rows = []
    for _ in range(a.runs):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(a.steps)], capture_output=True, text=True, timeout=400)
        line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
        if out.returncode != 0 or not line:
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
            raise SystemExit(f"a timing process ended with {out.returncode}")
        rows.append(json.loads(line[-1][7:]))
    from moda_amd import build
    summary = {"source_hash": build.source_hash(), "processes": len(rows), "sizes": {"H": 112, "W": 112, "C": 16, "B": [50, 1]},
               "median": {k: statistics.median(r[k] for r in rows) for k in rows[0]},
               "ranges": {k: [min(r[k] for r in rows), max(r[k] for r in rows)] for k in rows[0]}}
    path = os.path.join(ROOT, "profiles", "posecnn", "pose_cnn_bench.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    json.dump(summary, open(path, "w"), indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
