"""Time the root-pose stage of a training step at the reference's sizes -- compute_rts over T = 500 frames, convert_root_pose and
prepare_ray_cams for a batch of 512 ids over 32 frames, forward and backward -- on the HIP kernels and on the same chain restated in
plain torch ops on the device (what a user has without moda_root_pose / moda_ray_cams); the MLP is the package's in both.
Reports eager time, graph-replay time and the launch count of each (kernels seen by torch.profiler), and the captured harness step
with root_pose on and off.  One JSON line per process; --runs N starts N fresh processes and writes their ranges to
profiles/rootpose/root_pose_bench.json.

    python tools/root_pose_bench.py --runs 3
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_chain(m, frameid, dataid, ks, kaug, T):
    """The chain in plain torch ops (nerf.py:382-470, moda.py:1025-1046, 1419-1495 restated)."""
    import torch

    def quat_mat(q):
        q = torch.nn.functional.normalize(q, 2, -1)
        r, i, j, k = q.unbind(-1)
        ts = 2.0 / (q * q).sum(-1)
        return torch.stack((1 - ts * (j * j + k * k), ts * (i * j - k * r), ts * (i * k + j * r), ts * (i * j + k * r),
                            1 - ts * (i * i + k * k), ts * (j * k - i * r), ts * (i * k - j * r), ts * (j * k + i * r),
                            1 - ts * (i * i + j * j)), -1).reshape(-1, 3, 3)

    def so3(w):
        th = (w * w).sum(1).clamp(min=1e-4).sqrt()
        K = w.new_zeros((w.shape[0], 3, 3))
        x, y, z = w.unbind(1)
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -z, y, z, -x, -y, x
        return (th.sin() / th)[:, None, None] * K + ((1 - th.cos()) / (th * th))[:, None, None] * torch.bmm(K, K) + torch.eye(3, device=w.device)[None]

    def poses(ids):
        rows = m.base_rt.se3[ids]
        Rb, tb = quat_mat(rows[:, 3:7]), rows[:, :3] * 0.1
        Rb, tb = Rb * 10 - (Rb * 9).detach(), tb * 10 - (tb * 9).detach()
        d = m.delta_rows(ids)
        Rd, td = so3(d[:, 3:6]), d[:, :3] * 0.1
        t = tb + Rb.matmul(td[..., None])[..., 0]
        R = Rb.matmul(Rd)
        rt = torch.zeros(len(ids), 3, 4, device=ids.device)
        rt[:, :3, :3] = torch.eye(3, device=ids.device)[None]
        rt[:, 2, 3] = 0.3
        R0, t0 = rt[:, :3, :3].clone(), rt[:, :3, 3].clone()
        rt[:, :3, 3] = t0 + R0.matmul(t[..., None])[..., 0]
        rt[:, :3, :3] = R0.matmul(R)
        return rt

    from moda_amd.geom_utils import K2inv, K2mat, Kmatinv
    rtk_all = poses(torch.arange(T, device=frameid.device))
    rtk = torch.zeros(len(frameid), 4, 4, device=frameid.device)
    rtk[:, :3] = poses(frameid)
    rtk[:, 3] = ks[dataid]
    Kinv = Kmatinv(K2inv(kaug).matmul(K2mat(rtk[:, 3])))
    return rtk_all, rtk[:, :3, :3], rtk[:, :3, 3], Kinv


def one_process(steps):
    import numpy as np
    import torch
    import moda_amd
    from moda_amd import bench_support as BS, root_pose as RP, geom_utils as GU
    dev = "cuda"
    T, bs, frames = 500, 512, 32
    m = BS.make_root_rts(T, (0, T)).to(dev).train()
    ks = torch.nn.Parameter(torch.tensor([[300., 500., 200., 250.]], device=dev))
    gen = np.random.default_rng(0)
    frameid = torch.as_tensor(np.repeat(gen.choice(T, frames, replace=False), bs // frames), device=dev)
    dataid = torch.zeros(bs, dtype=torch.int64, device=dev)
    kaug = torch.as_tensor(np.abs(gen.normal(size=(bs, 4))) + 0.5, dtype=torch.float32, device=dev)
    w = [torch.randn(s, device=dev) for s in ((T, 3, 4), (bs, 3, 3), (bs, 3), (bs, 3, 3))]
    params = list(m.parameters()) + [ks]

    def hip():
        rt = RP.compute_rts(m, T)
        R, Tm, Ki = GU.prepare_ray_cams(RP.convert_root_pose(m, frameid, dataid, ks), kaug)
        return rt, R, Tm, Ki

    def plain():
        return torch_chain(m, frameid, dataid, ks, kaug, T)

    def fwd_bwd(fn):
        for p in params:
            p.grad = None
        outs = fn()
        sum((a * b).sum() for a, b in zip(w, outs)).backward()

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
    for name, fn in (("hip", hip), ("torch", plain)):
        for _ in range(3):
            fwd_bwd(fn)
        res[name + "_eager_ms"] = timed(lambda: fwd_bwd(fn), steps)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            fwd_bwd(fn)
            torch.cuda.synchronize()
        res[name + "_launches"] = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            fwd_bwd(fn)
            with torch.cuda.graph(graph, stream=side):
                fwd_bwd(fn)
        torch.cuda.current_stream().wait_stream(side)
        res[name + "_replay_ms"] = timed(graph.replay, steps)
    for flag in (False, True):
        h = BS.TrainHarness(default_losses=True, root_pose=flag)
        h.capture()
        for _ in range(3):
            h.step()
        res[f"harness_step_ms_root_pose_{int(flag)}"] = timed(h.step, max(5, steps // 4))
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=0, help="start this many fresh processes and write their ranges")
    ap.add_argument("--steps", type=int, default=40)
    a = ap.parse_args()
    if a.runs <= 0:
        return one_process(a.steps)
    rows = []
    for _ in range(a.runs):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(a.steps)], capture_output=True, text=True, timeout=900)
        line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
        if out.returncode != 0 or not line:
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
            raise SystemExit(f"a timing process ended with {out.returncode}")
        rows.append(json.loads(line[-1][7:]))
    from moda_amd import build
    summary = {"source_hash": build.source_hash(), "processes": len(rows), "sizes": {"T": 500, "batch": 512, "frames": 32},
               "ranges": {k: [min(r[k] for r in rows), max(r[k] for r in rows)] for k in rows[0]}}
    path = os.path.join(ROOT, "profiles", "rootpose", "root_pose_bench.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    json.dump(summary, open(path, "w"), indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
