"""Time the bone-location term's Sinkhorn divergence at the workload's shapes, (25, 1000) and (36, 1000) points, one JSON line:

  call    moda_amd.samples_loss.SamplesLoss forward + backward, issued eagerly and replayed from a captured graph, against the
          tensorized route of geomloss 0.2.4 restated in torch on the same device, `.item()` of the diameter included -- what the
          reference would run.  The three are interleaved repetition by repetition in one process; launch counts for both.
  step    the captured TrainHarness step (default_losses) with and without the term.

Medians (p10, p90) of synchronised repetitions after a warm-up; run it twice and report both (DESIGN section 5 on spread).

    python tools/sinkdiv_bench.py [--reps 50]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from moda_amd.samples_loss import SamplesLoss  # noqa: E402
from moda_amd.bench_support import TrainHarness  # noqa: E402

SHAPES = ((25, 1000), (36, 1000))


def clouds(N, M, dev, seed=0):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.randn((N, 3), device=dev, generator=g)
    v = torch.randn((M, 3), device=dev, generator=g)
    y = v / v.norm(dim=1, keepdim=True) * torch.tensor([3.0, 2.0, 2.5], device=dev)
    return x.requires_grad_(True), y


class TorchRoute:
    """geomloss 0.2.4, sinkhorn_divergence.py, tensorized: uniform weights, p = 2, blur .05, scaling .5, debias."""

    def __init__(self):
        self.launches = 0

    def __call__(self, x, y, blur=0.05, scaling=0.5):
        N, M = x.shape[0], y.shape[0]
        la, lb = torch.full((N,), 1.0 / N, device=x.device).log(), torch.full((M,), 1.0 / M, device=x.device).log()
        pts = torch.cat([x, y], 0).detach()
        d = (pts.max(0).values - pts.min(0).values).norm().item()                      # max_diameter: the host waits here
        eps_s = [d ** 2] + [math.exp(e) for e in np.arange(2 * math.log(d), 2 * math.log(blur), 2 * math.log(scaling))] + [blur ** 2]

        def cost(u, v):                                                                # squared_distances / 2
            return ((u * u).sum(-1)[:, None] + (v * v).sum(-1)[None, :] - 2 * u @ v.t()) / 2

        def softmin(eps, C, h):
            return -eps * (h[None, :] - C / eps).logsumexp(1)

        C_xx, C_yy, C_xy, C_yx = cost(x, x.detach()), cost(y, y.detach()), cost(x, y.detach()), cost(y, x.detach())
        with torch.no_grad():
            eps = eps_s[0]
            a_x, b_y, a_y, b_x = softmin(eps, C_xx, la), softmin(eps, C_yy, lb), softmin(eps, C_yx, la), softmin(eps, C_xy, lb)
            for eps in eps_s:
                at_x, bt_y = softmin(eps, C_xx, la + a_x / eps), softmin(eps, C_yy, lb + b_y / eps)
                at_y, bt_x = softmin(eps, C_yx, la + b_x / eps), softmin(eps, C_xy, lb + a_y / eps)
                a_x, b_y, a_y, b_x = 0.5 * (a_x + at_x), 0.5 * (b_y + bt_y), 0.5 * (a_y + at_y), 0.5 * (b_x + bt_x)
        eps = eps_s[-1]
        a_x, b_y = softmin(eps, C_xx, (la + a_x / eps).detach()), softmin(eps, C_yy, (lb + b_y / eps).detach())
        a_y, b_x = softmin(eps, C_yx, (la + b_x / eps).detach()), softmin(eps, C_xy, (lb + a_y / eps).detach())
        return (b_x - a_x).mean() + (a_y - b_y).mean()


def count_launches(fn):
    from torch.profiler import profile, ProfilerActivity
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return int(sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA))


def stats(ts):
    ts = np.sort(np.asarray(ts))
    return dict(median_ms=round(float(np.median(ts)), 4), p10_ms=round(float(ts[len(ts) // 10]), 4), p90_ms=round(float(ts[(9 * len(ts)) // 10]), 4))


def interleaved(fns, reps, warm=10):
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: stats(v) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda")
    out = {"reps": a.reps, "call": {}}
    for N, M in SHAPES:
        x, y = clouds(N, M, dev)
        ours, theirs = SamplesLoss("sinkhorn", p=2, blur=.05), TorchRoute()

        def eager():
            x.grad = None
            ours(x, y).backward()

        def torch_route():
            x.grad = None
            theirs(x, y).backward()

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                eager()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        x.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ours(x, y).backward()
        res = interleaved({"eager": eager, "graph_replay": graph.replay, "torch_route": torch_route}, a.reps)
        res["schedule_steps"] = int(ours.status[1])
        res["launches"] = {"ours": count_launches(eager), "torch_route": count_launches(torch_route)}
        out["call"][f"{N}x{M}"] = res
    for name, on in (("step_bone_loc_off", False), ("step_bone_loc_on", True)):
        h = TrainHarness(N=2048, S=128, precision="bf16", default_losses=True, bone_loc=on)
        h.capture(warm=3)
        out[name] = interleaved({"step": h.step}, a.reps, warm=5)["step"]
        del h
    print(json.dumps(out))


if __name__ == "__main__":
    main()
