"""Warm-up step timing (moda_amd/warmup.py, csrc/warmup_kernels.hip): one optimiser step of the shape warm-up at the reference's
size -- 10 000 points, the 8 x 256 coarse network -- in the bf16 and the exact fp32 training precision, three ways:

  eager     WarmupHarness.step(): device draw, moda_shape_target, train_forward(sigma_only), the shape-loss pair, GradClipper,
            DeviceAdamW;
  replayed  the same step captured as one graph, replayed after each draw;
  torch     the reference's route restated in torch around this project's own train_forward on the same commit: torch.rand on the
            host and its upload, torch operations for the samples, the target and the squared error, torch's clip_grad_norm_ and
            fused AdamW (constant rate: a host-side scheduler would add its own work).

Each of --procs fresh processes, one after the other: warm-up, then the median of --reps synchronised steps per form, and the
kernel launches of one step counted with torch's profiler.  The recorded losses are NOT comparable between the routes: the
device route follows OneCycleLR, which over the bench's 5 x 10^6 scheduled steps stays near learning_rate / 25, while the torch
route steps at the constant learning_rate; the timed work is the same.  Nothing is gated: the step is expected to be dominated by the
network, so what is recorded is the figures and whether the device route lies outside the run-to-run spread of the torch route.

  python tools/warmup_bench.py [--procs 3] [--reps 30] [--out profiles/warmup/warmup_bench.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

NSAMPLE, V = 10000, 2000
OPTS = dict(warmup_shape_ep=5, bound_factor=2, init_ellips=False, learning_rate=5e-4, clip_scale=10.)


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def count_launches(fn):
    from torch.profiler import profile, ProfilerActivity
    try:
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return int(sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA))
    except Exception as e:                        # a profiler that cannot attach is reported, not hidden
        return f"not counted ({type(e).__name__})"


def make_net():
    import moda_amd
    torch.manual_seed(1)
    return moda_amd.NeRF(D=8, W=256, in_channels_xyz=63, in_channels_dir=27).cuda().train(), moda_amd.Embedding(3, 10)


def template():
    g = torch.Generator().manual_seed(2)
    return ((torch.rand((V, 3), generator=g) * 2 - 1) * torch.tensor([1.0, 0.6, 0.35])).cuda()


class TorchRoute:
    """The reference's step with torch's own operations everywhere but the network."""

    def __init__(self, net, emb, verts):
        self.net, self.emb = net, emb
        self.pts = verts * 0.1
        self.params = [p for n, p in net.named_parameters() if n.startswith("sigma.") or (n.startswith("xyz_encoding_") and "final" not in n)]
        self.opt = torch.optim.AdamW(self.params, lr=OPTS["learning_rate"], betas=(0.9, 0.999), weight_decay=1e-4, fused=True)
        self.loss = None

    def step(self):
        obj_bound = self.pts.abs().max(0)[0][None, None]
        bound = obj_bound * (OPTS["bound_factor"] * 1.2)
        pts_samp = torch.rand(1, NSAMPLE, 3).cuda() * 2 * bound - bound
        dis = torch.sqrt(pts_samp.pow(2).sum(2).view(-1)) - obj_bound.min()
        y = self.net.train_forward(pts_samp, self.emb, sigma_only=True)
        loss = (-y.view(-1) - dis).pow(2).mean()
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.params, OPTS["clip_scale"])
        self.opt.step()
        self.loss = loss.detach()


def child(a):
    import moda_amd
    from moda_amd import warmup
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, shape=dict(nsample=NSAMPLE, D=8, W=256), precisions={},
               loss_note="losses are not comparable between the routes: the device route follows OneCycleLR (near learning_rate / 25 "
                         "over the scheduled steps), the torch route steps at the constant learning_rate; the timed work is the same")
    for prec in ("bf16", "fp32"):
        moda_amd.set_train_precision(prec)
        verts = template()
        net, emb = make_net()
        eager = warmup.WarmupHarness(net, emb, verts, OPTS, steps_per_epoch=10 ** 6, nsample=NSAMPLE)
        t_e = timed(eager.step, a.reps)
        n_e = count_launches(eager.step)
        net, emb = make_net()
        graph = warmup.WarmupHarness(net, emb, verts, OPTS, steps_per_epoch=10 ** 6, nsample=NSAMPLE)
        graph.capture()
        t_g = timed(graph.step, a.reps)
        n_g = count_launches(graph.step)
        net, emb = make_net()
        ref = TorchRoute(net, emb, verts)
        t_t = timed(ref.step, a.reps)
        n_t = count_launches(ref.step)
        res["precisions"][prec] = dict(eager_ms=t_e, replayed_ms=t_g, torch_route_ms=t_t, launches=dict(eager=n_e, replayed=n_g, torch_route=n_t),
                                       loss=dict(eager=eager.loss(), replayed=graph.loss(), torch_route=float(ref.loss)))
    moda_amd.set_train_precision("fp32")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warmup", "warmup_bench.json"))
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    runs = []
    for k in range(a.procs):                          # one fresh process per run, one after the other; stop at the first failure
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"run {k} failed with {p.returncode}")
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(k, json.dumps({pr: {n: round(v, 3) for n, v in r.items() if n.endswith("_ms")} for pr, r in runs[-1]["precisions"].items()}),
              flush=True)
    summary = {}
    for prec in runs[0]["precisions"]:
        col = lambda n: [r["precisions"][prec][n] for r in runs]
        e, g, t = col("eager_ms"), col("replayed_ms"), col("torch_route_ms")
        summary[prec] = dict(eager_ms=e, replayed_ms=g, torch_route_ms=t,
                             eager_outside_torch_spread=max(e) < min(t), replayed_outside_torch_spread=max(g) < min(t),
                             launches=runs[0]["precisions"][prec]["launches"])
    res = dict(device=runs[0]["device"], reps=a.reps, procs=a.procs, summary=summary, runs=runs, loss_note=runs[0]["loss_note"],
               note="outside_torch_spread: the slowest process of the device route is faster than the fastest process of the torch route")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
