"""What the device optimiser (moda_amd/optim.py, csrc/optim_kernels.hip) costs inside the training step and alone.

  step    the captured bench_support.TrainHarness step at the benchmark's training size with device_optimizer off (torch's fused
          AdamW at a constant rate, what `bench.py --mode train` times) and on (22 groups + OneCycleLR on the device), the two
          forms alternating inside one process: median step time over --steps synchronised steps after --warmup, and the device
          kernel launches of one step (torch.profiler over the step issued eagerly).
  stage   the optimiser stage alone over the harness's parameters and gradients: DeviceAdamW.step() against torch's fused
          AdamW(capturable=True) on clones of the same tensors, each captured into a graph of one step and replayed --replays
          times between two device events.  Both move the same bytes (4 reads, 3 writes per element).

Every run is a process of its own (--runs, default 3): the parent starts them one after the other, never opens the GPU itself, and
reports per figure the median over the runs and their range.  Prints one JSON line; sets no gate -- the figures go into DESIGN.md.

  python tools/optimizer_bench.py [--runs 3] [--steps 30] [--warmup 5] [--n 2048] [--s 128] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def launches(h):
    """Device kernels of one step ISSUED EAGERLY (the profiler does not see the kernels inside a graph replay; a captured step
    holds the launches its eager form issues), None when the profiler is not available."""
    import torch
    try:
        from torch.profiler import profile, ProfilerActivity
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            h.eager_step()
            torch.cuda.synchronize()
        dev = getattr(torch.autograd.DeviceType, "CUDA")
        return sum(1 for e in prof.events() if e.device_type == dev and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception as e:          # a figure that could not be taken is reported as missing, not guessed
        sys.stderr.write(f"launch count unavailable: {type(e).__name__}: {e}\n")
        return None


def replay_us(graph, replays):
    import torch
    for _ in range(10):
        graph.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / replays


def child(a):
    import numpy as np
    import torch
    from moda_amd.bench_support import TrainHarness
    from moda_amd.optim import DeviceAdamW
    res = dict(device=torch.cuda.get_device_name(0), step={}, stage={})
    forms = {"torch AdamW": dict(), "device optimiser": dict(device_optimizer=True, total_steps=a.total_steps, num_epochs=10)}
    hs = {}
    for name, kw in forms.items():
        hs[name] = TrainHarness(N=a.n, S=a.s, **kw)
        hs[name].capture(warm=3)
        for _ in range(a.warmup):
            hs[name].step()
    torch.cuda.synchronize()
    ts = {name: [] for name in hs}
    for _ in range(a.steps):                       # alternating: both forms see the same machine state
        for name, h in hs.items():
            t0 = time.perf_counter()
            h.step()
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    for name, h in hs.items():
        res["step"][name] = dict(step_ms=float(np.median(ts[name])), launches_per_step=launches(h), loss=h.loss())
    # the stage alone, over the gradients the last step left in the harness
    h = hs["torch AdamW"]
    named = [(n, p) for n, p in h.named_params() if p.grad is not None]
    res["stage"]["elements"] = int(sum(p.numel() for _, p in named))
    dev_params = [(n, torch.nn.Parameter(p.detach().clone())) for n, p in named]
    tor_params = [torch.nn.Parameter(p.detach().clone()) for _, p in named]
    for (_, q), r, (_, p) in zip(dev_params, tor_params, named):
        q.grad, r.grad = p.grad.detach().clone(), p.grad.detach().clone()
    dopt = DeviceAdamW(dev_params, 5e-4, a.total_steps, 0.2)
    topt = torch.optim.AdamW(tor_params, lr=2e-5, betas=(0.9, 0.999), weight_decay=1e-4, capturable=True, fused=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dopt.step()
        topt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gd, gt = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(gd):
        dopt.step()
    with torch.cuda.graph(gt):
        topt.step()
    res["stage"]["device optimiser"] = dict(us=replay_us(gd, a.replays), launches=2)
    res["stage"]["torch fused AdamW"] = dict(us=replay_us(gt, a.replays))
    res["stage"]["bytes"] = res["stage"]["elements"] * 4 * 7
    print("RESULT " + json.dumps(res), flush=True)


def spread(vals):
    import statistics
    vals = [v for v in vals if v is not None]
    return None if not vals else dict(median=statistics.median(vals), min=min(vals), max=max(vals))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--s", type=int, default=128)
    ap.add_argument("--total-steps", type=int, default=100000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    args = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    for _ in range(a.runs):
        out = subprocess.run(args, stdout=subprocess.PIPE, text=True, check=True).stdout
        runs.append(json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    res = dict(device=runs[0]["device"], N=a.n, S=a.s, steps=a.steps, runs=a.runs, step={}, stage={})
    for name in runs[0]["step"]:
        res["step"][name] = dict(step_ms=spread([r["step"][name]["step_ms"] for r in runs]),
                                 launches_per_step=runs[0]["step"][name]["launches_per_step"])
    on, off = "device optimiser", "torch AdamW"
    res["step"]["on_minus_off_ms"] = spread([r["step"][on]["step_ms"] - r["step"][off]["step_ms"] for r in runs])
    res["stage"] = dict(elements=runs[0]["stage"]["elements"], bytes=runs[0]["stage"]["bytes"],
                        device_optimiser_us=spread([r["stage"][on]["us"] for r in runs]), device_optimiser_launches=2,
                        torch_fused_adamw_us=spread([r["stage"]["torch fused AdamW"]["us"] for r in runs]))
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
