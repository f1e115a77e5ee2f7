"""What the clipping stage (moda_amd/train_utils.py, csrc/clip_kernels.hip) costs inside the training step, and what the
reference's route would cost in its place.  Three forms of bench_support.TrainHarness at the benchmark's training size:

  graph, clip off   the captured step as `bench.py --mode train` times it (forward + backward + AdamW)
  graph, clip on    the same with TrainHarness(clip_grad=True): three more launches inside the graph
  eager, torch      the eager step with the torch restatement of the reference's clip_grad (tests/clip_numpy.clip_grad_torch:
                    an isnan read-back per parameter, 22 clip_grad_norm_ calls) between the exchange and AdamW -- it cannot be
                    captured, so it is compared as the eager step it forces; `eager, clip off` is listed beside it

For each: the median step time over --steps synchronised steps after --warmup, and the device kernel launches of one step
(torch.profiler over the step issued eagerly).  Prints one JSON line; sets no gate -- the figures go into DESIGN.md.

  python tools/clip_grad_bench.py [--steps 30] [--warmup 5] [--n 2048] [--s 128]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def step_ms(h, steps, warmup):
    for _ in range(warmup):
        h.step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        h.step()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def launches(h):
    """Device kernels of one step ISSUED EAGERLY (the profiler does not see the kernels inside a graph replay; a captured step
    holds the launches its eager form issues), None when the profiler is not available."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--s", type=int, default=128)
    ap.add_argument("--clip-scale", type=float, default=10.0)
    a = ap.parse_args()
    import clip_numpy as cn
    from moda_amd import train_utils as TU
    from moda_amd.bench_support import TrainHarness
    factors = [f for _, f in TU.GRAD_GROUPS]
    res = dict(device=torch.cuda.get_device_name(0), N=a.n, S=a.s, steps=a.steps, clip_scale=a.clip_scale, forms={})
    forms = (("graph, clip off", dict(clip_grad=False), True, False), ("graph, clip on", dict(clip_grad=True), True, False),
             ("eager, clip off", dict(clip_grad=False), False, False), ("eager, torch", dict(clip_grad=True), False, True))
    for name, kw, graph, restated in forms:
        h = TrainHarness(N=a.n, S=a.s, clip_scale=a.clip_scale, **kw)
        if restated:
            h._clip = lambda h=h: cn.clip_grad_torch(h.named_params(), TU.grad_group, factors, a.clip_scale)
        if graph:
            h.capture(warm=3)
        else:
            for _ in range(3):
                h.step()
        ms = step_ms(h, a.steps, a.warmup)
        res["forms"][name] = dict(step_ms=ms, launches_per_step=launches(h), loss=h.loss())
        del h
        torch.cuda.empty_cache()
    f = res["forms"]
    res["clip_cost_in_graph_ms"] = f["graph, clip on"]["step_ms"] - f["graph, clip off"]["step_ms"]
    res["torch_route_cost_eager_ms"] = f["eager, torch"]["step_ms"] - f["eager, clip off"]["step_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
