"""Nearest-neighbour timing (moda_amd/mesh_eval.py, csrc/pointset_kernels.hip): moda_nn_fwd against what a user could write
with torch alone, a row-chunked `torch.cdist(x_chunk, y).min(dim=1)` on the same GPU, the chunk chosen as the largest power of
two that keeps the (chunk, M) distance matrix under 2 GB.  Sizes: N = M in {16384, 65536, 262144} and the skewed
N = 1500, M = 262144 (the split-over-targets route), B = 1, uniform points in [-1, 1]^3.  Each of --procs fresh processes,
one after the other: warm-up, then the median of --reps synchronised calls per side; the two index results are compared.
Gate, a condition and not a tuned figure: at 262144 x 262144, in EVERY process, moda_nn_fwd takes no longer than the torch
baseline.  Also recorded, without a gate: one full eval_mesh at 262144 x 65536 vertices (time, ICP iterations).

  python tools/nn_bench.py [--procs 5] [--reps 10] [--out profiles/mesh/nn_bench.json]
  python tools/nn_bench.py --eval-only       # the eval_mesh call alone, once: the program to put after `rocprofv3 ... --`"""
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

SIZES = ((16384, 16384), (65536, 65536), (262144, 262144), (1500, 262144))
GATE = "262144x262144"


def timed(fn, reps, warm=2):
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


def baseline_chunk(M):
    c = 1
    while 2 * c * M * 4 < 2e9:
        c *= 2
    return c


def torch_nearest(x, y, chunk):
    d, i = [], []
    for a in range(0, x.shape[0], chunk):
        m = torch.cdist(x[a:a + chunk], y).min(dim=1)
        d.append(m.values)
        i.append(m.indices)
    return torch.cat(d), torch.cat(i)


def surface(n, seed):
    """n points of the bumpy ellipsoid of the ICP tests (tests/pointset_numpy.py icp_case), shifted to depth 1."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn((n, 3), generator=g, dtype=torch.float64)
    u = u / u.norm(dim=1, keepdim=True)
    p = u * torch.tensor([0.30, 0.18, 0.11], dtype=torch.float64) * (1 + 0.25 * torch.sin(5 * u[:, :1]) * torch.cos(3 * u[:, 1:2]))
    return p + torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)


def eval_case():
    gt = surface(65536, 1)
    t = np.deg2rad(5.0)
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = torch.from_numpy(np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K)
    pred = surface(262144, 2) @ R + torch.tensor([0.02, -0.01, 0.03], dtype=torch.float64)
    return pred.float().cuda(), gt.float().cuda()


def run_eval(reps):
    import moda_amd
    pred, gt = eval_case()
    out = moda_amd.eval_mesh(pred, gt)                                       # warm-up, and the figures
    ms = timed(lambda: moda_amd.eval_mesh(pred, gt), reps, warm=0) if reps else None
    return dict(vertices=int(pred.shape[0]), vertices_gt=int(gt.shape[0]), eval_mesh_ms=ms, icp_iterations=len(out["icp"].t_history),
                icp_converged=bool(out["icp"].converged), cd=out["cd"], f001=out["f001"], f002=out["f002"], f005=out["f005"])


def child(a):
    import moda_amd
    from moda_amd import mesh_eval as ME
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, sizes={})
    for N, M in SIZES:
        g = torch.Generator().manual_seed(N + 7 * M)
        x = (torch.rand((N, 3), generator=g) * 2 - 1).cuda()
        y = (torch.rand((M, 3), generator=g) * 2 - 1).cuda()
        chunk = min(baseline_chunk(M), N)
        t_k = timed(lambda: ME._nearest(x[None], y[None]), a.reps)
        t_b = timed(lambda: torch_nearest(x, y, chunk), max(3, a.reps // 2), warm=1)
        _, ik = ME._nearest(x[None], y[None])
        _, ib = torch_nearest(x, y, chunk)
        splits, rng = ME.nn_plan(1, N, M)
        res["sizes"][f"{N}x{M}"] = dict(moda_nn_fwd_ms=t_k, torch_cdist_min_ms=t_b, ratio_torch_over_moda=t_b / t_k,
                                        pair_evaluations_per_s=N * M / (t_k * 1e-3), baseline_chunk_rows=chunk,
                                        baseline_matrix_bytes=chunk * M * 4, target_ranges=splits,
                                        index_agreement=float((ik[0].long() == ib).float().mean()))
    res["eval_mesh"] = run_eval(max(1, a.reps // 5))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--procs", type=int, default=5)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--eval-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh", "nn_bench.json"))
    a = ap.parse_args()
    if a.eval_only:
        print(json.dumps(run_eval(0)))
        return
    if a.child:
        child(a)
        return
    runs = []
    for k in range(a.procs):                          # one fresh process per run, one after the other; stop at the first failure
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=420)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"run {k} failed with {p.returncode}")
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(k, json.dumps({s: [round(r["moda_nn_fwd_ms"], 3), round(r["torch_cdist_min_ms"], 3)]
                             for s, r in runs[-1]["sizes"].items()}), flush=True)
    ratios = [r["sizes"][GATE]["ratio_torch_over_moda"] for r in runs]
    res = dict(device=runs[0]["device"], reps=a.reps, procs=a.procs, runs=runs,
               gate=dict(size=GATE, condition="moda_nn_fwd_ms <= torch_cdist_min_ms in every process",
                         ratios_torch_over_moda=ratios, min_ratio=min(ratios), ok=min(ratios) >= 1.0))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res["gate"]))
    if not res["gate"]["ok"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
