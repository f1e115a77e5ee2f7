"""k-means and surface-sampling timing (moda_amd/bones.py, csrc/bones_kernels.hip) against what a user could write with torch
alone on the same GPU.

  kmeans   N in {16384, 262144, 1048576} uniform points in [-1, 1]^3, K = 25, a fixed 20 iterations (tol = 0, iter_limit = 20),
           the same K start indices on both sides.  Baseline: kmeans_pytorch's loop restated in torch -- broadcast (N,K,3)
           differences, squared, summed, argmin; per cluster nonzero / index_select / mean; the shift test read on the host each
           iteration.
  sampler  F in {100000, 1000000} faces (random vertex triples of a 50 000-vertex cloud), S = 1000.  Baseline: cross-product
           areas, torch.multinomial with replacement, gathers and pytorch3d's barycentric formula.
Each of --procs fresh processes, one after the other: warm-up, then the median of --reps synchronised calls per side.
Gate, a condition and not a tuned figure: at EVERY listed size, in EVERY process, the moda_amd call takes no longer than the
torch baseline.

  python tools/kmeans_bench.py [--procs 3] [--reps 10] [--out profiles/mesh/kmeans_bench.json]"""
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

KMEANS_N = (16384, 262144, 1048576)
K, ITERS = 25, 20
SAMPLER_F = (100000, 1000000)
S = 1000


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


def torch_kmeans(X, init, iters):
    """The package's loop (kmeans_pytorch/__init__.py: pairwise_distance, argmin, the per-cluster loop, the host-side test)."""
    state = X[init].clone()
    it = 0
    while True:
        dis = ((X.unsqueeze(1) - state.unsqueeze(0)) ** 2.0).sum(dim=-1).squeeze()
        choice = torch.argmin(dis, dim=1)
        pre = state.clone()
        for index in range(state.shape[0]):
            selected = torch.nonzero(choice == index).squeeze()
            selected = torch.index_select(X, 0, selected)
            if selected.shape[0] == 0:
                selected = X[torch.randint(len(X), (1,))]
            state[index] = selected.mean(dim=0)
        shift = torch.sum(torch.sqrt(torch.sum((state - pre) ** 2, dim=1)))
        it += 1
        if float(shift) ** 2 < 0.0 or it >= iters:                           # tol = 0: the read-back stays, the test never passes
            return choice, state


def torch_sample(verts, faces, u):
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    areas = 0.5 * torch.linalg.cross(b - a, c - a).norm(dim=1)
    idx = torch.multinomial(areas, u.shape[0], replacement=True)
    s = u[:, 1].sqrt()
    w0, w1, w2 = 1 - s, s * (1 - u[:, 2]), s * u[:, 2]
    return w0[:, None] * a[idx] + w1[:, None] * b[idx] + w2[:, None] * c[idx]


def child(a):
    import moda_amd
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, kmeans={}, sampler={})
    for N in KMEANS_N:
        g = torch.Generator().manual_seed(N)
        X = (torch.rand((N, 3), generator=g) * 2 - 1).cuda()
        init = torch.randperm(N, generator=g)[:K].cuda()
        t_k = timed(lambda: moda_amd.kmeans(X, K, init=init, tol=0.0, iter_limit=ITERS), a.reps)
        t_b = timed(lambda: torch_kmeans(X, init, ITERS), max(3, a.reps // 2), warm=1)
        rk = moda_amd.kmeans(X, K, init=init, tol=0.0, iter_limit=ITERS)
        cb, sb = torch_kmeans(X, init, ITERS)
        res["kmeans"][str(N)] = dict(moda_kmeans_ms=t_k, torch_loop_ms=t_b, ratio_torch_over_moda=t_b / t_k, iterations=rk.iterations,
                                     assignment_agreement=float((rk[0] == cb).float().mean()),
                                     max_centre_difference=float((rk[1] - sb).abs().max()))
    for F in SAMPLER_F:
        g = torch.Generator().manual_seed(F)
        verts = (torch.rand((50000, 3), generator=g) * 2 - 1).cuda()
        faces = torch.randint(0, 50000, (F, 3), generator=g, dtype=torch.int32).cuda()
        faces64 = faces.long()
        u = torch.rand((S, 3), generator=g).cuda()
        t_k = timed(lambda: moda_amd.sample_points_from_meshes(verts, faces, u=u), a.reps)
        t_b = timed(lambda: torch_sample(verts, faces64, u), a.reps)
        res["sampler"][str(F)] = dict(moda_sample_ms=t_k, torch_multinomial_ms=t_b, ratio_torch_over_moda=t_b / t_k, samples=S)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh", "kmeans_bench.json"))
    a = ap.parse_args()
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
        print(k, json.dumps({**{f"kmeans {n}": [round(r["moda_kmeans_ms"], 3), round(r["torch_loop_ms"], 3)]
                                for n, r in runs[-1]["kmeans"].items()},
                             **{f"sampler {f}": [round(r["moda_sample_ms"], 3), round(r["torch_multinomial_ms"], 3)]
                                for f, r in runs[-1]["sampler"].items()}}), flush=True)
    ratios = {f"{part} {size}": [r[part][size]["ratio_torch_over_moda"] for r in runs]
              for part in ("kmeans", "sampler") for size in runs[0][part]}
    worst = min(min(v) for v in ratios.values())
    res = dict(device=runs[0]["device"], reps=a.reps, procs=a.procs, runs=runs,
               gate=dict(condition="the moda_amd call takes no longer than the torch baseline at every size in every process",
                         ratios_torch_over_moda=ratios, min_ratio=worst, ok=worst >= 1.0))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res["gate"]))
    if not res["gate"]["ok"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
