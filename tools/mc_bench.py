"""Mesh-extraction timing (moda_amd/mesh.py) on the G13 mock model's lattice queries: query_volume (the parent commit's path),
marching_cubes, largest_part and extract_mesh end to end, at 64^3, 128^3 and 256^3 in the library's default precision, in one
process: warm-up, then the median of --reps runs each (wall clock around a synchronised call; the mesh calls read their
counts back, so they synchronise anyway).  Gate: at 256^3, marching_cubes + largest_part <= 0.10 x query_volume, in EVERY
one of --procs separate processes (each a fresh interpreter and model); all runs are reported.  The CPU float64 oracle
(tests/mc_numpy.py) is timed once per size and process as context.

  python tools/mc_bench.py [--procs 5] [--reps 20] [--out profiles/mesh/mc_bench.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def timed(fn, reps, warm=3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--procs", type=int, default=5)
    ap.add_argument("--grids", default="64,128,256")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh", "mc_bench.json"))
    a = ap.parse_args()
    if not a.child:
        runs = []
        for k in range(a.procs):                      # one fresh process per run, one after the other
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--grids", a.grids],
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"run {k} failed with {p.returncode}")
            runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(k, json.dumps({g: round(r["ratio_mc_cc_over_query"], 4) for g, r in runs[-1]["grids"].items()}), flush=True)
        res = dict(device=runs[0]["device"], precision=runs[0]["precision"], reps=a.reps, procs=a.procs, runs=runs)
        if "256" in runs[0]["grids"]:
            ratios = [r["grids"]["256"]["ratio_mc_cc_over_query"] for r in runs]
            res["gate_256"] = dict(ratios=ratios, max_ratio=max(ratios), limit=0.10, ok=max(ratios) <= 0.10)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
        print(json.dumps(res.get("gate_256")))
        return
    import types
    import moda_amd
    from moda_amd import mesh as M, mesh_queries as MQ
    from test_gpu_mesh_queries import build_model
    import mc_numpy as mcn

    model, models, emb = build_model()
    bound = np.asarray([0.2, 0.15, 0.25], np.float32)
    res = dict(device=torch.cuda.get_device_name(0), precision=moda_amd.get_precision(), reps=a.reps, grids={})
    for g in (int(x) for x in a.grids.split(",")):
        vol, vis = MQ.query_volume(models["coarse"], emb["xyz"], bound, g, nerf_vis=models["nerf_vis"])
        thr = float(torch.quantile(vol.reshape(-1)[::max(1, vol.numel() // 1000000)].float(), 0.5))   # a half-full lattice
        t_q = timed(lambda: MQ.query_volume(models["coarse"], emb["xyz"], bound, g), a.reps)
        t_mc = timed(lambda: M.marching_cubes(vol, thr), a.reps)
        v, f = M.marching_cubes(vol, thr)
        mesh = M.TriMesh(v, f)
        t_cc = timed(lambda: M.largest_part(mesh), a.reps)
        part = M.largest_part(mesh)
        import tempfile
        logdir = tempfile.mkdtemp()
        os.makedirs(os.path.join(logdir, "mc_bench"), exist_ok=True)
        model.opts = types.SimpleNamespace(queryfw=False, symm_shape=False, full_mesh=True, nerf_vis=True, use_cc=True,
                                           ce_color=True, checkpoint_dir=logdir, logname="mc_bench")
        model.nerf_coarse, model.nerf_vis, model.near_far = models["coarse"], models["nerf_vis"], torch.zeros(1)
        model.latest_vars = {"obj_bound": bound, "idk": np.zeros(1)}
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            t_ex = timed(lambda: M.extract_mesh(model, 0, g, threshold=thr), max(5, a.reps // 2), warm=1)
        vn = vol.cpu().numpy()
        t0 = time.perf_counter()
        mcn.marching_cubes(vn, thr)
        t_cpu = (time.perf_counter() - t0) * 1e3
        row = dict(query_volume_ms=t_q, marching_cubes_ms=t_mc, largest_part_ms=t_cc, extract_mesh_ms=t_ex,
                   mc_numpy_cpu_ms=t_cpu, vertices=int(v.shape[0]), faces=int(f.shape[0]), kept_vertices=int(part.vertices_t.shape[0]),
                   ratio_mc_cc_over_query=(t_mc + t_cc) / t_q)
        res["grids"][str(g)] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
