"""Mesh sequence warp timing (moda_amd/animate.py, csrc/animate_kernels.hip): warp_fw_frames -- one skin-MLP pass, one pose-head
pass and one moda_dqs_frames launch for all F frames, vertices and result on the device -- against the route the package offered
before it: a loop of F mesh_queries.warp_fw calls over the same vertices, each of which takes numpy in, uploads the vertices,
re-evaluates the skin MLP and the skinning softmax, and returns numpy.
Cases: F in {20, 300}; V = the vertices of a 64^3 and of a 256^3 marching-cubes extraction of the bench mock model's coarse
network at its median density (the largest part is NOT taken: the count is what matters here); B = 25; the library's default
precision.  Each of --procs fresh processes, one after the other: warm-up, then the median of synchronised calls per side
(--reps; the 256^3 cases take --reps-big).  Kernel launches are counted with torch's profiler on one warp_fw_frames call and on ONE
warp_fw call (the loop issues F times that).  No gate: the figures are recorded, whichever way they fall.

  python tools/animate_bench.py [--procs 3] [--reps 5] [--reps-big 2] [--grids 64,256] [--out profiles/animate/animate_bench.json]"""
import argparse
import json
import os
import subprocess
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

BONES, FRAMES, N_FRAMES = 25, (20, 300), 300


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), ts


def count_launches(fn):
    from torch.profiler import profile, ProfilerActivity
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return int(sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA))
    except Exception as e:                        # a profiler that cannot attach is reported, not hidden
        return f"not counted ({type(e).__name__})"


def make_model():
    from moda_amd import feeders as FD
    from moda_amd.bench_support import make_models, DEV
    models, emb = make_models(13, BONES, with_skin=True, with_vis=True)
    model = types.SimpleNamespace(device=DEV, embedding_xyz=emb["xyz"], nerf_coarse=models["coarse"], bones=models["bones_rst"],
                                  rest_pose_code=models["rest_pose_code"], nerf_skin=models["nerf_skin"], skin_aux=models["skin_aux"])
    model.pose_code = FD.FrameCode(6, 128, np.asarray([0, N_FRAMES])).to(DEV)
    head = FD.DQ_RTHead(use_quat=True, in_channels_xyz=128, in_channels_dir=0, out_channels=7 * BONES, raw_feat=True).to(DEV).eval()
    with torch.no_grad():
        head.rgb[0].weight.mul_(0.05)
        head.rgb[0].bias.copy_(torch.tensor([0, 0, 0, 1, 0, 0, 0.0], device=DEV).repeat(BONES))
    model.nerf_body_rts = torch.nn.Sequential(model.pose_code, head)
    opts = types.SimpleNamespace(flowbw=False, lbs=False, neudbs=True, nerf_skin=True, nerf_dis=False, num_bones=BONES)
    return model, opts


def extract(model, grid):
    from moda_amd import mesh as M, mesh_queries as MQ
    bound = np.asarray([0.2, 0.2, 0.2], np.float32)
    vol, _ = MQ.query_volume(model.nerf_coarse, model.embedding_xyz, bound, grid)
    b = np.asarray(bound, np.float64)
    verts, faces, _ = M._run_mc(vol, float(vol.float().median()), scale=2.0 * b / grid, shift=-b)
    return verts.contiguous()


def child(a):
    import moda_amd
    from moda_amd import animate as AM, mesh_queries as MQ
    model, opts = make_model()
    cases = []
    for grid in a.grid_list:
        verts = extract(model, grid)
        host = verts.cpu().numpy()
        V = int(verts.shape[0])
        reps = a.reps if grid < 256 else a.reps_big
        per_call = count_launches(lambda: MQ.warp_fw(opts, model, {}, host, 3))
        for F in FRAMES:
            ids = list(range(F))
            batched = lambda: AM.warp_fw_frames(opts, model, verts, ids)

            def loop():
                return [MQ.warp_fw(opts, model, {}, host, i)[0] for i in ids]
            t_b, all_b = timed(batched, reps)
            t_l, all_l = timed(loop, reps)
            got = batched()[0]
            ref = loop()
            diff = max(float(np.abs(got[i].cpu().numpy() - ref[i]).max()) for i in (0, F // 2, F - 1))
            cases.append(dict(grid=grid, V=V, F=F, reps=reps, batched_ms=t_b, loop_ms=t_l, ratio_loop_over_batched=t_l / t_b,
                              batched_all_ms=all_b, loop_all_ms=all_l, output_bytes=F * V * 12,
                              launches=dict(batched=count_launches(batched), loop_one_call=per_call,
                                            loop=(per_call * F if isinstance(per_call, int) else per_call)),
                              max_abs_difference_between_routes=diff))
            del got, ref
            torch.cuda.empty_cache()
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), precision=moda_amd.get_precision(), bones=BONES, cases=cases,
                          note="the loop returns numpy per frame (its contract) and the batched route leaves (F, V, 3) on the "
                               "device; no read-back of the batched result is included")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reps-big", type=int, default=2)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--grids", default="64,256")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "animate", "animate_bench.json"))
    a = ap.parse_args()
    a.grid_list = [int(g) for g in a.grids.split(",")]
    if a.child:
        child(a)
        return
    runs = []
    for k in range(a.procs):                          # one fresh process per run, one after the other; stop at the first failure
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--reps-big", str(a.reps_big),
                            "--grids", a.grids], capture_output=True, text=True, timeout=400)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"run {k} failed with {p.returncode}")
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
        for c in runs[-1]["cases"]:
            print(k, json.dumps({n: (round(c[n], 3) if isinstance(c[n], float) else c[n]) for n in ("grid", "V", "F", "batched_ms", "loop_ms")}),
                  flush=True)
    summary = []
    for i, c in enumerate(runs[0]["cases"]):
        b, l = [r["cases"][i]["batched_ms"] for r in runs], [r["cases"][i]["loop_ms"] for r in runs]
        summary.append(dict(grid=c["grid"], V=c["V"], F=c["F"], batched_ms=[min(b), max(b)], loop_ms=[min(l), max(l)],
                            ratio_loop_over_batched=[min(x / y for x, y in zip(l, b)), max(x / y for x, y in zip(l, b))],
                            launches=c["launches"]))
    res = dict(device=runs[0]["device"], precision=runs[0]["precision"], procs=a.procs, summary=summary, runs=runs)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
