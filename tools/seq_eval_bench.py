"""Whole-sequence mesh evaluation timing (moda_amd/mesh_eval.py: eval_sequence against the loop of eval_mesh calls it replaces).
F in {20, 300} frames of a mesh the size a 64^3 extraction gives (V = 9000 vertices of the bumpy ellipsoid of the ICP tests, at
depth 1), each frame moved by its own small rigid motion, against per-frame ground truth of differing sizes (8000 to 10000
vertices of the same surface).  The two sides: the loop (`eval_mesh(verts[f], gts[f])` for every frame, which is also what the
commit before eval_sequence offers) and `eval_sequence(verts, gts).summary()`.  Each of --procs fresh processes, one after the
other, per size: one untimed run of each side on the very scene that is timed (so every shape, plan and allocation is warm),
then --reps rounds, each a synchronised wall-clock run of both sides in alternating order (loop first in even rounds, sequence
first in odd ones); the median per side and the range over the rounds are kept, and the per-frame figures of the two sides are
compared.  No gate: the figures are recorded, min and max of the medians over the processes.

  python tools/seq_eval_bench.py [--procs 3] [--reps 4] [--frames 20 300] [--out profiles/mesh/seq_eval_bench.json]"""
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

V = 9000


def surface(n, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.randn((n, 3), generator=g, dtype=torch.float64)
    u = u / u.norm(dim=1, keepdim=True)
    p = u * torch.tensor([0.30, 0.18, 0.11], dtype=torch.float64) * (1 + 0.25 * torch.sin(5 * u[:, :1]) * torch.cos(3 * u[:, 1:2]))
    return p + torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(degrees)
    return torch.as_tensor(np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K)


def scene(F):
    rng = np.random.default_rng(F)
    base = surface(V, 1)
    centre = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
    verts, gts = [], []
    for f in range(F):
        R = rotation(rng.standard_normal(3), rng.uniform(2.0, 8.0))
        verts.append((base - centre) @ R + centre + torch.as_tensor(rng.uniform(-0.01, 0.01, 3)))
        gts.append(surface(int(rng.integers(8000, 10001)), 100 + f).float().cuda())
    return torch.stack(verts).float().cuda().contiguous(), gts


def worker(frames, reps):
    import moda_amd
    out = {"device": torch.cuda.get_device_name(0)}

    def run_loop(verts, gts):
        res = [moda_amd.eval_mesh(verts[f], gts[f]) for f in range(len(gts))]
        torch.cuda.synchronize()
        return res

    def run_seq(verts, gts):
        seq = moda_amd.eval_sequence(verts, gts)
        summ = seq.summary()
        torch.cuda.synchronize()
        return seq, summ

    def clock(fn, *a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn(*a)
        return (time.perf_counter() - t0) * 1e3, r

    for F in frames:
        verts, gts = scene(F)
        loop, (seq, summ) = run_loop(verts, gts), run_seq(verts, gts)         # untimed: the timed shapes, warm
        t_loop, t_seq = [], []
        for r in range(reps):
            for side in (("loop", "seq") if r % 2 == 0 else ("seq", "loop")):
                if side == "loop":
                    t, loop = clock(run_loop, verts, gts)
                    t_loop.append(t)
                else:
                    t, (seq, summ) = clock(run_seq, verts, gts)
                    t_seq.append(t)
        cd = seq.cd.cpu().numpy()
        it_loop, it_seq = [len(e["icp"].t_history) for e in loop], seq.iterations.tolist()
        out[str(F)] = dict(loop_ms=float(np.median(t_loop)), sequence_ms=float(np.median(t_seq)),
                           ratio=float(np.median(t_loop) / np.median(t_seq)),
                           loop_ms_range=[min(t_loop), max(t_loop)], sequence_ms_range=[min(t_seq), max(t_seq)],
                           iterations_equal=it_loop == it_seq, iterations_min=min(it_seq), iterations_max=max(it_seq),
                           max_rel_cd_difference=float(max(abs(cd[f] - loop[f]["cd"]) / loop[f]["cd"] for f in range(F))),
                           max_f002_difference=float(max(abs(float(seq.f002[f]) - loop[f]["f002"]) for f in range(F))),
                           summary=summ)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--frames", type=int, nargs="+", default=[20, 300])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh", "seq_eval_bench.json"))
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.frames, a.reps)
    runs = []
    for _ in range(a.procs):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(a.reps), "--frames"]
                           + [str(f) for f in a.frames],
                           capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit(f"worker failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        runs.append(json.loads(line[-1][7:]))
    res = {"device": runs[0]["device"], "procs": a.procs, "reps": a.reps, "V": V, "runs": runs}
    for F in a.frames:
        k = str(F)
        res[k] = {m: [min(r[k][m] for r in runs), max(r[k][m] for r in runs)] for m in ("loop_ms", "sequence_ms", "ratio")}
        print(f"F = {F}: eval_mesh loop {res[k]['loop_ms'][0]:.1f}-{res[k]['loop_ms'][1]:.1f} ms, eval_sequence "
              f"{res[k]['sequence_ms'][0]:.1f}-{res[k]['sequence_ms'][1]:.1f} ms, ratio {res[k]['ratio'][0]:.2f}-{res[k]['ratio'][1]:.2f}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
