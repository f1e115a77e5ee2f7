"""Mesh sequence rendering (moda_amd/seq_render.py) against the loop it replaces: mesh_render.render_mesh per frame plus the overlay
and the resize as torch ops, with the host wait render_mesh takes in each frame.

Workload: F in {20, 300} frames of an icosphere of about the size a 64^3 extraction gives (subdivision 4: 2562 vertices, 5120
faces), (H, W) = (1080, 1920), modes `vp 0` and `vp -1 --vis_bones` (25 ellipsoids).  Method: `--procs` processes, each reporting
the median of `--reps` synchronised calls after one warm-up call; no gate.  Launch counts come from a trace run of its own, not
from this script.  One JSON line; --out writes it to a file."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def median_ms(fn, reps, torch):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def make_sequence(F, H, W, torch, moda_amd):
    import seqvis_numpy as sn
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    v, f = sn.icosphere(4)
    verts = np.stack([v * (0.8 + 0.1 * np.sin(0.1 * i)) for i in range(F)]).astype(np.float32)
    colors = rng.integers(0, 256, (len(v), 3)).astype(np.uint8)
    rtk = np.stack([sn.camera(sn.rodrigues([0, 0.02 * i, 0]), (0, 0, 3.0), (900.0, 900.0, W / 2, H / 2)) for i in range(F)])
    b = np.zeros((F, 25, 10), np.float32)
    b[:, :, 3] = 1.0
    b[:, :, :3] = rng.uniform(-0.6, 0.6, (1, 25, 3))
    t = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    bones = t(b)
    return moda_amd.MeshSequence(t(verts), t(f, torch.int32), t(colors), bones, moda_amd.bone_ellipsoids(bones, 2.0), None, t(rtk),
                                 t(verts[0]), t(colors), moda_amd.bone_ellipsoids(bones[:1], 2.0))


def loop_route(seq, H, W, overlay, out_width, torch, moda_amd):
    """What a user of the parent commit writes: render_mesh per frame at S = max(H, W), crop, overlay, resize."""
    import torch.nn.functional as Fn
    S, h = max(H, W), int(H * out_width / W)
    frames = []
    for i in range(len(seq)):
        color, depth, sil = moda_amd.render_mesh(seq.frame(i), seq.rtk[i], S)
        color = color[:H, :W]
        color = ((color.float() + overlay[i].float()) * 0.5).round().clamp(0, 255)
        frames.append(Fn.interpolate(color.permute(2, 0, 1)[None], size=(h, out_width), mode="bilinear", align_corners=False)
                      .round().clamp(0, 255).to(torch.uint8)[0].permute(1, 2, 0))
    return torch.stack(frames)


def one_process(reps, sizes):
    import torch
    import moda_amd
    H, W, ow = 1080, 1920, 480
    res = {}
    for F in sizes:
        seq = make_sequence(F, H, W, torch, moda_amd)
        overlay = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device="cuda")
        res[f"F{F}_vp0_ms"] = median_ms(lambda: seq.render((H, W), vp=0, overlay=overlay, out_width=ow), reps, torch)
        res[f"F{F}_bones_ms"] = median_ms(lambda: seq.render((H, W), vp=-1, bones=True, mesh_opacity=0.5, overlay=overlay, out_width=ow),
                                          reps, torch)
        res[f"F{F}_loop_vp0_ms"] = median_ms(lambda: loop_route(seq, H, W, overlay, ow, torch, moda_amd), reps, torch)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="+", default=[20, 300])
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print("SEQ_RENDER_BENCH " + json.dumps(one_process(args.reps, args.frames)), flush=True)
        return
    runs = []
    for _ in range(args.procs):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--frames"]
                             + [str(f) for f in args.frames], capture_output=True, text=True, check=True).stdout
        runs.append(json.loads(next(line for line in out.splitlines() if line.startswith("SEQ_RENDER_BENCH "))[len("SEQ_RENDER_BENCH "):]))
    result = {"bench": "seq_render", "procs": args.procs, "reps": args.reps, "runs": runs,
              "range": {k: [min(r[k] for r in runs), max(r[k] for r in runs)] for k in runs[0]}}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
