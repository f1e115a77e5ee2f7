"""Rasteriser timing (moda_amd/mesh_render.py, csrc/raster_kernels.hip) at render_dp's shape: 16 views, 256 x 256, 16 channels,
on an icosphere cut to 13 800 faces (the DensePose surface's size) and on the marching-cubes mesh of the 64^3 sphere SDF that
tests/test_gpu_marching_cubes.py extracts (extract_mesh's own fixture grid, G13, is 6^3: too small to time).
Comparator: the reference kernel cannot run on this GPU and the parent commit has no rasteriser, so the other side is what a
user could write with torch alone -- a brute-force restatement of the reference kernel on the same GPU (a chunk of pixels
against ALL faces, both windings, masked minimum of the depth), run as the reference's render_dp runs it: six 3-channel renders.
Each of --procs fresh processes, one after the other: warm-up, then the median of --reps event-timed calls per side; the
clock the device reports before and after is recorded.  No gate: the figures are findings.

  python tools/raster_bench.py [--procs 3] [--reps 20] [--out profiles/mesh/raster_bench.json]
  python tools/raster_bench.py --once        # one rasterize + interpolate: the program to put after `rocprofv3 ... --`"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

B, S, C = 16, 256, 16


def scenes():
    import moda_amd
    import raster_numpy as rn
    v, f = rn.icosphere(5, 0.9)
    out = {"icosphere_13800": (v, f[:13800])}
    n = 64
    ax = [np.arange(n, dtype=np.float64) - (n - 1) / 2 + o for o in (0.137, 0.071, -0.053)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    vol = (0.35 * n - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32)   # the sphere SDF of tests/test_gpu_marching_cubes.py
    mv, mf = moda_amd.marching_cubes(torch.as_tensor(vol).cuda(), 0.0)
    out["marching_cubes_64"] = ((mv.cpu().numpy().astype(np.float64) - (n - 1) / 2) / (0.5 * n) * 0.8, mf.cpu().numpy())
    res = {}
    for name, (v, f) in out.items():
        vs = np.stack([v @ rn.rotation(s).T + [0, 0, 3.0] for s in range(B)]).astype(np.float32)
        att = np.random.default_rng(1).uniform(0.1, 1, (B, len(v), C)).astype(np.float32)
        res[name] = (torch.as_tensor(vs).cuda(), torch.as_tensor(f, dtype=torch.int32).cuda(), torch.as_tensor(att).cuda())
    return res


def torch_render3(verts, faces, attrs3, chunk=2048, near=1.0, far=100.0):
    """One 3-channel render of every view, brute force: -> (B,4,S,S)."""
    i = torch.arange(S, device=verts.device, dtype=torch.float32)
    xs, ys = (2 * i + 1 - S) / S, (2 * (S - 1 - i) + 1 - S) / S
    X, Y = xs[None, :].expand(S, S).reshape(-1), ys[:, None].expand(S, S).reshape(-1)
    out = torch.zeros((verts.shape[0], 4, S * S), device=verts.device)
    f = faces.long()
    for b in range(verts.shape[0]):
        p = verts[b][f]                                                       # (F,3,3)
        x0, y0, x1, y1, x2, y2 = p[:, 0, 0], p[:, 0, 1], p[:, 1, 0], p[:, 1, 1], p[:, 2, 0], p[:, 2, 1]
        det = x2 * (y0 - y1) + x0 * (y1 - y2) + x1 * (y2 - y0)
        det = torch.where(det > 0, det.clamp(min=1e-10), det.clamp(max=-1e-10))
        A = torch.stack([y1 - y2, y2 - y0, y0 - y1], -1) / det[:, None]
        Bc = torch.stack([x2 - x1, x0 - x2, x1 - x0], -1) / det[:, None]
        Cc = torch.stack([x1 * y2 - x2 * y1, x2 * y0 - x0 * y2, x0 * y1 - x1 * y0], -1) / det[:, None]
        a3 = attrs3[b][f]                                                     # (F,3,3)
        for s in range(0, S * S, chunk):
            w = A[None] * X[s:s + chunk, None, None] + Bc[None] * Y[s:s + chunk, None, None] + Cc[None]      # (P,F,3)
            inside = ((w >= 0) & (w <= 1)).all(-1)
            wc = w.clamp(0, 1)
            wc = wc / wc.sum(-1, keepdim=True).clamp(min=1e-5)
            zp = 1.0 / (wc / p[None, :, :, 2]).sum(-1)
            zp = torch.where(inside & ~((zp < near) | (zp > far)), zp, torch.full_like(zp, float("inf")))
            z, k = zp.min(dim=1)
            col = (wc[torch.arange(len(k)), k][:, :, None] * a3[k]).sum(1)
            out[b, :3, s:s + chunk] = torch.where(torch.isfinite(z)[:, None], col, torch.zeros_like(col)).T
            out[b, 3, s:s + chunk] = inside.any(1).float()
    return out.reshape(-1, 4, S, S)


def torch_render_dp(verts, faces, attrs):
    outs = []
    for i in range(0, C, 3):                                                  # moda.py:986-995
        chunk = attrs[..., i:i + 3]
        if chunk.shape[-1] < 3:
            chunk = torch.cat([chunk, attrs[..., :3 - chunk.shape[-1]]], -1)
        outs.append(torch_render3(verts, faces, chunk)[:, :3])
    return torch.cat(outs, 1)[:, :C]


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def clock():
    """The clock state as the device reports it (a read-only query); a string saying why when it cannot be read."""
    try:
        return {"sclk_mhz": int(torch.cuda.clock_rate())}
    except Exception as e:
        first = f"torch.cuda.clock_rate: {type(e).__name__}"
    try:
        p = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=30)
        return {"rocm_smi_showclocks": json.loads(p.stdout)}
    except Exception as e:
        return {"unavailable": f"{first}; rocm-smi --showclocks: {type(e).__name__}"}


def child(a):
    from moda_amd import mesh_render as R
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, views=B, image_size=S, channels=C, clock_before=clock(), scenes={})
    for name, (v, f, att) in scenes().items():
        def ours():
            fi, bw, _, _ = R.rasterize(v, f, S)
            return R.interpolate(att, f, fi, bw)
        t_all = timed(ours, a.reps, 3)
        t_ras = timed(lambda: R.rasterize(v, f, S), a.reps, 1)
        t_unb = timed(lambda: R.rasterize(v, f, S, binned=False), max(2, a.reps // 5), 1)
        t_ref = timed(lambda: torch_render_dp(v, f, att), a.base_reps, 1)
        img, ref = ours(), torch_render_dp(v, f, att)
        agree = float(((img - ref).abs().amax(1) <= 1e-3).float().mean())
        res["scenes"][name] = dict(faces=int(f.shape[0]), vertices=int(v.shape[1]), rasterize_plus_interpolate_ms=t_all,
                                   rasterize_ms=t_ras, rasterize_unbinned_ms=t_unb, torch_brute_force_6_renders_ms=t_ref,
                                   ratio_torch_over_moda=t_ref / t_all, pixels_agreeing_to_1e_3=agree)
    res["clock_after"] = clock()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--base-reps", type=int, default=2)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh", "raster_bench.json"))
    a = ap.parse_args()
    if a.once:
        from moda_amd import mesh_render as R
        v, f, att = scenes()["icosphere_13800"]
        for _ in range(3):
            fi, bw, _, _ = R.rasterize(v, f, S)
            R.interpolate(att, f, fi, bw)
        torch.cuda.synchronize()
        return
    if a.child:
        child(a)
        return
    runs = []
    for k in range(a.procs):                          # one fresh process per run, one after the other; stop at the first failure
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--base-reps",
                            str(a.base_reps)], capture_output=True, text=True, timeout=420)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"run {k} failed with {p.returncode}")
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(k, json.dumps({s: [round(r["rasterize_plus_interpolate_ms"], 3), round(r["torch_brute_force_6_renders_ms"], 1)]
                             for s, r in runs[-1]["scenes"].items()}), flush=True)
    res = dict(device=runs[0]["device"], reps=a.reps, procs=a.procs, runs=runs,
               ratios_torch_over_moda={s: [r["scenes"][s]["ratio_torch_over_moda"] for r in runs] for s in runs[0]["scenes"]})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res["ratios_torch_over_moda"]))


if __name__ == "__main__":
    main()
