"""Camera tools (moda_amd/cams.py) against the reference's route restated in torch on the GPU.

  hull   visual_hull_align at V = 100 views of 512 x 512, G = 64, against the reference's loop over chunks of 1000 lattice points
         with F.grid_sample (geom_utils.py:1583-1608) on device tensors.
  cams   save_cams + align_sim3 at N = 1000 frames in 10 videos against the numpy / scipy route with its host round trips: the
         per-frame loop of save_cams on arrays copied from the device, Rotation.from_matrix(...).mean() (scipy, when it is
         installed; otherwise that leg is left out and said so), the table copied back.

Every process takes the median of --reps synchronised calls after a warm-up; --procs 3 runs three processes one after the other
and reports the range of their medians.  One JSON line; --out writes it to a file as well.  Nothing is gated.

    python tools/cams_bench.py --procs 3 --reps 10 --out profiles/cams/cams_bench.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps, torch):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def rotations(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.linalg.det(q)[:, None]
    return q


def hull_scene(rng, V, S):
    rtk = np.tile(np.eye(4), (V, 1, 1))
    rtk[:, :3, :3] = rotations(rng, V)
    rtk[:, 2, 3] = 3.0 + rng.uniform(-0.2, 0.2, V)
    rtk[:, 3] = [1.2 * S, 1.2 * S, S / 2.0, S / 2.0]
    pc = rtk[:, :3, :3] @ np.asarray([0.2, -0.1, 0.15]) + rtk[:, :3, 3]
    u, v, rad = 1.2 * S * pc[:, 0] / pc[:, 2] + S / 2.0, 1.2 * S * pc[:, 1] / pc[:, 2] + S / 2.0, 1.2 * S * 0.35 / pc[:, 2]
    yy, xx = np.mgrid[:S, :S] + 0.5
    masks = ((xx[None] - u[:, None, None]) ** 2 + (yy[None] - v[:, None, None]) ** 2 <= rad[:, None, None] ** 2)
    return rtk.astype(np.float32), np.tile(np.asarray([1, 1, 0, 0], np.float32), (V, 1)), masks.astype(np.float32)


def hull_torch(rtk, kaug, masks, G, torch):
    """visual_hull_align as the reference writes it, on device tensors."""
    import torch.nn.functional as F
    from moda_amd.geom_utils import K2inv, K2mat, mat2K, obj_to_cam, pinhole_cam
    V, h, w = masks.shape
    rmat, tmat = rtk[:, :3, :3], rtk[:, :3, 3:]
    kmat = mat2K(K2inv(kaug).matmul(K2mat(rtk[:, 3])))
    rmatc = rmat.permute(0, 2, 1)
    tmatc = -rmatc.matmul(tmat)
    bound = tmatc.norm(2, -1).mean()
    pts = torch.linspace(-1, 1, G, device=rtk.device) * bound
    q = torch.stack(torch.meshgrid(pts, pts, pts, indexing="ij"), -1).view(-1, 3)
    scores = []
    for i in range(0, len(q), 1000):
        c = q[None, i:i + 1000].repeat(V, 1, 1)
        c = pinhole_cam(obj_to_cam(c, rmat, tmat[..., 0]), kmat)
        xy = torch.stack([c[..., 0] / w * 2 - 1, c[..., 1] / h * 2 - 1], -1)
        scores.append(F.grid_sample(masks[:, None], xy[:, None], align_corners=False)[:, 0, 0].sum(0))
    centre = q[torch.cat(scores) > 0.8 * V].mean(0)
    out = rtk.clone()
    out[:, :3, 3:] = (-rmat).matmul(tmatc - centre[None, :, None])
    return out


def cams_host(rtk, valid, off, data_offset, scale, state, b, torch, Rotation):
    """save_cams' loop and align_sim3 on the host, with the copies the reference's route makes."""
    r, ok = rtk.cpu().numpy(), valid.cpu().numpy()
    tab_rtk, tab_raw = state.rtk.cpu().numpy(), state.rt_raw.cpu().numpy()
    row = 0
    for v in range(len(off) - 1):
        ids = np.where(ok[off[v]:off[v + 1]])[0] + off[v]
        for i in range(off[v], off[v + 1]):
            if len(ids) and not ok[i]:
                r[i, :3, :3] = r[ids[np.abs(i - ids).argmin()], :3, :3]
            r[i, :3, 3] *= scale
            for _ in range(2 if i == off[v + 1] - 1 else 1):
                tab_raw[row], tab_rtk[row, :3, :3] = r[i, :3, :4], r[i, :3, :3]
                row += 1
    state.rtk.copy_(torch.from_numpy(tab_rtk))
    state.rt_raw.copy_(torch.from_numpy(tab_raw))
    if Rotation is None:
        return
    a, bb = r.astype(np.float64), b.cpu().numpy().astype(np.float64)
    dso3 = np.matmul(bb[:, :3, :3].transpose(0, 2, 1), a[:, :3, :3])
    dscale = np.linalg.norm(a[:, :3, 3], 2, -1) / np.linalg.norm(bb[:, :3, 3], 2, -1)
    bb[:, :3, :3] = np.matmul(bb[:, :3, :3], Rotation.from_matrix(dso3).mean().as_matrix()[None])
    bb[:, :3, 3] *= dscale.mean()
    m = np.matmul(a[:, :3, :3], bb[:, :3, :3].transpose(0, 2, 1))
    err = np.arccos(np.clip((np.trace(m, axis1=1, axis2=2) - 1) / 2, -1 + 1e-4, 1 - 1e-4)) / np.pi * 180
    return err.max(), np.median(err), err.mean(), err.std(ddof=1)


def one_process(reps):
    import importlib

    import torch
    import moda_amd
    CM = importlib.import_module("moda_amd.cams")
    try:
        from scipy.spatial.transform import Rotation
    except ImportError:
        Rotation = None
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    rtk, kaug, masks = (torch.from_numpy(x).to(dev) for x in hull_scene(rng, 100, 512))
    res = {"hull_ms": median_ms(lambda: CM.visual_hull_align(rtk, kaug, masks), reps, torch),
           "hull_torch_ms": median_ms(lambda: hull_torch(rtk, kaug, masks, 64, torch), reps, torch)}
    ours, ref = CM.visual_hull_align(rtk, kaug, masks)[0], hull_torch(rtk, kaug, masks, 64, torch)
    res["hull_translation_diff"] = float((ours[:, :3, 3] - ref[:, :3, 3]).abs().max())
    N, nv = 1000, 10
    off = [v * (N // nv) for v in range(nv + 1)]
    data_offset = [o + v for v, o in enumerate(off)]
    cam = np.tile(np.eye(4), (N, 1, 1))
    cam[:, :3, :3], cam[:, :3, 3] = rotations(rng, N), rng.standard_normal((N, 3)) + [0, 0, 3]
    a = torch.from_numpy(cam.astype(np.float32)).to(dev)
    cam[:, :3, 3] *= 0.4
    b = torch.from_numpy(cam.astype(np.float32)).to(dev)
    valid = torch.from_numpy(rng.uniform(size=N) < 0.7).to(dev)
    state = moda_amd.FrameState(data_offset[-1], dev)

    def device_route():
        init = CM.save_cams(a, valid, data_offset, 0.5, state)
        return CM.align_sim3(init.rtk, b)

    res["cams_ms"] = median_ms(device_route, reps, torch)
    res["cams_host_ms"] = median_ms(lambda: cams_host(a, valid, off, data_offset, 0.5, state, b, torch, Rotation), reps, torch)
    res["scipy"] = Rotation is not None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print("CAMS_BENCH " + json.dumps(one_process(args.reps)), flush=True)
        return
    runs = []
    for _ in range(args.procs):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)], capture_output=True,
                             text=True, check=True).stdout
        runs.append(json.loads(next(line for line in out.splitlines() if line.startswith("CAMS_BENCH "))[len("CAMS_BENCH "):]))
    result = {"bench": "cams", "procs": args.procs, "reps": args.reps, "runs": runs,
              "range": {k: [min(r[k] for r in runs), max(r[k] for r in runs)] for k in runs[0] if k.endswith("_ms")}}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
