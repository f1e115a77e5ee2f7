"""Novel-view frame rendering timing (moda_amd/nvs.py, csrc/nvs_kernels.hip): render_nvs on 8 frames of 256 x 256 with disc masks
of about 40 % of the pixels, the 8 x 256 coarse network with 25 bones, the skin and the visibility networks, ndepth 64, chunk
32768, in the library's default precision -- against the reference's route (scripts/visualize/nvs.py:109-174) restated in torch
around the SAME render_rays: a per-frame loop with boolean indexing of the pixel grid, raycast, the codes repeated over the
frame's rays, the chunk loop, .cpu() of the four results, thresholding and canvas assembly in numpy.
Each of --procs fresh processes, one after the other: warm-up, then the median of --reps synchronised calls per side.
Gate, a condition and not a tuned figure: in EVERY process the device route takes no longer than the restated route.
Also recorded: the two ends alone (ray list + rays + code rows + assembly on stored per-ray results, against the restated route's
indexing, repeats, four .cpu() and numpy assembly), kernel launches per call counted with torch's profiler, the share of the
call that is not render_rays, and whether the two routes' canvases agree.

  python tools/nvs_bench.py [--procs 3] [--reps 10] [--out profiles/nvs/nvs_bench.json]"""
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

B, S, NDEPTH, CHUNK, BONES = 8, 256, 64, 32768, 25


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


def count_launches(fn):
    from torch.profiler import profile, ProfilerActivity
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return int(sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA))
    except Exception as e:                        # a profiler that cannot attach is reported, not hidden
        return f"not counted ({type(e).__name__})"


def make_scene():
    from moda_amd import synth, feeders as FD
    from moda_amd.bench_support import make_models, make_opts, DEV
    models, emb = make_models(13, BONES, with_skin=True, with_vis=True)
    model = types.SimpleNamespace(nerf_models=models, embeddings=emb, opts=make_opts(num_bones=BONES, ndepth=NDEPTH, chunk=CHUNK))
    model.pose_code = FD.FrameCode(6, 128, np.asarray([0, 50])).to(DEV)
    model.env_code = FD.FrameCode(6, 64, np.asarray([0, 50])).to(DEV)
    head = FD.DQ_RTHead(use_quat=True, in_channels_xyz=128, in_channels_dir=0, out_channels=7 * BONES, raw_feat=True).to(DEV)
    with torch.no_grad():
        head.rgb[0].weight.mul_(0.05)
        head.rgb[0].bias.copy_(torch.tensor([0, 0, 0, 1, 0, 0, 0.0], device=DEV).repeat(BONES))
    model.nerf_body_rts = torch.nn.Sequential(model.pose_code, head)
    model.rest_pose_code = models["rest_pose_code"]
    model.latest_vars = {"obj_bound": np.asarray([0.2, 0.2, 0.2], np.float32)}
    cam = synth.make_cameras(13, B)
    rtks = np.zeros((B, 4, 4), np.float32)
    rtks[:, :3, :3], rtks[:, :3, 3] = cam["Rmat"], cam["Tmat"]
    rtks[:, 3] = [2.0 * S, 2.0 * S, S / 2, S / 2]
    yy, xx = np.mgrid[:S, :S]
    masks = np.stack([((xx - S / 2 - 3 * b) ** 2 + (yy - S / 2 + 2 * b) ** 2 < (0.357 * S) ** 2) for b in range(B)]).astype(np.float32)
    near_far = torch.tensor([[0.6, 1.4]] * B, device=DEV)
    return model, rtks, masks, torch.arange(B, device=DEV) * 5 + 2, near_far, DEV


def restated_front(model, rtks_t, mask_t, embedid, near_far, i):
    """nvs.py:41-55 and :122-132 for frame i with torch: boolean indexing of the whole pixel grid, raycast, repeated codes."""
    from moda_amd import feeders as FD
    from moda_amd.geom_utils import K2inv
    r = rtks_t[i:i + 1]
    keep = mask_t[i].view(-1) > 0
    _, xys = FD.sample_xy(S, 1, 0, mask_t.device, return_all=True)
    rays = FD.raycast(xys[:, keep], r[:, :3, :3], r[:, :3, 3], K2inv(r[:, 3]), near_far[i:i + 1])
    n = rays["nsample"]
    rays["env_code"] = model.env_code(embedid[i:i + 1])[:, None].repeat(1, n, 1)
    rays["time_embedded"] = model.pose_code(embedid[i:i + 1])[:, None].repeat(1, n, 1)
    rays["bone_rts"] = model.nerf_body_rts(embedid[i:i + 1]).repeat(1, n, 1)
    FD.update_delta_rts(model, rays)
    return rays


def restated_back(masks_np, i, rgb, dph, sil, vis):
    """nvs.py:160-174: four .cpu(), numpy thresholding and `ones` canvases."""
    rgb, dph, sil, vis = rgb.cpu().numpy(), dph.cpu().numpy(), sil.cpu().numpy(), vis.cpu().numpy()
    sil[sil < 0.5] = 0
    rgb[sil < 0.5] = 1
    out = [np.ones((S, S, 3)), np.ones((S, S)), np.ones((S, S)), np.ones((S, S))]
    keep = masks_np[i] > 0
    for canvas, v in zip(out, (rgb, dph, sil, vis)):
        canvas[keep] = v
    return out


def restated_route(model, rtks_t, mask_t, masks_np, embedid, near_far, render=True, stored=None):
    import moda_amd
    from moda_amd import feeders as FD
    frames = []
    with torch.no_grad():
        for i in range(B):
            rays = restated_front(model, rtks_t, mask_t, embedid, near_far, i)
            n = rays["nsample"]
            if render:
                res = {k: [] for k in ("img_coarse", "depth_rnd", "sil_coarse", "vis_pred")}
                for j in range(0, n, CHUNK):
                    out = moda_amd.render_rays(model.nerf_models, model.embeddings, FD.chunk_rays(rays, j, CHUNK), N_samples=NDEPTH,
                                               perturb=0, noise_std=0, chunk=CHUNK, use_fine=True, img_size=S,
                                               obj_bound=model.latest_vars["obj_bound"], render_vis=True, opts=model.opts)
                    for k in res:
                        res[k].append(out[k])
                rgb, dph, sil, vis = (torch.cat(res[k], 0).view(n, -1) for k in res)
            else:
                rgb, dph, sil, vis = (t[stored[1][i]:stored[1][i + 1]] for t in stored[0])
            frames.append(restated_back(masks_np, i, rgb, dph[..., 0], sil[..., 0], vis[..., 0]))
    return frames


def child(a):
    import moda_amd
    from moda_amd import nvs as NV
    model, rtks, masks, embedid, near_far, dev = make_scene()
    mask_t, rtks_t = torch.from_numpy(masks).to(dev), torch.from_numpy(rtks).to(dev)
    device_route = lambda: NV.render_nvs(model, rtks_t, mask_t, embedid, near_far=near_far)
    torch_route = lambda: restated_route(model, rtks_t, mask_t, masks, embedid, near_far)
    t_d, t_t = timed(device_route, a.reps), timed(torch_route, a.reps)
    fr, ref = device_route(), torch_route()
    n = int(fr.offsets[-1])
    g = torch.Generator(device=dev).manual_seed(37)
    stored = [torch.rand((n, c), device=dev, generator=g) for c in (3, 1, 1, 1)]
    off = fr.offsets.tolist()
    _, Rmat, Tmat, Kinv = NV._cameras("bench", rtks_t, dev)

    def device_ends():
        with torch.no_grad():
            lst = NV._compact("bench", mask_t)
            rows = {"time_embedded": model.pose_code(embedid)[:, None], "env_code": model.env_code(embedid)[:, None],
                    "bone_rts": model.nerf_body_rts(embedid)}
            moda_amd.feeders.update_delta_rts(model, rows)
            NV._rays("bench", lst, S, Rmat, Tmat, Kinv, near_far, rows=rows)
            return NV._assemble(lst.rank, n, lst.counts, *stored, False)

    torch_ends = lambda: restated_route(model, rtks_t, mask_t, masks, embedid, near_far, render=False, stored=(stored, off))
    e_d, e_t = timed(device_ends, a.reps), timed(torch_ends, a.reps)
    agree = {k: float(np.abs(np.stack([f[i] for f in ref]) - getattr(fr, k).cpu().numpy().astype(np.float64)).max())
             for i, k in enumerate(("rgb", "depth", "sil", "vis"))}
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, precision=moda_amd.get_precision(),
               shape=dict(frames=B, img_size=S, ndepth=NDEPTH, chunk=CHUNK, bones=BONES, rays=n, mask_share=n / (B * S * S)),
               device_route_ms=t_d, restated_route_ms=t_t, ratio_restated_over_device=t_t / t_d,
               ends_device_ms=e_d, ends_restated_ms=e_t, share_not_render_rays=dict(device=e_d / t_d, restated=e_t / t_t),
               launches=dict(device_route=count_launches(device_route), restated_route=count_launches(torch_route),
                             ends_device=count_launches(device_ends), ends_restated=count_launches(torch_ends)),
               max_abs_difference_between_routes=agree,
               note="the routes call render_rays on different chunks (32768 rays across frames against a frame's rays), so their "
                    "canvases agree to the renderer's chunk invariance in this precision, not by construction")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nvs", "nvs_bench.json"))
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    runs = []
    for k in range(a.procs):                          # one fresh process per run, one after the other; stop at the first failure
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=280)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"run {k} failed with {p.returncode}")
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(k, json.dumps({n: round(runs[-1][n], 3) for n in ("device_route_ms", "restated_route_ms", "ends_device_ms", "ends_restated_ms")}),
              flush=True)
    ratios = [r["ratio_restated_over_device"] for r in runs]
    res = dict(device=runs[0]["device"], reps=a.reps, procs=a.procs, runs=runs,
               gate=dict(condition="render_nvs is no slower than the restated route in every process",
                         ratios_restated_over_device=ratios, min_ratio=min(ratios), ok=min(ratios) >= 1.0))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res["gate"]))
    if not res["gate"]["ok"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
