"""Pixel-sampling timing (moda_amd/pixel_sampling.py, csrc/pixsample_kernels.hip) at the recipe's shape -- P = 256 line pairs
(512 lines of W = 512 pixels), use_embed, nsample 4 and 6, active sampling on and off -- against the reference's route restated in
torch on the same GPU: nerf_unc on all 2P lines, torch.topk, the Python stack / cat loops of moda.py:1075-1191,
pixel_lines.obs_to_rays_line (which forms t[batch_map]), ending in the two .cpu() calls.  Both sides share the injected draws, the
model, raycast / update_rays / update_delta_rts and run under no_grad.

Per case: median ms of the new route called eagerly and replayed from a captured graph, median ms of the baseline, and the number
of device kernels a call launches (torch.profiler; null where the profiler is unavailable).  Each of --procs fresh processes, one
after the other.  Gate, a condition and not a tuned figure: in EVERY case, in EVERY process, the eager new route takes no longer
than the baseline.

  python tools/sample_pxs_bench.py [--procs 3] [--reps 20] [--out profiles/pxs/sample_pxs_bench.json]"""
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

P, W, BONES, N_FRAMES = 256, 512, 25, 64
CASES = [(4, True), (4, False), (6, True), (6, False)]          # (nsample, active)


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


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return int(sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA")))
    except Exception:
        return None


def make_model(active):
    import moda_amd
    from moda_amd import feeders as FD, synth
    from moda_amd.bench_support import DEV, T, make_models
    models, emb = make_models(5, BONES, with_skin=True)
    unc = moda_amd.NeRFUnc(in_channels_xyz=63, D=8, W=256, out_channels=1, in_channels_dir=32, raw_feat=True, init_beta=1.)
    unc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.nerf_params(
        5, "nerf_unc", D=8, W=256, in_channels_xyz=63, in_channels_dir=32, out_channels=1, init_beta=1.0).items()})
    models["nerf_unc"] = unc.to(DEV).eval()
    m = types.SimpleNamespace(device=DEV, training=True, progress=0.5 if active else 0.0, img_size=W, max_ts=float(N_FRAMES))
    m.opts = types.SimpleNamespace(lineload=True, use_unc=True, nactive=0.5, warmup_steps=0.2, use_embed=True, flowbw=False, lbs=False,
                                   neudbs=True, num_bones=BONES)
    off = np.asarray([0, N_FRAMES])
    m.pose_code = FD.FrameCodeTable(N_FRAMES, 6, 128, off).to(DEV)
    m.env_code = FD.FrameCodeTable(N_FRAMES, 6, 64, off).to(DEV)
    head = FD.DQ_RTHead(use_quat=True, in_channels_xyz=128, in_channels_dir=0, out_channels=7 * BONES, raw_feat=True).to(DEV).eval()
    m.nerf_body_rts = torch.nn.Sequential(m.pose_code, head)
    m.rest_pose_code = models["rest_pose_code"]
    m.vid_code = torch.nn.Embedding(2, 32).to(DEV)
    m.embedding_xyz = emb["xyz"]
    m.nerf_models = models
    m.near_far = T(np.stack([np.full(N_FRAMES, 0.6, np.float32), np.full(N_FRAMES, 1.4, np.float32)], 1))
    return m


def reference_route(m, bs, nsample, Rmat, Tmat, Kinv, dataid, frameid, frameid_sub, lineid, errid, obs, rand_inds_all, active):
    """moda.py:1048-1213 with lineload in training, statement by statement, in torch (the MLP, raycast and update_rays are the
    package's own on both sides)."""
    from moda_amd import feeders as FD, pixel_lines as PL, pixel_sampling as PS
    nsample_a = 4 * nsample
    xys_all = torch.stack([rand_inds_all.float(), lineid[:, None].float().expand(-1, rand_inds_all.shape[1])], -1)
    if active:
        nsample_s = int(m.opts.nactive * nsample)
        nsample = int(nsample * (1 - m.opts.nactive))
    rand_inds_a, xys_a = rand_inds_all[:, -nsample_a:].clone(), xys_all[:, -nsample_a:].clone()
    rand_inds, xys = rand_inds_all[:, :nsample].clone(), xys_all[:, :nsample].clone()
    rep = lambda t, n: t[:, None].repeat(*((1, n) + (1,) * (t.dim() - 1)))
    per = dict(frameid=frameid, frameid_sub=frameid_sub, dataid=dataid, errid=errid, Rmat=Rmat, Tmat=Tmat, Kinv=Kinv,
               batch_map=torch.Tensor(range(bs)).to(Rmat.device).long())
    a = {k: rep(v, nsample_a) for k, v in per.items()}
    u = {k: rep(v, nsample) for k, v in per.items()}
    if active:
        unc_pred = PS._predict_unc(m, dataid, frameid_sub, xys_a, Kinv)                    # all 2P lines, as the reference
        unc_pred = unc_pred.view(2, -1)
        two = lambda t: t.view((2, -1) + tuple(t.shape[2:]))
        xys, xys_a, rand_inds, rand_inds_a = two(xys), two(xys_a), two(rand_inds), two(rand_inds_a)
        a = {k: two(v) for k, v in a.items()}
        u = {k: two(v) for k, v in u.items()}
        topk_samp = unc_pred.topk(nsample_s * bs // 2, dim=-1)[1]
        pick = lambda t: torch.stack([t[i][topk_samp[0]] for i in range(2)], 0)
        xys, rand_inds = torch.cat([xys, pick(xys_a)], 1), torch.cat([rand_inds, pick(rand_inds_a)], 1)
        u = {k: torch.cat([u[k], pick(a[k])], 1) for k in u}
    flat = {k: v.reshape((-1,) + tuple(per[k].shape[1:])) for k, v in u.items()}
    xys, rand_inds = xys.reshape(-1, 1, 2), rand_inds.reshape(-1, 1)
    near_far = m.near_far[flat["frameid"].long()]
    rays = FD.raycast(xys, flat["Rmat"], flat["Tmat"], flat["Kinv"], near_far)
    FD.update_rays(m, rays, (2 if active else bs) > 1, flat["frameid"])
    ts = flat["frameid_sub"].float() / m.max_ts * 2 - 1
    rays["ts"] = ts[:, None, None].repeat(1, 1, 1)
    rays["vid_code"] = m.vid_code(flat["dataid"].long())[:, None].repeat(1, 1, 1)
    xysn = torch.cat([xys, torch.ones_like(xys[..., :1])], 2)
    rays["xysn"] = xysn.matmul(flat["Kinv"].permute(0, 2, 1))[..., :2]
    FD.update_delta_rts(m, rays)
    PL.obs_to_rays_line(rays, rand_inds, *obs, flat["batch_map"])
    return rand_inds, rays, flat["frameid"].cpu(), flat["errid"].cpu()


def child(a):
    import moda_amd
    from moda_amd import pixel_sampling as PS, synth
    from moda_amd.bench_support import DEV, T
    moda_amd.set_precision("fp32")
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, cases={})
    bs = 2 * P
    g = torch.Generator().manual_seed(0)
    cam = synth.make_cameras(5, bs)
    Rmat, Tmat, Kinv = T(cam["Rmat"]), T(cam["Tmat"]), T(cam["Kinv"])
    ids = {k: torch.randint(0, hi, (bs,), generator=g).to(DEV) for k, hi in
           (("dataid", 2), ("frameid", N_FRAMES), ("lineid", W), ("errid", N_FRAMES * W))}
    obs = [torch.rand((bs, c, W, 1), generator=g).to(DEV) for c in (3, 1, 1, 2, 1, 16)]
    for nsample, active in CASES:
        m = make_model(active)
        rand = torch.randint(0, W, (bs, 5 * nsample), generator=g).to(DEV)
        new = lambda: PS.sample_pxs(m, bs, nsample, Rmat, Tmat, Kinv, ids["dataid"], ids["frameid"], ids["frameid"], ids["frameid"],
                                    ids["lineid"], ids["errid"], *obs, rand_inds=rand)
        old = lambda: reference_route(m, bs, nsample, Rmat, Tmat, Kinv, ids["dataid"], ids["frameid"], ids["frameid"], ids["lineid"],
                                      ids["errid"], obs, rand, active)
        with torch.no_grad():
            r_new, r_old = new(), old()
            same = bool(torch.equal(r_new[0], r_old[0]) and torch.equal(r_new[1]["feats_at_samp"], r_old[1]["feats_at_samp"]))
            t_new, t_old = timed(new, a.reps), timed(old, a.reps)
            n_new, n_old = launches(new), launches(old)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                new()
            t_graph = timed(graph.replay, a.reps)
        res["cases"][f"nsample{nsample}_{'active' if active else 'plain'}"] = dict(
            new_eager_ms=t_new, new_graph_ms=t_graph, torch_route_ms=t_old, ratio_torch_over_new=t_old / t_new, launches_new=n_new,
            launches_torch_route=n_old, rays=int(r_new[0].shape[0]), same_pixels_as_torch_route=same)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pxs", "sample_pxs_bench.json"))
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    runs = []
    for k in range(a.procs):                          # one fresh process per run, one after the other; stop at the first failure
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"run {k} failed with {p.returncode}")
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(k, json.dumps({c: [round(r["new_eager_ms"], 3), round(r["new_graph_ms"], 3), round(r["torch_route_ms"], 3)]
                             for c, r in runs[-1]["cases"].items()}), flush=True)
    ratios = {c: [r["cases"][c]["ratio_torch_over_new"] for r in runs] for c in runs[0]["cases"]}
    worst = min(min(v) for v in ratios.values())
    res = dict(device=runs[0]["device"], reps=a.reps, procs=a.procs, shape=dict(P=P, W=W, use_embed=True), runs=runs,
               gate=dict(condition="the eager new route takes no longer than the torch route in every case in every process",
                         ratios_torch_over_new=ratios, min_ratio=worst, ok=worst >= 1.0))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res["gate"]))
    if not res["gate"]["ok"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
