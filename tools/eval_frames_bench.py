"""Evaluation-frame timing (moda_amd/eval_frames.py, csrc/evalvis_kernels.hip): 9 frames in chunks of rnd_frame_chunk = 3,
render_size 64, the 8 x 256 coarse network with 25 bones, the skin and the feature networks, ndepth 64, in the library's
default precision -- against the reference's route (nnutils/train_utils.py:480-520, :612-622, utils/io.py:242-258) restated in
torch around the SAME render_rays: per chunk the in-place masking with one .max() / .min() host read per key, then per key
.cpu().numpy() and, for the flow keys, numpy flow_to_image per frame, `max() <= 1 -> * 255`, astype(uint8).
Each of --procs fresh processes, one after the other: warm-up, then the median of --reps synchronised calls per side.
Recorded per process: the whole call on both routes (render + canvases + 8-bit video frames of every key), the stage behind
render_rays alone on stored rendered chunks, kernel launches per call counted with torch's profiler, the share of the call that
is not render_rays, and whether the two routes' canvases agree to 1e-5 relative.  No gate: no speed is claimed in advance.

  python tools/eval_frames_bench.py [--procs 3] [--reps 10] [--out profiles/evalvis/eval_frames_bench.json]"""
import argparse
import importlib
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

FRAMES, STEP, S, NDEPTH, CHUNK, BONES, N_FRAMES = 9, 3, 64, 64, 32768, 25, 12


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


def numpy_flow_to_image(flow, wheel):
    """flowlib.flow_to_image restated for one (H, W, 2) frame, as numpy >= 2 runs it on an fp32 array."""
    u, v = flow[..., 0].copy(), flow[..., 1].copy()
    unknown = (abs(u) > 1e7) | (abs(v) > 1e7)
    u[unknown] = 0
    v[unknown] = 0
    maxrad = max(-1, np.max(np.sqrt(u ** 2 + v ** 2)))
    u, v = u / (maxrad + np.finfo(float).eps), v / (maxrad + np.finfo(float).eps)
    nan = np.isnan(u) | np.isnan(v)
    u[nan] = 0
    v[nan] = 0
    rad = np.sqrt(u ** 2 + v ** 2)
    fk = (np.arctan2(-v, -u) / np.pi + 1) / 2 * 54 + 1
    k0 = np.floor(fk).astype(int)
    k1 = k0 + 1
    k1[k1 == 56] = 1
    f = fk - k0
    img = np.zeros(u.shape + (3,))
    for i in range(3):
        col = (1 - f) * (wheel[k0 - 1, i] / 255) + f * (wheel[k1 - 1, i] / 255)
        idx = rad <= 1
        col[idx] = 1 - rad[idx] * (1 - col[idx])
        col[~idx] *= 0.75
        img[..., i] = np.uint8(np.floor(255 * col * (1 - nan)))
    img[unknown] = 0
    return np.uint8(img)


def make_scene():
    from moda_amd import synth, feeders as FD
    from moda_amd.bench_support import make_models, make_opts, DEV, T
    models, emb = make_models(17, BONES, with_skin=True, with_feat=True)
    model = types.SimpleNamespace(device=DEV, training=False, progress=0.5, img_size=S, max_ts=float(N_FRAMES), num_bone_used=BONES,
                                  nerf_models=models, embeddings=emb, embedding_xyz=emb["xyz"])
    model.opts = make_opts(dist_corresp=True, num_bones=BONES, ndepth=NDEPTH, chunk=CHUNK, perturb=0, noise_std=0.0, fine_steps=1.1,
                           rnd_frame_chunk=STEP, render_size=S, lineload=False, use_unc=False, use_embed=True, use_proj=True,
                           nactive=0.5, warmup_steps=0.2, flowbw=False, env_code=True, appearance_code=False)
    off = np.asarray([0, N_FRAMES])
    model.pose_code = FD.FrameCodeTable(N_FRAMES, 6, 128, off).to(DEV)
    model.env_code = FD.FrameCodeTable(N_FRAMES, 6, 64, off).to(DEV)
    head = FD.DQ_RTHead(use_quat=True, in_channels_xyz=128, in_channels_dir=0, out_channels=7 * BONES, raw_feat=True).to(DEV)
    with torch.no_grad():
        head.rgb[0].weight.mul_(0.05)
        head.rgb[0].bias.copy_(torch.tensor([0, 0, 0, 1, 0, 0, 0.0], device=DEV).repeat(BONES))
    model.nerf_body_rts = torch.nn.Sequential(model.pose_code, head)
    model.rest_pose_code = models["rest_pose_code"]
    model.near_far = T(np.stack([np.full(N_FRAMES, 0.6, np.float32), np.full(N_FRAMES, 1.4, np.float32)], 1))
    model.latest_vars = {"obj_bound": np.asarray([0.2, 0.2, 0.2], np.float32)}
    model.vis_min, model.vis_len = np.asarray([-0.2, -0.2, -0.2], np.float32), np.asarray([0.4, 0.4, 0.4], np.float32)
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[:S, :S]
    sil = ((xx - S / 2) ** 2 + (yy - S / 2) ** 2 < (0.36 * S) ** 2).astype(np.float32)
    obs_all = dict(imgs=rng.random((N_FRAMES, 3, S, S)), masks=np.tile(sil, (N_FRAMES, 1, 1)), vis2d=np.ones((N_FRAMES, S, S)),
                   flow=rng.standard_normal((N_FRAMES, 2, S, S)) * 0.05, occ=rng.random((N_FRAMES, S, S)),
                   dp_feats=rng.standard_normal((N_FRAMES, 16, S, S)))
    obs_all = {k: T(v.astype(np.float32)) for k, v in obs_all.items()}
    cam = synth.make_cameras(17, N_FRAMES)

    def set_input(m, idx):
        """What collate + set_input leave on the model: the frames of idx, then their pairs (the next frame)."""
        ids = torch.as_tensor(list(idx) + [(i + 1) % N_FRAMES for i in idx], device=DEV)
        bs = ids.shape[0]
        for k, v in obs_all.items():
            setattr(m, k, v[ids].contiguous())
        rtk = np.zeros((bs, 4, 4), np.float32)
        sel = ids.cpu().numpy()
        rtk[:, :3, :3], rtk[:, :3, 3] = cam["Rmat"][sel], cam["Tmat"][sel]
        rtk[:, 3] = [2.0 * S, 2.0 * S, S / 2, S / 2]
        m.rtk, m.kaug = T(rtk), T(np.tile(np.asarray([1, 1, 0, 0], np.float32), (bs, 1)))
        m.frameid = m.frameid_sub = m.embedid = ids
        m.dataid = torch.zeros_like(ids)
        m.errid, m.lineid = ids.clone(), None

    return model, set_input, DEV


def restated_canvases(rendered, model, opts):
    """train_utils.py:496-520 as written: in place, every `.max()` / `.min()` a 0-dim tensor that `255 / t` reads on the host."""
    hbs = next(iter(rendered.values())).shape[0]
    sil = torch.nn.functional.interpolate(model.masks[:hbs, None], (opts.render_size, opts.render_size))[:, 0, ..., None]
    r = {k: v.clone() for k, v in rendered.items() if k not in ("dis_reg", "dis_reg_forward")}
    r["flo_coarse"] *= sil
    r["img_loss_samp"] *= sil
    if "frame_cyc_dis" in r:
        r["frame_cyc_dis"] *= 255 / r["frame_cyc_dis"].max()
    r["pts_pred"] *= sil
    r["pts_exp"] *= r["sil_coarse"]
    for k in ("feat_err", "proj_err"):
        r[k] *= sil
        r[k] *= 255 / r[k].max()
    return r


def restated_video(seq, wheel, flow_tags):
    """eval():612-622 + save_vid up to the uint8 frame: .cpu().numpy() per key, numpy per frame."""
    out = {}
    for k, v in seq.items():
        frames = v.cpu().numpy()
        up = min(30, len(frames))
        res = []
        for i in range(int(up)):
            frame = frames[int(i / up * len(frames))]
            if k in flow_tags:
                frame = numpy_flow_to_image(frame, wheel)
            if frame.max() <= 1:
                frame = frame * 255
            with np.errstate(invalid="ignore"):
                res.append(frame.astype(np.uint8))
        out[k] = np.stack(res)
    return out


def child(a):
    import moda_amd
    EF = importlib.import_module("moda_amd.eval_frames")
    model, set_input, dev = make_scene()
    opts = model.opts
    frames = list(range(FRAMES))
    wheel = EF.color_wheel()
    chunks = [frames[j:j + STEP] for j in range(0, FRAMES, STEP)]

    def render_chunk(idx):
        set_input(model, idx)
        return {k: v[:len(idx)] for k, v in EF.render_vid(model).items()}

    def device_back(stored):
        status = EF.new_status(dev)
        seq = {}
        for idx, rendered in zip(chunks, stored):
            set_input(model, idx)
            for k, v in EF.eval_canvases(rendered, model, opts, status=status)[0].items():
                seq.setdefault(k, []).append(v)
        ef = EF.EvalFrames({k: torch.cat(v, 0) for k, v in seq.items()}, status)
        return ef, {k: ef.video(k) for k in ef.rendered_seq}

    def torch_back(stored):
        seq = {}
        for idx, rendered in zip(chunks, stored):
            set_input(model, idx)
            for k, v in restated_canvases(rendered, model, opts).items():
                seq.setdefault(k, []).append(v)
        seq = {k: torch.cat(v, 0) for k, v in seq.items()}
        return seq, restated_video(seq, wheel, EF.FLOW_TAGS)

    render_all = lambda: [render_chunk(idx) for idx in chunks]
    stored = render_all()
    device_route = lambda: device_back(render_all())
    torch_route = lambda: torch_back(render_all())
    res = {"render_only_ms": timed(render_all, a.reps), "device_ms": timed(device_route, a.reps), "torch_ms": timed(torch_route, a.reps),
           "device_back_ms": timed(lambda: device_back(stored), a.reps), "torch_back_ms": timed(lambda: torch_back(stored), a.reps),
           "device_launches": count_launches(device_route), "torch_launches": count_launches(torch_route),
           "device_back_launches": count_launches(lambda: device_back(stored)), "torch_back_launches": count_launches(lambda: torch_back(stored))}
    res["device_share_not_render"] = 1 - res["render_only_ms"] / res["device_ms"]
    res["torch_share_not_render"] = 1 - res["render_only_ms"] / res["torch_ms"]
    ef, _ = device_back(stored)
    ref, _ = torch_back(stored)
    worst = 0.0
    for k in ("flo_coarse", "img_loss_samp", "pts_pred", "pts_exp", "feat_err", "proj_err"):
        d, r = ef.rendered_seq[k].double(), ref[k].double()
        worst = max(worst, float(((d - r).abs() / r.abs().clamp_min(1e-6)).max()))
    res["canvases_worst_rel_diff"] = worst
    res["canvases_agree"] = bool(worst < 1e-5)
    res["status"] = ef.status.cpu().tolist()
    res["keys"] = sorted(ef.rendered_seq)
    res["precision"] = moda_amd.get_precision()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evalvis", "eval_frames_bench.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for _ in range(a.procs):                      # fresh processes, one after the other
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)], capture_output=True, text=True)
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
        if out.returncode != 0 or not line:
            print(out.stdout[-2000:], out.stderr[-4000:], file=sys.stderr)
            raise SystemExit(f"a child process failed with code {out.returncode}")
        runs.append(json.loads(line[-1][7:]))
    spread = lambda k: [min(r[k] for r in runs), max(r[k] for r in runs)]
    summary = {"case": dict(frames=FRAMES, rnd_frame_chunk=STEP, render_size=S, ndepth=NDEPTH, bones=BONES), "procs": a.procs, "reps": a.reps,
               "spread": {k: spread(k) for k in ("render_only_ms", "device_ms", "torch_ms", "device_back_ms", "torch_back_ms",
                                                 "device_share_not_render", "torch_share_not_render")},
               "runs": runs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps(summary["spread"]))


if __name__ == "__main__":
    main()
