"""Frame-table timing (moda_amd/frame_state.py, csrc/frames_kernels.hip) against the reference's route restated in torch on the
same GPU, host round trips included: `.cpu().numpy()` of the pose table, the numpy patch of latest_vars['rtk'],
`torch.Tensor(...).to(device)` of rtk / idk, pts_to_view's chunks of 100 frames over a tiled copy of the points, obj_to_cam and
pinhole_cam as matmuls, max / min, and the two masked assignments (moda.py:485-491, geom_utils.py:1105-1155).  The baseline is
never this package's code.

  (a) the per-step reset, N = 8 box corners, M = 1024 frames: reset_near_far eager and replayed from a captured graph;
  (b) get_near_far with the points given as numpy, as reset_nf and nvs.py give them: N = 27 554, M = 1024 and N = 262 144, M = 64;
  (c) the captured TrainHarness step with nf_reset on and off: the difference of the medians beside each one's spread (max - min
      of the timed replays).  Recorded, not gated.

Median of --reps calls after warm-up, in each of --procs fresh processes, one after the other.  Gate for (a) and (b), a
condition and not a tuned figure: in EVERY case, in EVERY process, the eager new route takes no longer than the baseline.

  python tools/near_far_bench.py [--procs 3] [--reps 10] [--out profiles/frames/near_far_bench.json]"""
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

GNF_CASES = [(27554, 1024), (262144, 64)]          # (N, M)
RESET_M = 1024


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
    return float(np.median(ts)), float(max(ts) - min(ts))


def ref_get_near_far(near_far, vars_np, tol_fac=1.2, pts=None):
    """geom_utils.py:1105-1155 statement by statement in torch."""
    device = near_far.device
    rtk = torch.Tensor(vars_np['rtk']).to(device)
    idk = torch.Tensor(vars_np['idk']).to(device)
    out_pts = []
    for i in range(0, rtk.shape[0], 100):
        rtk_sub = rtk[i:i + 100]
        pts_sub = torch.Tensor(np.tile(pts[None], (len(rtk_sub), 1, 1))).to(device)
        verts = pts_sub.clone().matmul(rtk_sub[:, :3, :3].permute(0, 2, 1)) + rtk_sub[:, :3, 3].view(-1, 1, 3)
        K = rtk_sub[:, 3]
        Kmat = torch.zeros(K.shape[0], 3, 3, device=device)
        Kmat[:, 0, 0], Kmat[:, 1, 1], Kmat[:, 0, 2], Kmat[:, 1, 2], Kmat[:, 2, 2] = K[:, 0], K[:, 1], K[:, 2], K[:, 3], 1
        verts = verts.clone().matmul(Kmat.permute(0, 2, 1))
        z = verts[:, :, 2:3]
        out_pts.append(torch.cat([verts[:, :, :2] / (1e-6 + z), z], -1))
    p = torch.cat(out_pts, 0)
    pmax, pmin = p[..., -1].max(-1)[0], p[..., -1].min(-1)[0]
    delta = (pmax - pmin) * (tol_fac - 1)
    near, far = pmin - delta, pmax + delta
    near_far[idk == 1, 0] = torch.clamp(near[idk == 1], min=1e-3)
    near_far[idk == 1, 1] = torch.clamp(far[idk == 1], min=1e-3)
    return near_far


def ref_reset(near_far, latest_vars, rtk_all, corners):
    """moda.py:485-491."""
    rtk_np = rtk_all.clone().detach().cpu().numpy()
    valid_rts = latest_vars['idk'].astype(bool)
    latest_vars['rtk'][valid_rts, :3] = rtk_np[valid_rts]
    return ref_get_near_far(near_far, latest_vars, pts=corners)


def tables(M, rng):
    q, _ = np.linalg.qr(rng.standard_normal((M, 3, 3)))
    rtk = np.zeros((M, 4, 4), np.float32)
    rtk[:, :3, :3] = q
    rtk[:, :3, 3] = rng.standard_normal((M, 3)) * 0.3 + np.asarray([0, 0, 3.0])
    rtk[:, 3] = [400, 400, 256, 256]
    return rtk


def child(a):
    from moda_amd import frame_state as FS
    from moda_amd.bench_support import DEV, TrainHarness
    rng = np.random.default_rng(0)
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, cases={})
    # (a) the per-step reset
    M = RESET_M
    rtk = tables(M, rng)
    bounds = np.asarray([[-0.3, -0.2, -0.25], [0.3, 0.2, 0.25]])
    st = FS.FrameState.from_vars({"rtk": rtk, "idk": np.ones(M, np.float32),
                                  "mesh_rest": types.SimpleNamespace(bounds=bounds, vertices=np.zeros((8, 3)))}, None, DEV)
    model = types.SimpleNamespace(latest_vars=st, near_far=st.near_far)
    rtk_all = torch.from_numpy(tables(M, rng)[:, :3]).to(DEV)
    corners = FS.box_corners(bounds)
    lv = {"rtk": rtk.astype(np.float64), "idk": np.ones(M)}
    nf_ref = torch.zeros(M, 2, device=DEV)
    new = lambda: FS.reset_near_far(model, rtk_all)
    old = lambda: ref_reset(nf_ref, lv, rtk_all, corners)
    new(), old()
    err = float((st.near_far - nf_ref).abs().max())
    (t_new, _), (t_old, _) = timed(new, a.reps), timed(old, a.reps)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        new()
    t_graph, _ = timed(graph.replay, a.reps)
    res["cases"][f"reset_N8_M{M}"] = dict(new_eager_ms=t_new, new_graph_ms=t_graph, torch_route_ms=t_old, ratio_torch_over_new=t_old / t_new,
                                          max_abs_diff_to_torch_route=err)
    # (b) get_near_far from numpy points
    for N, M in GNF_CASES:
        rtk = tables(M, rng)
        pts = (rng.standard_normal((N, 3)) * 0.3).astype(np.float32)
        st = FS.FrameState.from_vars({"rtk": rtk, "idk": np.ones(M, np.float32)}, None, DEV)
        lv = {"rtk": rtk, "idk": np.ones(M)}
        nf_ref = torch.zeros(M, 2, device=DEV)
        new = lambda: FS.get_near_far(st.near_far, st, pts=pts)
        old = lambda: ref_get_near_far(nf_ref, lv, pts=pts)
        new(), old()
        err = float((st.near_far - nf_ref).abs().max())
        (t_new, _), (t_old, _) = timed(new, a.reps), timed(old, a.reps)
        res["cases"][f"get_near_far_N{N}_M{M}"] = dict(new_eager_ms=t_new, torch_route_ms=t_old, ratio_torch_over_new=t_old / t_new,
                                                       splits=FS.near_far_splits(N, M), max_abs_diff_to_torch_route=err)
        st.check()
    # (c) the captured harness step, nf_reset on against off
    step = {}
    for on in (False, True):
        h = TrainHarness(default_losses=True, root_pose=True, nf_reset=on)
        h.capture()
        step["on" if on else "off"] = timed(h.step, a.reps)
        del h
        torch.cuda.empty_cache()
    res["harness_step"] = dict(off_ms=step["off"][0], off_spread_ms=step["off"][1], on_ms=step["on"][0], on_spread_ms=step["on"][1],
                               difference_ms=step["on"][0] - step["off"][0])
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames", "near_far_bench.json"))
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
        print(k, json.dumps({c: [round(v, 3) for key, v in r.items() if key.endswith("_ms")] for c, r in runs[-1]["cases"].items()}),
              json.dumps({k2: round(v, 3) for k2, v in runs[-1]["harness_step"].items()}), flush=True)
    ratios = {c: [r["cases"][c]["ratio_torch_over_new"] for r in runs] for c in runs[0]["cases"]}
    worst = min(min(v) for v in ratios.values())
    res = dict(device=runs[0]["device"], reps=a.reps, procs=a.procs, runs=runs,
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
