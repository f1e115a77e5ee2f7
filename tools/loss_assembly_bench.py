"""Time the loss stage with the reference's default flags (loss_flt, rm_novp) on the training shape: 2048 rays, 1000 frames x 512
lines.  Two comparisons, one JSON line:

  stage   the reference's route restated in torch -- the filter through `.cpu().numpy()` as nnutils/loss_utils.py:432-445 writes
          it, boolean gathers per term as nnutils/moda.py:540-642 -- against moda_amd.loss_utils.forward_loss, forward + backward;
  step    the captured TrainHarness step with default_losses on and off.

Medians of synchronised repetitions after a warm-up; run it twice and report both (DESIGN section 5 on spread).

    python tools/loss_assembly_bench.py [--reps 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from moda_amd import loss_utils as LU  # noqa: E402
from moda_amd.bench_support import TrainHarness  # noqa: E402

N, FRAMES, LINES = 2048, 1000, 512
OPTS = dict(bone_loc_reg=0.0, root_sm=False, lineload=True)


def make_rendered(dev, seed=0):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    r = lambda *sh: torch.rand(sh, device=dev, generator=g)
    rendered = dict(img_loss_samp=r(N, 3), sil_loss_samp=r(N, 1), frnd_loss_samp=r(N, 1), flo_loss_samp=r(N, 1), feat_err=r(N, 1),
                    proj_err=r(N, 1), frame_cyc_dis=r(N), vis_loss=r(), sil_coarse=r(N, 1), sil_at_samp=(r(N, 1) > 0.3).float(),
                    vis_at_samp=(r(N, 1) > 0.1).float(), sil_at_samp_flo=r(N, 1) > 0.5)
    for k in ("img_loss_samp", "sil_loss_samp", "frnd_loss_samp", "flo_loss_samp", "feat_err", "proj_err", "frame_cyc_dis", "vis_loss"):
        rendered[k].requires_grad_(True)
    frame = torch.randint(0, FRAMES, (N // 4,), device=dev, generator=g).repeat_interleave(4)
    errid = frame * LINES + torch.randint(0, LINES, (N // 4,), device=dev, generator=g).repeat_interleave(4)
    return rendered, errid, frame


def torch_route(rendered, errid, frameid, sil_err):
    """moda.py:522-642 with the default flags as the reference writes it (its own weights)."""
    o = LU.LOSS_OPTS
    v = (rendered["sil_loss_samp"] * o["sil_wt"]).detach().cpu().numpy().reshape(-1)          # loss_utils.py:437
    e, f = errid.cpu().numpy(), frameid.cpu().numpy()
    sil_err[e] = v
    rows = sil_err.reshape(-1, LINES)
    mean = rows.sum(-1) / (1e-9 + (rows > 0).astype(float).sum(-1))
    invalid = torch.from_numpy((mean > np.median(mean[mean > 0]) * 10)[f]).to(errid.device)
    n_removed = int(invalid.sum())                                                            # the print of moda.py:537-538
    sil, sc = rendered["sil_at_samp"], rendered["sil_coarse"].detach()
    keep = (~invalid)[:, None].float()
    total = ((rendered["img_loss_samp"] * o["img_wt"] * keep) * sc)[sil[..., 0] > 0].mean()
    total = total + (rendered["sil_loss_samp"] * keep * o["sil_wt"])[rendered["vis_at_samp"] > 0].mean()
    total = total + ((rendered["frnd_loss_samp"] * o["frnd_wt"] * keep) * sc)[sil > 0].mean()
    total = total + ((rendered["flo_loss_samp"] * keep) * sc)[rendered["sil_at_samp_flo"]].mean() * 2 * o["flow_wt"]
    total = total + ((rendered["feat_err"] * o["feat_wt"] * keep) * sc)[sil > 0].mean()
    total = total + (rendered["proj_err"] * o["proj_wt"] * keep)[sil > 0].mean()
    total = total + rendered["frame_cyc_dis"].mean() * o["cyc_wt"] + 0.01 * rendered["vis_loss"].mean()
    return total, n_removed


def median_ms(fn, reps, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.sort(np.asarray(ts))
    return dict(median_ms=round(float(np.median(ts)), 4), p10_ms=round(float(ts[len(ts) // 10]), 4), p90_ms=round(float(ts[(9 * len(ts)) // 10]), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda")
    rendered, errid, frameid = make_rendered(dev)
    leaves = [t for t in rendered.values() if t.requires_grad]
    flt = LU.LossFilter(FRAMES, LINES)
    sil_err = np.zeros(FRAMES * LINES)

    def ours():
        for t in leaves:
            t.grad = None
        LU.forward_loss(rendered, OPTS, loss_filter=flt, errid=errid, frameid=frameid, progress=1.0)[0].backward()

    def theirs():
        for t in leaves:
            t.grad = None
        torch_route(rendered, errid, frameid, sil_err)[0].backward()

    out = {"shape": {"rays": N, "frames": FRAMES, "lines": LINES}, "reps": a.reps,
           "stage_torch_route": median_ms(theirs, a.reps), "stage_forward_loss": median_ms(ours, a.reps)}
    for name, on in (("step_default_losses_off", False), ("step_default_losses_on", True)):
        h = TrainHarness(N=2048, S=128, precision="bf16", default_losses=on)
        h.capture(warm=3)
        out[name] = median_ms(h.step, a.reps, warm=5)
        del h
    print(json.dumps(out))


if __name__ == "__main__":
    main()
