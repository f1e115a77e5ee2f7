"""Frame-pair preparation timing (moda_amd/frame_pairs.py, csrc/framepair_kernels.hip): prepare_frame_pairs at the reference's
size -- img_size 512, source frames 1080 x 1920, bs = 4 pairs -- against what torch alone offers on the same GPU for the same
work: boolean reductions for the box, the crop parameters as small tensor operations, F.grid_sample per plane (bilinear for img
and flow, nearest for mask, dp and the all-ones plane), the flow re-expression and the forward-backward check by a second
F.grid_sample, then the same tail as the product (F.normalize, cse.resample_dp, the pair-major reordering).  The torch side is a
baseline for time, not a restatement of cv2.remap: grid_sample has no 1/32 lattice.
Each of --procs fresh processes, one after the other: warm-up, then the median of --reps synchronised calls per side.
Gate, a condition and not a tuned figure: in EVERY process the product takes no longer than the torch route.
Also recorded: the time of the four frame-pair launches alone (the tail left out) and the bytes per second they reach against
what they must move: the masks once, the crop's footprint of every source plane once, every output plane once, the cropped
flow written and read back once.

  python tools/frame_pairs_bench.py [--procs 3] [--reps 10] [--out profiles/framepairs/frame_pairs_bench.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

H, W, S, BS = 1080, 1920, 512, 4


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


def make_raw(g):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    masks, flows = [], []
    for f in range(2 * BS):
        cy, cx = H * (0.45 + 0.02 * f), W * (0.42 + 0.02 * f)
        masks.append(((((yy - cy) / (0.33 * H)) ** 2 + ((xx - cx) / (0.2 * W)) ** 2) < 1).to(torch.uint8))
        sign = 1.0 if f % 2 == 0 else -1.0
        flows.append(torch.stack([sign * (6 + 2 * torch.sin(yy / 90)), sign * (-4 + 2 * torch.cos(xx / 70))], -1)
                     + 0.2 * torch.randn((H, W, 2), generator=g))
    lead = (BS, 2)
    return {"img": torch.randint(0, 256, lead + (H, W, 3), generator=g, dtype=torch.uint8).cuda(),
            "mask": torch.stack(masks).view(*lead, H, W).cuda(), "flow": torch.stack(flows).view(*lead, H, W, 2).cuda(),
            "occ": torch.rand(lead + (H, W), generator=g).cuda(),
            "dp": torch.randint(0, 27554, lead + (H, W), generator=g, dtype=torch.int32).cuda(),
            "dp_feat": torch.randn(lead + (16, 112, 112), generator=g).cuda(),
            "dp_bbox": torch.tensor([500.0, 200.0, 1400.0, 900.0]).repeat(BS, 2, 1).cuda(),
            "rtk": torch.randn(lead + (4, 4), generator=g).cuda(), "dataid": torch.zeros(lead, dtype=torch.int64).cuda(),
            "frameid": torch.arange(2 * BS).view(lead).cuda()}


def torch_route(raw, cse):
    """The same batch with torch operations alone (device tensors, no read-back)."""
    B = 2 * BS
    pm = lambda t: t.transpose(0, 1).reshape(B, *t.shape[2:])
    on = pm(raw["mask"]) > 0
    cols, rows = on.any(1), on.any(2)
    first = lambda t: t.to(torch.uint8).argmax(1)
    last = lambda t: t.shape[1] - 1 - t.flip(1).to(torch.uint8).argmax(1)
    x0, x1, y0, y1 = first(cols), last(cols), first(rows), last(rows)
    cx, cy = (x1 + x0) // 2, (y1 + y0) // 2
    lx = (1.2 * ((x1 - x0) // 2).double()).long()
    ly = (1.2 * ((y1 - y0) // 2).double()).long()
    aff = torch.stack([2 * lx.double() / S, 2 * ly.double() / S, (cx - lx).double(), (cy - ly).double()], 1)
    kaug = aff.float()
    ar = torch.arange(S, device=on.device, dtype=torch.float64)
    px = (ar[None, :] * aff[:, 0:1] + aff[:, 2:3])                          # (B, S) source x
    py = (ar[None, :] * aff[:, 1:2] + aff[:, 3:4])
    grid = torch.stack([((2 * px + 1) / W - 1)[:, None, :].expand(B, S, S), ((2 * py + 1) / H - 1)[:, :, None].expand(B, S, S)], -1).float()
    img = F.grid_sample(pm(raw["img"]).permute(0, 3, 1, 2).float() / 255, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    flow = F.grid_sample(pm(raw["flow"]).permute(0, 3, 1, 2), grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    near = torch.stack([on.float(), pm(raw["dp"]).float(), torch.ones_like(on, dtype=torch.float32)], 1)
    near = F.grid_sample(near, grid, mode="nearest", padding_mode="zeros", align_corners=False)
    vis = near[:, 2]
    masks = ((near[:, 0] * vis) > 0).float()
    # flow_process: the flow in the other frame's crop, the check through a second grid_sample
    other = torch.cat([aff[BS:], aff[:BS]])
    pos = torch.stack([ar[None, None, :].expand(B, S, S), ar[None, :, None].expand(B, S, S)], 1)
    hp = torch.stack([px[:, None, :].expand(B, S, S), py[:, :, None].expand(B, S, S)], 1)
    fs = ((flow.double() + hp - other[:, 2:, None, None]) / other[:, :2, None, None] - pos).float()
    warped = pos + torch.cat([fs[BS:], fs[:BS]]).double()
    g2 = ((2 * (pos.float() + fs) + 1) / S - 1).permute(0, 2, 3, 1)
    dis = (F.grid_sample(warped.float(), g2, mode="bilinear", padding_mode="zeros", align_corners=False) - pos).norm(2, 1)
    occ = torch.exp(-25 * (dis / S * 2))
    occ = torch.where(occ < 0.25, torch.zeros_like(occ), occ)
    rtk = pm(raw["rtk"].float()).contiguous()
    dp_bbox = pm(raw["dp_bbox"].float()).contiguous()
    feats = F.normalize(pm(raw["dp_feat"]).contiguous(), 2, 1)
    return {"imgs": img, "masks": masks, "vis2d": vis, "dps": near[:, 1], "flow": 2 * (fs / S), "occ": occ, "rtk": rtk,
            "rt_raw": rtk[:, :3].clone(), "kaug": kaug, "dp_feats": feats, "dp_feats_rsmp": cse.resample_dp(feats, dp_bbox, kaug, S),
            "dataid": pm(raw["dataid"]), "frameid": pm(raw["frameid"])}


def child(a):
    import moda_amd  # noqa: F401
    from moda_amd import cse, frame_pairs as FP
    raw = make_raw(torch.Generator().manual_seed(35))
    B = 2 * BS
    t_k = timed(lambda: FP.prepare_frame_pairs(raw, S), a.reps)
    t_t = timed(lambda: torch_route(raw, cse), a.reps)

    def launches():
        kaug, aff, _ = FP.compute_crop_params(raw["mask"], S, pair_major=True)
        crop = FP.crop_frames(aff, S, img=raw["img"], flow=raw["flow"], mask=raw["mask"], dp=raw["dp"], pair_major=True)
        return FP.flow_process(crop["flow"], aff, S)

    t_l = timed(launches, a.reps)
    out, ref = FP.prepare_frame_pairs(raw, S), torch_route(raw, cse)
    aff = FP.compute_crop_params(raw["mask"], S, pair_major=True)[1].cpu().numpy()
    foot = float(sum(min(W, a0 * S) * min(H, a1 * S) for a0, a1 in aff[:, :2]))      # source pixels under the crops
    must = B * H * W * 1 + foot * (3 + 8 + 1 + 4) + B * S * S * 4 * (3 + 1 + 1 + 1 + 2 + 1) + 2 * B * S * S * 2 * 4
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, shape=dict(bs=BS, h=H, w=W, img_size=S),
               moda_ms=t_k, torch_ms=t_t, ratio_torch_over_moda=t_t / t_k, moda_frame_pair_launches_ms=t_l,
               must_move_bytes=must, achieved_bytes_per_s=must / (t_l * 1e-3), status=out["status"].tolist(),
               kaug_equal=bool(torch.equal(out["kaug"], ref["kaug"])), vis2d_agreement=float((out["vis2d"] == ref["vis2d"]).float().mean()),
               img_mean_abs_difference=float((out["imgs"] - ref["imgs"]).abs().mean()),
               occ_mean_abs_difference=float((out["occ"] - ref["occ"]).abs().mean()),
               note="the differences are between cv2.remap's 1/32 lattice and grid_sample's exact weights, not errors of either")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "framepairs", "frame_pairs_bench.json"))
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
        print(k, json.dumps({n: round(runs[-1][n], 3) for n in ("moda_ms", "torch_ms", "moda_frame_pair_launches_ms")}), flush=True)
    ratios = [r["ratio_torch_over_moda"] for r in runs]
    res = dict(device=runs[0]["device"], reps=a.reps, procs=a.procs, runs=runs,
               gate=dict(condition="prepare_frame_pairs is no slower than the torch route in every process",
                         ratios_torch_over_moda=ratios, min_ratio=min(ratios), ok=min(ratios) >= 1.0))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res["gate"]))
    if not res["gate"]["ok"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
