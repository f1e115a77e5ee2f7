"""DensePose-CSE matching timing (moda_amd/cse.py, csrc/cse_kernels.hip): ood_check_cse at N = 27554 and 5004 embedding rows,
112 x 112 features, bs = 1 and 8, and compute_flow_cse at 112 x 112, against two restatements in torch alone on the same GPU:
  reference   the reference's route: a host loop over frames, per frame chunks of rows whose (chunk, 16, h w) product is
              broadcast and summed (chunk = 5000 as in the reference, halved until the temporary is under 2 GB); for the flow
              the full (h w)^2 cost volume by matmul (the reference's 16 x (h w)^2 broadcast does not fit), reduced twice;
  matmul      the strongest plain-torch route: `matmul` in row chunks (the score chunk under 1 GB) followed by `argmax`.
Each of --procs fresh processes, one after the other: warm-up, then the median of --reps synchronised calls per side; the index
results of the kernel and of the matmul route are compared (agreement rate: they may differ only at near-ties).
Gate, a condition and not a tuned figure: at every size, in EVERY process, the kernel route takes no longer than the matmul route.
Also recorded: launches per call, and the share of the fp32 rate reached by the arg-max alone, 2 * 16 * N * M * B / time against
157 TFLOP/s.

  python tools/cse_match_bench.py [--procs 3] [--reps 10] [--out profiles/cse/cse_match_bench.json]"""
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

H = 112
OOD_SIZES = ((27554, 1), (27554, 8), (5004, 1), (5004, 8))
PEAK_FP32 = 157e12


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


def ood_tail(max_idx, dp_idx, h, w):
    """The rest of the reference's ood_check_cse after the arg-max, restated (device tensors, one frame)."""
    ar = torch.arange(w, device=max_idx.device, dtype=torch.float32)
    ref = torch.stack([ar[None, :].expand(h, w), ar[:, None].expand(h, w)], -1)
    rpj = max_idx[dp_idx]
    err = (torch.stack([rpj % w, rpj // w], -1) - ref).norm(2, -1)
    return err[dp_idx != 0].mean()


def ood_torch(dp_feats, dp_embed, dp_idx, route, chunk):
    bs, _, h, w = dp_feats.shape
    N = dp_embed.shape[0]
    dp_idx = torch.nn.functional.interpolate(dp_idx.float()[None], (h, w), mode='nearest').long()[0]
    errs, idxs = [], []
    for i in range(bs):
        max_idx = torch.zeros(N, device=dp_feats.device)
        for j in range(0, N, chunk):
            if route == "reference":
                cost = (dp_embed.view(N, 16, 1)[j:j + chunk] * dp_feats[i].view(1, 16, h * w)).sum(-2)
            else:
                cost = dp_embed[j:j + chunk] @ dp_feats[i].view(16, h * w)
            max_idx[j:j + chunk] = cost.argmax(-1)
        idxs.append(max_idx)
        errs.append(ood_tail(max_idx, dp_idx[i], h, w))
    errs = torch.stack(errs)
    return errs < 12, errs, torch.stack(idxs)


def flow_torch(a, b):
    cost = a.flatten(1).t() @ b.flatten(1)
    return cost.max(1)[1], cost.max(0)[1]


def child(a):
    import moda_amd
    from moda_amd import cse
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, sizes={})
    g = torch.Generator().manual_seed(34)
    unit = lambda t, d: t / t.norm(dim=d, keepdim=True)
    for N, bs in OOD_SIZES:
        feats = unit(torch.randn((bs, 16, H, H), generator=g), 1)
        feats[:, :, :20] = 0
        feats = feats.cuda()
        embed = unit(torch.randn((N, 16), generator=g), 1).cuda()
        dp_idx = torch.randint(0, N, (bs, H, H), generator=g).cuda()
        ref_chunk = 5000
        while ref_chunk * 16 * H * H * 4 > 2e9:
            ref_chunk //= 2
        mm_chunk = min(N, int(1e9 // (H * H * 4)))
        img = feats.view(bs, 16, H * H).transpose(1, 2)
        t_k = timed(lambda: cse.ood_check_cse(feats, embed, dp_idx), a.reps)
        t_a = timed(lambda: cse.feat_argmax(embed, img), a.reps)
        t_m = timed(lambda: ood_torch(feats, embed, dp_idx, "matmul", mm_chunk), a.reps)
        t_r = timed(lambda: ood_torch(feats, embed, dp_idx, "reference", ref_chunk), max(2, a.reps // 5), warm=1)
        vk, ek = cse.ood_check_cse(feats, embed, dp_idx)
        vm, em, im = ood_torch(feats, embed, dp_idx, "matmul", mm_chunk)
        ik = cse.feat_argmax(embed, img)
        splits, _ = cse.argmax_splits(bs, N, H * H)
        res["sizes"][f"ood_N{N}_bs{bs}"] = dict(
            moda_ms=t_k, moda_argmax_ms=t_a, torch_matmul_ms=t_m, torch_reference_ms=t_r, ratio_matmul_over_moda=t_m / t_k,
            ratio_reference_over_moda=t_r / t_k, launches=(3 if splits > 1 else 1) + 2 + 2, candidate_ranges=splits,
            fp32_share=2 * 16 * N * H * H * bs / (t_a * 1e-3) / PEAK_FP32, reference_chunk_rows=ref_chunk, matmul_chunk_rows=mm_chunk,
            index_agreement=float((ik == im.long()).float().mean()), max_error_difference=float((ek - em).abs().max()),
            valid_equal=bool(torch.equal(vk, vm)))
    fa = unit(torch.randn((16, H, H), generator=g), 0).cuda()
    fb = unit(torch.randn((16, H, H), generator=g), 0).cuda()
    warp = torch.tensor([[2.0, 0, 30.0], [0, 2.0, 40.0], [0, 0, 1]]).cuda()
    t_k = timed(lambda: cse.compute_flow_cse(fa, fb, warp, warp, 256), a.reps)
    t_a = timed(lambda: (cse.feat_argmax(fa.flatten(1).t(), fb.flatten(1).t()), cse.feat_argmax(fb.flatten(1).t(), fa.flatten(1).t())), a.reps)
    t_m = timed(lambda: flow_torch(fa, fb), a.reps)
    ma, mb = flow_torch(fa, fb)
    ka, kb = cse.feat_argmax(fa.flatten(1).t(), fb.flatten(1).t()), cse.feat_argmax(fb.flatten(1).t(), fa.flatten(1).t())
    P = H * H
    res["sizes"]["flow_112"] = dict(moda_ms=t_k, moda_argmax_ms=t_a, torch_matmul_ms=t_m, torch_reference_ms=t_m,
                                    ratio_matmul_over_moda=t_m / t_a, fp32_share=2 * 2 * 16 * P * P / (t_a * 1e-3) / PEAK_FP32,
                                    candidate_ranges=cse.argmax_splits(1, P, P)[0],
                                    note="the torch side is the two arg-max reductions alone, so the gate compares them with moda_argmax_ms",
                                    index_agreement=float(((ka == ma).float().mean() + (kb == mb).float().mean()) / 2))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cse", "cse_match_bench.json"))
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
        print(k, json.dumps({s: [round(r["moda_ms"], 3), round(r["torch_matmul_ms"], 3), round(r["torch_reference_ms"], 3)]
                             for s, r in runs[-1]["sizes"].items()}), flush=True)
    ratios = {s: [r["sizes"][s]["ratio_matmul_over_moda"] for r in runs] for s in runs[0]["sizes"]}
    worst = min(min(v) for v in ratios.values())
    res = dict(device=runs[0]["device"], reps=a.reps, procs=a.procs, runs=runs,
               gate=dict(condition="the kernel route is no slower than the torch matmul + argmax route at every size in every process",
                         ratios_matmul_over_moda=ratios, min_ratio=worst, ok=worst >= 1.0))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res["gate"]))
    if not res["gate"]["ok"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
