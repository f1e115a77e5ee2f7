"""Generate tests/golden/g30_loss_assembly.npz by running the reference's own loss-stage functions on the CPU (development
container only, like gen_golden.py): loss_filter_line and loss_filter (nnutils/loss_utils.py:432-476) over three consecutive
calls on one state, compute_root_sm_2nd_loss (:486-517) and rot_angle (nnutils/geom_utils.py:1196-1205) with loss and
gradient in fp32 and in float64.  Inputs and outputs only.

The filter inputs are multiples of 2^-10 below 2^4, so every sum is exact in any order and in either precision: the recorded
flags do not depend on the reference's summation order.  nnutils/moda.py cannot be imported here (absl flags, mcubes,
torchvision, pytorch3d), so the assembly of moda.py:517-768 is restated (tests/lossasm_numpy.py) and not recorded.

    python tests/golden/gen_golden_lossasm.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from _ref_import import import_reference  # noqa: E402


def dyadic(rng, shape, hi=16.0):
    return (rng.integers(0, int(hi * 1024), size=shape) / 1024.0).astype(np.float32)


def rotations(rng, n, step):
    """n rotation matrices, a random walk of axis-angle steps of about `step` radians (Rodrigues, float64 -> fp32)."""
    out, R = [], np.eye(3)
    for _ in range(n):
        w = rng.normal(size=3) * step
        th = np.linalg.norm(w)
        k = w / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = R @ (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K)
        out.append(R.copy())
    return np.stack(out)


def main():
    _, _, geom, _ = import_reference()
    import importlib
    lu = importlib.import_module("nnutils.loss_utils")
    for seed in range(30, 130):                       # the first seed whose filter calls reject something, but not everything
        out = record(lu, geom, np.random.default_rng(seed))
        if all(out[k].any() and not out[k].all() for k in ("line1_invalid", "frame2_invalid")):
            break
    else:
        raise SystemExit("no seed gives a rejected frame")
    out["seed"] = np.asarray(seed)
    path = os.path.join(HERE, "g30_loss_assembly.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, seed", seed)


def record(lu, geom, rng):
    out = {}

    # loss_filter_line: 7 frames of 8 lines, 24 rays per call, every id repeated 2-4 times in shuffled order
    T, S, N = 7, 8, 24
    sil_err = np.zeros(T * S)
    for call in range(3):
        ids = rng.choice(T * S, size=8, replace=False)
        errid = np.concatenate([np.repeat(ids[:4], 2), np.repeat(ids[4:6], 4), np.repeat(ids[6:], 4)])[:N]
        rng.shuffle(errid)
        frameid = errid // S
        vals = dyadic(rng, (N, 1))
        if call == 1:
            vals[errid // S == errid[0] // S] *= 64                     # one frame far above ten medians
        inv = lu.loss_filter_line(sil_err, errid, frameid, torch.from_numpy(vals), S)
        out.update({f"line{call}_errid": errid.astype(np.int64), f"line{call}_frameid": frameid.astype(np.int64),
                    f"line{call}_vals": vals, f"line{call}_invalid": np.asarray(inv), f"line{call}_state": sil_err.copy()})
    out["line_shape"] = np.asarray([T, S, N])

    # loss_filter + the update of moda.py:533: 9 frames, 5 rows of 6 rays
    T2, bs, n = 9, 5, 6
    hist = np.zeros(T2)
    for call in range(3):
        x = dyadic(rng, (bs, n, 1))
        if call == 2:
            x[3] *= 256
        m = rng.random((bs, n, 1)) > 0.3
        errid = rng.choice(T2, size=bs, replace=False)
        flo_err, inv = lu.loss_filter(hist, torch.from_numpy(x), torch.from_numpy(m))
        hist[errid] = flo_err
        out.update({f"frame{call}_x": x, f"frame{call}_mask": m, f"frame{call}_errid": errid.astype(np.int64),
                    f"frame{call}_flo_err": np.asarray(flo_err, np.float32), f"frame{call}_invalid": np.asarray(inv),
                    f"frame{call}_state": hist.copy()})

    # root smoothness: videos of 2, 3, 5 and 10 frames; one pair of identical poses (upper clamp) and one repeated translation step
    off = (0, 2, 5, 10, 20)
    rtk = np.zeros((off[-1], 4, 4), np.float32)
    rtk[:, :3, :3] = rotations(rng, off[-1], 0.3).astype(np.float32)
    rtk[:, :3, 3] = rng.normal(size=(off[-1], 3)).astype(np.float32)
    rtk[:, 3, 3] = 1
    rtk[12] = rtk[11]
    rtk[13] = rtk[11]
    for dt, name in ((torch.float32, "f32"), (torch.float64, "f64")):
        r = torch.from_numpy(rtk).to(dt).requires_grad_(True)
        loss = lu.compute_root_sm_2nd_loss(r, off)
        loss.backward()
        out["root_loss_" + name] = loss.detach().numpy()
        out["root_grad_" + name] = r.grad.numpy()
        mats = torch.from_numpy(rtk[:, :3, :3]).to(dt)
        out["rot_angle_" + name] = geom.rot_angle(mats[:-1].matmul(mats[1:].permute(0, 2, 1))).numpy()
    out["root_rtk"] = rtk
    out["root_offset"] = np.asarray(off)
    return out


if __name__ == "__main__":
    main()
