"""Generate tests/golden/g37_nvs.npz by running the reference's own sample_xy, K2inv and raycast (nnutils/geom_utils.py),
composed as scripts/visualize/nvs.py:41-55 construct_rays_nvs composes them, on the CPU (development container only, like
gen_golden_warmup.py).  nvs.py itself imports absl, cv2, imageio and the trainer at module level, so its ten-line function is
replayed here statement by statement; every function it calls is the reference's.  Inputs and outputs only.

Three frames of 24 x 24: one mask empty, one full, one a disc; each frame is one reference call (the reference takes one mask),
the records are the calls' outputs concatenated in frame order.

Keys: img_size, rtks (3,4,4), near_far (3,2), masks (3,24,24) fp32, counts (3), and per tag t in (nf, auto) -- near_far given /
None -- t/rays_o, t/rays_d (n,3), t/near, t/far (n,1), t/rtk_vec (n,21), t/xys (n,2).

    python tests/golden/gen_golden_nvs.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402

S = 24
KEYS = ("rays_o", "rays_d", "near", "far", "rtk_vec", "xys")


def cameras(rng, B):
    """(B,4,4) fp32: a rotation about a seeded axis, a translation in front of the camera, an intrinsics row."""
    rtks = np.zeros((B, 4, 4), np.float32)
    for b in range(B):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        a = rng.uniform(0.2, 1.2)
        Kx = np.asarray([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        rtks[b, :3, :3] = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
        rtks[b, :3, 3] = [rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.8, 1.6)]
        rtks[b, 3] = [rng.uniform(20, 40), rng.uniform(20, 40), S / 2 + rng.uniform(-2, 2), S / 2 + rng.uniform(-2, 2)]
    return rtks


def main():
    _, _, geom, _ = _ref_import.import_reference()
    rng = np.random.default_rng(37)
    B = 3
    rtks = cameras(rng, B)
    near_far = np.stack([rng.uniform(0.3, 0.6, B), rng.uniform(1.8, 2.4, B)], 1).astype(np.float32)
    yy, xx = np.mgrid[:S, :S]
    masks = np.zeros((B, S, S), np.float32)
    masks[1] = 1
    masks[2] = ((xx - 11.3) ** 2 + (yy - 12.6) ** 2 < 8.2 ** 2).astype(np.float32)
    out = {"img_size": np.int64(S), "rtks": rtks, "near_far": near_far, "masks": masks, "counts": (masks > 0).sum((1, 2))}
    for tag, nf_all in (("nf", torch.from_numpy(near_far)), ("auto", None)):
        parts = {k: [] for k in KEYS}
        for i in range(B):                                                   # nvs.py:41-55, one frame a call
            r = torch.Tensor(rtks[i:i + 1])
            rndmask = torch.Tensor(masks[i]).view(-1) > 0
            _, xys = geom.sample_xy(S, 1, 0, "cpu", return_all=True)
            xys = xys[:, rndmask]
            rays = geom.raycast(xys, r[:, :3, :3], r[:, :3, 3], geom.K2inv(r[:, 3]), None if nf_all is None else nf_all[i:i + 1])
            assert rays["nsample"] == int(out["counts"][i]) and rays["bs"] == 1
            for k in KEYS:
                parts[k].append(rays[k].reshape(rays["nsample"], rays[k].shape[-1]).numpy())
        for k in KEYS:
            out[f"{tag}/{k}"] = np.concatenate(parts[k], 0).astype(np.float32)
    path = os.path.join(HERE, "g37_nvs.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items() if hasattr(v, "shape")})


if __name__ == "__main__":
    main()
